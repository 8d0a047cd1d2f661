/*
 * hc-mvs_amd/csrc/handoff_kernels.hip -- the hand-off between two levels of the coarse-to-fine schedule on the device (gfx950): the
 * previous level's depth and normal maps become the initial maps of a level (init mode, SceneDensify.cpp:527-553) or the extra
 * hypothesis of its last sweep (hint mode, restore/libs/MVS/SceneDensify.cpp:508-532).  The per-pixel arithmetic is handoff_device.h's,
 * shared with the host form.
 *
 * One launch serves a batch of items of mixed sizes: a workgroup finds its item by bisection in the prefix table of workgroup counts
 * and owns kHandoffChunk consecutive destination pixels of it, one pixel per thread and round.  A thread computes the coefficients of
 * its pixel once and resamples depth and the three normal channels with them; the 4 x 4 (2 x 2) source footprints of neighbouring
 * lanes overlap and come out of L2, the 16 B per destination pixel leave as plain stores: an HBM-streaming kernel.  The depth range
 * and the counters are reduced per wave (shuffles), then per workgroup through LDS, and leave the workgroup as ONE plain store of a
 * partial result; a second launch, one workgroup per item, reduces the item's partials into its result slot.  No atomics: the first
 * version sent an atomicMin, an atomicMax and three 64-bit atomicAdds per workgroup to the item's slot -- a thousand workgroups of
 * all eight XCDs on one cache line -- and took 5.2 ms where this one takes 1.9 ms (64 maps to 1080p).
 */
#include "handoff_kernels.h"

namespace hcmvs {
namespace {

constexpr int kRounds = 8;                                 // pixels per thread
constexpr int kWaves = kHandoffBlock / 64;
static_assert(kHandoffChunk == kHandoffBlock * kRounds, "a workgroup's pixels");

__device__ __forceinline__ int handoff_find(const int32_t* first, int n, int block) {
	int lo = 0, hi = n;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (first[mid] <= block) lo = mid; else hi = mid;
	}
	return lo;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
	return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
	return v;
}
__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}
template <int kMode>
__global__ __launch_bounds__(kHandoffBlock) void handoff_kernel(const HandoffItem* __restrict__ items, const int32_t* __restrict__ first, int nItems,
                                                                HandoffResult* partials) {
	const int q = handoff_find(first, nItems, (int)blockIdx.x);
	const HandoffItem it = items[q];
	const HandoffGeom& g = it.g;
	const int n = g.dw * g.dh; // < 2^29
	const int base = ((int)blockIdx.x - first[q]) * kHandoffChunk + (int)threadIdx.x;
	uint32_t lo = kMode == kHandoffInit ? 0x7F7FFFFFu : kHandoffKeyMinIdentity, hi = 0u, lastNaN = 0u;
	uint32_t nValid = 0, nClamped = 0, nRescaled = 0;
#pragma unroll 1
	for (int k = 0; k < kRounds; ++k) {
		const int idx = base + k * kHandoffBlock;
		if (idx >= n) break;
		const int y = idx / g.dw, x = idx - y * g.dw;
		HandoffPixel p;
		if (kMode == kHandoffInit) handoff_init_pixel(g, it.srcDepth, it.srcNormal, x, y, p);
		else handoff_hint_pixel(g, it.srcDepth, it.srcNormal, x, y, p);
		it.dstDepth[idx] = p.d;
		float* o = it.dstNormal + 3 * (size_t)idx;
		o[0] = p.n[0]; o[1] = p.n[1]; o[2] = p.n[2];
		if (kMode == kHandoffInit) { // cleaned depths are >= 0 and never NaN: their bits order like the floats
			const uint32_t b = __float_as_uint(p.d);
			lo = b < lo ? b : lo; hi = b > hi ? b : hi;
		} else if (p.raw != p.raw) {
			lastNaN = (uint32_t)idx + 1u; // ascending within a thread
		} else {
			const uint32_t b = handoff_order_key(p.raw);
			lo = b < lo ? b : lo; hi = b > hi ? b : hi;
		}
		nValid += p.valid ? 1u : 0u; nClamped += p.clamped ? 1u : 0u; nRescaled += p.rescaled ? 1u : 0u;
	}
	__shared__ uint32_t sLo[kWaves], sHi[kWaves], sNaN[kWaves], sValid[kWaves], sClamped[kWaves], sRescaled[kWaves];
	lo = wave_min(lo); hi = wave_max(hi); lastNaN = wave_max(lastNaN);
	nValid = wave_add(nValid); nClamped = wave_add(nClamped); nRescaled = wave_add(nRescaled);
	const int wave = (int)threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { sLo[wave] = lo; sHi[wave] = hi; sNaN[wave] = lastNaN; sValid[wave] = nValid; sClamped[wave] = nClamped; sRescaled[wave] = nRescaled; }
	__syncthreads();
	if (threadIdx.x != 0) return;
	for (int w = 1; w < kWaves; ++w) {
		lo = sLo[w] < lo ? sLo[w] : lo; hi = sHi[w] > hi ? sHi[w] : hi; lastNaN = sNaN[w] > lastNaN ? sNaN[w] : lastNaN;
		nValid += sValid[w]; nClamped += sClamped[w]; nRescaled += sRescaled[w];
	}
	HandoffResult r;
	r.lo = lo; r.hi = hi; r.lastNaN = lastNaN; r.tailHi = 0u;
	r.valid = nValid; r.clamped = nClamped; r.rescaled = nRescaled;
	partials[blockIdx.x] = r;
}

// After the pass, one workgroup per item: the partials of the item's workgroups become its result slot.  Hint mode: an item whose
// enlarged depth held a NaN then gets the fold over the pixels behind the last one (the largest of them, none of which is NaN), or NaN
// when there is none; the enlarged depth of those pixels is computed again.
template <int kMode>
__global__ __launch_bounds__(kHandoffBlock) void handoff_reduce_kernel(const HandoffItem* __restrict__ items, const int32_t* __restrict__ first,
                                                                       const HandoffResult* __restrict__ partials, HandoffResult* results) {
	const int q = (int)blockIdx.x;
	uint32_t lo = kMode == kHandoffInit ? 0x7F7FFFFFu : kHandoffKeyMinIdentity, hi = 0u, lastNaN = 0u;
	unsigned long long nValid = 0, nClamped = 0, nRescaled = 0;
	for (int b = first[q] + (int)threadIdx.x; b < first[q + 1]; b += kHandoffBlock) {
		const HandoffResult p = partials[b];
		lo = p.lo < lo ? p.lo : lo; hi = p.hi > hi ? p.hi : hi; lastNaN = p.lastNaN > lastNaN ? p.lastNaN : lastNaN;
		nValid += p.valid; nClamped += p.clamped; nRescaled += p.rescaled;
	}
	__shared__ uint32_t sLo[kWaves], sHi[kWaves], sNaN[kWaves];
	__shared__ unsigned long long sValid[kWaves], sClamped[kWaves], sRescaled[kWaves];
	lo = wave_min(lo); hi = wave_max(hi); lastNaN = wave_max(lastNaN);
	for (int o = 32; o > 0; o >>= 1) { nValid += __shfl_xor(nValid, o, 64); nClamped += __shfl_xor(nClamped, o, 64); nRescaled += __shfl_xor(nRescaled, o, 64); }
	const int wave = (int)threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { sLo[wave] = lo; sHi[wave] = hi; sNaN[wave] = lastNaN; sValid[wave] = nValid; sClamped[wave] = nClamped; sRescaled[wave] = nRescaled; }
	__syncthreads();
	for (int w = 0; w < kWaves; ++w) lastNaN = sNaN[w] > lastNaN ? sNaN[w] : lastNaN; // every thread: the tail below starts there
	if (threadIdx.x == 0) {
		lo = sLo[0]; hi = sHi[0]; nValid = sValid[0]; nClamped = sClamped[0]; nRescaled = sRescaled[0];
		for (int w = 1; w < kWaves; ++w) {
			lo = sLo[w] < lo ? sLo[w] : lo; hi = sHi[w] > hi ? sHi[w] : hi;
			nValid += sValid[w]; nClamped += sClamped[w]; nRescaled += sRescaled[w];
		}
		HandoffResult r;
		r.lo = lo; r.hi = hi; r.lastNaN = lastNaN; r.tailHi = 0u;
		r.valid = nValid; r.clamped = nClamped; r.rescaled = nRescaled;
		results[q] = r;
	}
	if (kMode != kHandoffHint || !lastNaN) return; // uniform over the workgroup
	const HandoffItem it = items[q];
	const int n = it.g.dw * it.g.dh;
	uint32_t tail = kHandoffKeyMaxIdentity;
	for (int idx = (int)lastNaN + (int)threadIdx.x; idx < n; idx += kHandoffBlock) {
		const int y = idx / it.g.dw, x = idx - y * it.g.dw;
		const uint32_t b = handoff_order_key(handoff_hint_raw_depth(it.g, it.srcDepth, x, y));
		tail = b > tail ? b : tail;
	}
	__shared__ uint32_t sTail[kWaves];
	tail = wave_max(tail);
	if ((threadIdx.x & 63) == 0) sTail[wave] = tail;
	__syncthreads();
	if (threadIdx.x != 0) return;
	for (int w = 0; w < kWaves; ++w) tail = sTail[w] > tail ? sTail[w] : tail;
	results[q].tailHi = tail == kHandoffKeyMaxIdentity ? 0x7FC00000u : __float_as_uint(handoff_key_value(tail));
}

} // namespace

void launch_handoff(int mode, const HandoffItem* items, const int32_t* first, int nItems, int nBlocks, HandoffResult* partials, HandoffResult* results,
                    hipStream_t s) {
	if (mode == kHandoffInit) {
		hipLaunchKernelGGL(handoff_kernel<kHandoffInit>, dim3((unsigned)nBlocks), dim3(kHandoffBlock), 0, s, items, first, nItems, partials);
		hipLaunchKernelGGL(handoff_reduce_kernel<kHandoffInit>, dim3((unsigned)nItems), dim3(kHandoffBlock), 0, s, items, first, partials, results);
	} else {
		hipLaunchKernelGGL(handoff_kernel<kHandoffHint>, dim3((unsigned)nBlocks), dim3(kHandoffBlock), 0, s, items, first, nItems, partials);
		hipLaunchKernelGGL(handoff_reduce_kernel<kHandoffHint>, dim3((unsigned)nItems), dim3(kHandoffBlock), 0, s, items, first, partials, results);
	}
}

} // namespace hcmvs

/*
 * hc-mvs_amd/csrc/speckle_kernels.hip -- the speckle filter on the device (gfx950): connected-component labelling of depth maps under
 * the edge rule of speckle_plan.h (section 3.5b), and the removal of the segments below speckle_size.
 *
 * A union-find over raster indices in which a parent is always the smaller index, so the root of a set is the smallest raster index in
 * it -- the canonical label -- and every link, made with atomicMin, only lowers a label: finds and unions of other threads may run at
 * the same time and may even read an older parent (it is still a member of the set, and still smaller).  Five launches, whatever the
 * maps hold, nothing read back in between; a workgroup owns one 64 x 16 tile of one map of the batch (a wave: one row of it) and finds
 * the map by bisection in the prefix table of tile counts.
 *   1 tile:   the tile's depths go to LDS, its right and down edges are united in LDS, every pixel's label becomes the tile-local root
 *             as a raster index of the map, and the pixel count of every tile-local component is left at its root (0 elsewhere).
 *   2 border: the pixels of a tile's top row and left column are united with their neighbours in the tile above / to the left, in
 *             global memory.  Only tile-local roots ever get a new parent.
 *   3 sizes:  every tile-local root finds its root, keeps it as its label and adds its count to the root's: one atomic per (tile,
 *             local component) -- a segment of a million pixels is a few thousand adds, not a million.
 *   4 apply:  a pixel's label is two loads away (its tile-local root, then that one's label); segments below speckle_size are cleared,
 *             the labels are written out where wanted, the counters leave the workgroup as one partial.
 *   5 sum:    one workgroup adds the partials up.
 * Every find and union loop is bounded by the map's pixel count, which no chain of strictly decreasing indices can exceed; a loop that
 * gets there raises the call's error word and gives up.
 */
#include "speckle_kernels.h"

namespace hcmvs {
namespace {

constexpr int kTilePixels = kSpeckleTileW * kSpeckleTileH;
constexpr int kRounds = kTilePixels / kSpeckleBlock;   // pixels per thread
constexpr int kWaves = kSpeckleBlock / 64;
constexpr int kBorderBlock = 128;                      // top row and left column of a tile: 64 + 16 threads at work
static_assert(kSpeckleTileW == 64, "a wave is one row of a tile");
static_assert(kTilePixels % kSpeckleBlock == 0, "whole rounds");
static_assert(kSpeckleTileW + kSpeckleTileH <= kBorderBlock, "one thread per border pixel");

__device__ __forceinline__ int speckle_find_item(const int32_t* first, int n, int block) {
	int lo = 0, hi = n;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (first[mid] <= block) lo = mid; else hi = mid;
	}
	return lo;
}

// the tile of this workgroup: its item and its origin in the map
struct Tile {
	int q, x0, y0;
};
__device__ __forceinline__ Tile speckle_tile(const SpeckleItem* items, const int32_t* first, int nItems, SpeckleItem& it) {
	Tile t;
	t.q = speckle_find_item(first, nItems, (int)blockIdx.x);
	it = items[t.q];
	const int k = (int)blockIdx.x - first[t.q];
	const int ty = k / it.tilesX, tx = k - ty * it.tilesX;
	t.x0 = tx * kSpeckleTileW; t.y0 = ty * kSpeckleTileH;
	return t;
}

__device__ __forceinline__ void raise_error(SpeckleResult* result) { atomicOr(&result->error, 1u); }

// ---- LDS --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root of x, or -1 past the bound
__device__ __forceinline__ int lds_find(const int* L, int x) {
	for (int k = 0; k <= kTilePixels; ++k) {
		const int p = lds_load(L + x);
		if (p == x) return x;
		x = p;
	}
	return -1;
}
__device__ __forceinline__ bool lds_union(int* L, int a, int b) {
	for (int k = 0; k <= kTilePixels; ++k) {
		a = lds_find(L, a); b = lds_find(L, b);
		if (a < 0 || b < 0) return false;
		if (a == b) return true;
		if (a < b) { const int t = a; a = b; b = t; }
		const int old = atomicMin(L + a, b); // a was a root when old == a: it now hangs below b
		if (old == a) return true;
		a = old;                             // someone else linked a in the meantime: go on from where it points (old < a)
	}
	return false;
}

// ---- global memory ------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t agent_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t global_find(const int32_t* L, int32_t x, int32_t n) {
	for (int32_t k = 0; k < n; ++k) { // a chain visits strictly decreasing indices of [0, n): at most n of them
		const int32_t p = agent_load(L + x);
		if (p == x) return x;
		if (p < 0 || p > x) return -1; // never a label of a valid pixel
		x = p;
	}
	return -1;
}
__device__ __forceinline__ bool global_union(int32_t* L, int32_t a, int32_t b, int32_t n) {
	for (int32_t k = 0; k < n; ++k) { // a failed link leaves a strictly smaller a
		a = global_find(L, a, n); b = global_find(L, b, n);
		if (a < 0 || b < 0) return false;
		if (a == b) return true;
		if (a < b) { const int32_t t = a; a = b; b = t; }
		const int32_t old = atomicMin(L + a, b);
		if (old == a) return true;
		if (old < 0 || old > a) return false;
		a = old;
	}
	return false;
}

// ---- 1: the tile --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpeckleBlock) void speckle_tile_kernel(const SpeckleItem* __restrict__ items, const int32_t* __restrict__ first, int nItems,
                                                                     float thr, SpeckleResult* result) {
	__shared__ float sD[kTilePixels];
	__shared__ int sL[kTilePixels];
	__shared__ int sC[kTilePixels];
	SpeckleItem it;
	const Tile t = speckle_tile(items, first, nItems, it);
	const int lane = (int)threadIdx.x & 63, row0 = (int)threadIdx.x >> 6;
	const int gx = t.x0 + lane;
	float d[kRounds];
	bool inside[kRounds];
#pragma unroll
	for (int k = 0; k < kRounds; ++k) {
		const int ly = row0 + k * kWaves, li = ly * kSpeckleTileW + lane, gy = t.y0 + ly;
		inside[k] = gx < it.w && gy < it.h;
		d[k] = inside[k] ? it.depth[(size_t)gy * it.w + gx] : 0.f;
		sD[li] = d[k];
		sL[li] = speckle_valid(d[k]) ? li : -1;
		sC[li] = 0;
	}
	__syncthreads();
	bool ok = true;
#pragma unroll
	for (int k = 0; k < kRounds; ++k) {
		const int ly = row0 + k * kWaves, li = ly * kSpeckleTileW + lane;
		if (!speckle_valid(d[k])) continue;
		if (lane + 1 < kSpeckleTileW) {
			const float dq = sD[li + 1];
			if (speckle_valid(dq) && speckle_joined(d[k], dq, thr)) ok &= lds_union(sL, li, li + 1);
		}
		if (ly + 1 < kSpeckleTileH) {
			const float dq = sD[li + kSpeckleTileW];
			if (speckle_valid(dq) && speckle_joined(d[k], dq, thr)) ok &= lds_union(sL, li, li + kSpeckleTileW);
		}
	}
	__syncthreads();
	int root[kRounds];
#pragma unroll
	for (int k = 0; k < kRounds; ++k) {
		const int li = (row0 + k * kWaves) * kSpeckleTileW + lane;
		root[k] = speckle_valid(d[k]) ? lds_find(sL, li) : -1;
		if (speckle_valid(d[k]) && root[k] < 0) ok = false;
	}
	// the pixel counts of the tile-local components: the lanes of a row that share a root add once
#pragma unroll
	for (int k = 0; k < kRounds; ++k) {
		unsigned long long todo = __ballot(root[k] >= 0);
		while (todo) { // wave-uniform; at most 64 rounds
			const int leader = __ffsll((long long)todo) - 1;
			const int lr = __shfl(root[k], leader, 64);
			const unsigned long long same = __ballot(root[k] == lr);
			if (lane == leader) atomicAdd(sC + lr, __popcll(same));
			todo &= ~same;
		}
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < kRounds; ++k) {
		if (!inside[k]) continue;
		const int ly = row0 + k * kWaves, li = ly * kSpeckleTileW + lane;
		const size_t g = (size_t)(t.y0 + ly) * it.w + gx;
		const int r = root[k];
		it.labels[g] = r < 0 ? -1 : (int32_t)((t.y0 + (r >> 6)) * it.w + t.x0 + (r & 63)); // < w * h < 2^31
		it.sizes[g] = r == li ? sC[li] : 0;
	}
	if (!ok) raise_error(result);
}

// ---- 2: the borders -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBorderBlock) void speckle_border_kernel(const SpeckleItem* __restrict__ items, const int32_t* __restrict__ first, int nItems,
                                                                      float thr, SpeckleResult* result) {
	SpeckleItem it;
	const Tile t = speckle_tile(items, first, nItems, it);
	const int k = (int)threadIdx.x;
	int x, y, back; // back: the distance to the neighbour in the other tile
	if (k < kSpeckleTileW) { x = t.x0 + k; y = t.y0; back = it.w; if (t.y0 == 0) return; }
	else if (k < kSpeckleTileW + kSpeckleTileH) { x = t.x0; y = t.y0 + (k - kSpeckleTileW); back = 1; if (t.x0 == 0) return; }
	else return;
	if (x >= it.w || y >= it.h) return;
	const int32_t n = it.w * it.h;
	const int32_t p = y * it.w + x, q = p - back; // q >= 0: y > 0 (back = w) or x > 0 (back = 1)
	const float dp = it.depth[p], dq = it.depth[q];
	if (!speckle_valid(dp) || !speckle_valid(dq) || !speckle_joined(dp, dq, thr)) return;
	if (!global_union(it.labels, p, q, n)) raise_error(result);
}

// ---- 3: the sizes -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpeckleBlock) void speckle_size_kernel(const SpeckleItem* __restrict__ items, const int32_t* __restrict__ first, int nItems,
                                                                     SpeckleResult* result) {
	SpeckleItem it;
	const Tile t = speckle_tile(items, first, nItems, it);
	const int lane = (int)threadIdx.x & 63, row0 = (int)threadIdx.x >> 6;
	const int gx = t.x0 + lane;
	if (gx >= it.w) return;
	const int32_t n = it.w * it.h;
	for (int k = 0; k < kRounds; ++k) {
		const int gy = t.y0 + row0 + k * kWaves;
		if (gy >= it.h) break;
		const int32_t g = gy * it.w + gx;
		// a count is only ever added to at a root, and a root adds nothing of its own below: what a tile-local root reads here is its own
		const int32_t mine = it.sizes[g];
		if (mine <= 0) continue; // not a tile-local root
		const int32_t r = global_find(it.labels, g, n);
		if (r < 0) { raise_error(result); continue; }
		if (r == g) continue;
		__hip_atomic_store(it.labels + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // another thread's find may pass through g: either parent serves
		atomicAdd(it.sizes + r, mine);
	}
}

// ---- 4: apply -----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_add(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
	for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
	return v;
}

__global__ __launch_bounds__(kSpeckleBlock) void speckle_apply_kernel(const SpeckleItem* __restrict__ items, const int32_t* __restrict__ first, int nItems,
                                                                      uint32_t speckleSize, SpecklePartial* partials) {
	SpeckleItem it;
	const Tile t = speckle_tile(items, first, nItems, it);
	const int lane = (int)threadIdx.x & 63, row0 = (int)threadIdx.x >> 6;
	const int gx = t.x0 + lane;
	uint32_t valid = 0, removed = 0, segments = 0, small = 0, largest = 0;
	for (int k = 0; k < kRounds; ++k) {
		const int gy = t.y0 + row0 + k * kWaves;
		if (gx >= it.w || gy >= it.h) break;
		const int32_t g = gy * it.w + gx;
		const int32_t l = it.labels[g]; // the tile-local root (or the root, where launch 3 wrote it), -1: not valid
		if (l < 0) {
			if (it.outLabels) it.outLabels[g] = -1;
			continue;
		}
		const int32_t r = it.labels[l];
		const uint32_t size = (uint32_t)it.sizes[r];
		const bool gone = size < speckleSize;
		valid += 1; removed += gone ? 1u : 0u;
		if (r == g) { segments += 1; small += gone ? 1u : 0u; largest = size > largest ? size : largest; }
		if (it.outLabels) it.outLabels[g] = r;
		if (!gone) continue;
		it.depth[g] = 0.f;
		if (it.normal) { float* o = it.normal + 3 * (size_t)g; o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; }
		if (it.conf) it.conf[g] = 0.f;
	}
	__shared__ uint32_t sV[kWaves], sR[kWaves], sS[kWaves], sM[kWaves], sL[kWaves];
	valid = wave_add(valid); removed = wave_add(removed); segments = wave_add(segments); small = wave_add(small); largest = wave_max(largest);
	const int wave = (int)threadIdx.x >> 6;
	if (lane == 0) { sV[wave] = valid; sR[wave] = removed; sS[wave] = segments; sM[wave] = small; sL[wave] = largest; }
	__syncthreads();
	if (threadIdx.x != 0) return;
	for (int w = 1; w < kWaves; ++w) { valid += sV[w]; removed += sR[w]; segments += sS[w]; small += sM[w]; largest = sL[w] > largest ? sL[w] : largest; }
	SpecklePartial p;
	p.valid = valid; p.removed = removed; p.segments = segments; p.small = small; p.largest = largest; p.pad = 0;
	partials[blockIdx.x] = p;
}

// ---- 5: the counters ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpeckleBlock) void speckle_sum_kernel(const SpecklePartial* __restrict__ partials, int nTiles, SpeckleResult* result) {
	unsigned long long valid = 0, removed = 0, segments = 0, small = 0;
	uint32_t largest = 0;
	for (int b = (int)threadIdx.x; b < nTiles; b += kSpeckleBlock) {
		const SpecklePartial p = partials[b];
		valid += p.valid; removed += p.removed; segments += p.segments; small += p.small; largest = p.largest > largest ? p.largest : largest;
	}
	for (int o = 32; o > 0; o >>= 1) {
		valid += __shfl_xor(valid, o, 64); removed += __shfl_xor(removed, o, 64); segments += __shfl_xor(segments, o, 64); small += __shfl_xor(small, o, 64);
	}
	largest = wave_max(largest);
	__shared__ unsigned long long sV[kWaves], sR[kWaves], sS[kWaves], sM[kWaves];
	__shared__ uint32_t sL[kWaves];
	const int wave = (int)threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { sV[wave] = valid; sR[wave] = removed; sS[wave] = segments; sM[wave] = small; sL[wave] = largest; }
	__syncthreads();
	if (threadIdx.x != 0) return;
	for (int w = 1; w < kWaves; ++w) { valid += sV[w]; removed += sR[w]; segments += sS[w]; small += sM[w]; largest = sL[w] > largest ? sL[w] : largest; }
	result->valid = valid; result->removed = removed; result->segments = segments; result->small = small; result->largest = largest; // error: left as raised
}

} // namespace

void launch_speckle(const SpeckleItem* items, const int32_t* first, int nItems, int nTiles, float thr, uint32_t speckleSize, SpecklePartial* partials,
                    SpeckleResult* result, hipStream_t s) {
	const dim3 grid((unsigned)nTiles);
	hipLaunchKernelGGL(speckle_tile_kernel, grid, dim3(kSpeckleBlock), 0, s, items, first, nItems, thr, result);
	hipLaunchKernelGGL(speckle_border_kernel, grid, dim3(kBorderBlock), 0, s, items, first, nItems, thr, result);
	hipLaunchKernelGGL(speckle_size_kernel, grid, dim3(kSpeckleBlock), 0, s, items, first, nItems, result);
	hipLaunchKernelGGL(speckle_apply_kernel, grid, dim3(kSpeckleBlock), 0, s, items, first, nItems, speckleSize, partials);
	hipLaunchKernelGGL(speckle_sum_kernel, dim3(1), dim3(kSpeckleBlock), 0, s, partials, nTiles, result);
}

} // namespace hcmvs

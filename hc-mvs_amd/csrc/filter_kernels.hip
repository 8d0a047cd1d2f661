/*
 * hc-mvs_amd/csrc/filter_kernels.hip -- gfx950 kernels of the scene-level depth-map filter stage (hcmvs_filter_sequence).
 *
 * What the reference computes (files of the reference's libs/MVS/):
 *   Scene::DenseReconstructionFilter  SceneDensify.cpp:4100-4185 (queued at :3721-3756)  every depth map is filtered against up to
 *                                     8 of its neighbours' maps (FilterDepthMap, :3006-3259); the filtered maps replace the
 *                                     estimated ones only after ALL images were filtered (:4134-4135)
 *
 * How it is mapped to the GPU: a batch of reference images at a time.  One fill of the batch's z-buffer planes, ONE splat launch
 * over all (reference, neighbour) pairs of the batch -- a workgroup finds its pair in a prefix table of workgroup counts and
 * grid-strides inside it --, ONE vote launch over all images of the batch, which writes the new depth and confidence into
 * staging slabs (the registered maps stay as they were when the call began: every image is filtered from that snapshot) and counts
 * into per-image slots; after the last batch one commit launch copies the slabs over the registered maps.  The per-pixel
 * arithmetic is filter_device.h's, shared with the per-image kernels of hcmvs_filter.
 *
 * The splat is bound by the rate of 64-bit atomics at the memory side (4 per valid neighbour pixel), not by HBM bandwidth: a wave
 * issues, per footprint corner, one atomic instruction whose 64 lanes hit mostly consecutive 8-byte keys of one or two rows of the
 * reference view (neighbouring source pixels project next to each other) -- the contiguous shape DESIGN.md section 3.4 measures.
 */
#include "filter_device.h"

namespace hcmvs {

constexpr int kFilterBlock = 256;

// the pair / image a workgroup belongs to: the last entry of the ascending table first[0 .. n] that is <= block
__device__ __forceinline__ int filter_find(const int* first, int n, int block) {
	int lo = 0, hi = n;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (first[mid] <= block) lo = mid; else hi = mid;
	}
	return lo;
}

__global__ __launch_bounds__(kFilterBlock) void filter_splat_batch_kernel(const FilterRef* refs, const FilterPair* pairs, const int* pairFirst, int nPairs) {
	const int p = filter_find(pairFirst, nPairs, (int)blockIdx.x);
	const FilterRef& r = refs[pairs[p].ref];
	const DevMap& nb = r.nbs[pairs[p].nb];
	unsigned long long* key = r.keys + (size_t)r.map.w * r.map.h * pairs[p].nb;
	const int n = nb.w * nb.h, stride = (pairFirst[p + 1] - pairFirst[p]) * kFilterBlock;
	for (int s = ((int)blockIdx.x - pairFirst[p]) * kFilterBlock + (int)threadIdx.x; s < n; s += stride) filter_splat_pixel(r.map, nb, key, s);
}

__global__ __launch_bounds__(kFilterBlock) void filter_vote_batch_kernel(const FilterRef* refs, const int* refFirst, int nRefs, int adjust, int nMinViews,
                                                                         int nMinViewsAdjust, float fDepthDiffThreshold) {
	const int q = filter_find(refFirst, nRefs, (int)blockIdx.x);
	const FilterRef& r = refs[q];
	const int area = r.map.w * r.map.h, stride = (refFirst[q + 1] - refFirst[q]) * kFilterBlock;
	unsigned nProc = 0, nDisc = 0;
	for (int idx = ((int)blockIdx.x - refFirst[q]) * kFilterBlock + (int)threadIdx.x; idx < area; idx += stride) {
		const float depth = r.map.depth[idx];
		float d = 0.f, c = 0.f;
		if (depth != 0.f) {
			++nProc;
			if (!filter_vote_pixel(r.map, r.nbs, r.nNbs, r.keys, idx, depth, adjust, nMinViews, nMinViewsAdjust, fDepthDiffThreshold, d, c)) ++nDisc;
		}
		r.newDepth[idx] = d; r.newConf[idx] = c;
	}
	// the workgroup's counts: summed per wave, then through LDS -- two atomics per workgroup on the image's slot
	__shared__ unsigned sProc[kFilterBlock / 64], sDisc[kFilterBlock / 64];
	for (int o = 32; o > 0; o >>= 1) { nProc += __shfl_down(nProc, o, 64); nDisc += __shfl_down(nDisc, o, 64); }
	if ((threadIdx.x & 63) == 0) { sProc[threadIdx.x >> 6] = nProc; sDisc[threadIdx.x >> 6] = nDisc; }
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long a = 0, b = 0;
		for (int w = 0; w < kFilterBlock / 64; ++w) { a += sProc[w]; b += sDisc[w]; }
		if (a) atomicAdd(&r.counters[0], a);
		if (b) atomicAdd(&r.counters[1], b);
	}
}

// after the last batch: the staged depth and confidence of every filtered image replace its registered maps (blockIdx.y = image)
__global__ void filter_commit_kernel(const FilterRef* refs, int nRefs) {
	for (int q = blockIdx.y; q < nRefs; q += gridDim.y) {
		const FilterRef& r = refs[q];
		float* depth = r.map.depth;
		float* conf = const_cast<float*>(r.map.conf);
		const size_t n = (size_t)r.map.w * r.map.h;
		for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { depth[i] = r.newDepth[i]; conf[i] = r.newConf[i]; }
	}
}

int filter_blocks(size_t pixels) { // workgroups of one pair / one image: 4 pixels per thread, as the per-image kernels at 1080p
	const size_t b = (pixels + (size_t)kFilterBlock * 4 - 1) / ((size_t)kFilterBlock * 4);
	return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
void launch_filter_splat_batch(const FilterRef* refs, const FilterPair* pairs, const int* pairFirst, int nPairs, int nBlocks, hipStream_t s) {
	hipLaunchKernelGGL(filter_splat_batch_kernel, dim3(nBlocks), dim3(kFilterBlock), 0, s, refs, pairs, pairFirst, nPairs);
}
void launch_filter_vote_batch(const FilterRef* refs, const int* refFirst, int nRefs, int nBlocks, int adjust, int nMinViews, int nMinViewsAdjust, float thr,
                              hipStream_t s) {
	hipLaunchKernelGGL(filter_vote_batch_kernel, dim3(nBlocks), dim3(kFilterBlock), 0, s, refs, refFirst, nRefs, adjust, nMinViews, nMinViewsAdjust, thr);
}
void launch_filter_commit(const FilterRef* refs, int nRefs, hipStream_t s) {
	hipLaunchKernelGGL(filter_commit_kernel, dim3(256, nRefs < 1024 ? nRefs : 1024), dim3(256), 0, s, refs, nRefs);
}

} // namespace hcmvs

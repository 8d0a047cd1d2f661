/*
 * hc-mvs_amd/csrc/filter_device.h -- the per-pixel arithmetic of FilterDepthMap (SceneDensify.cpp:3006-3259), shared by the per-image
 * kernels of hcmvs_filter (fuse_kernels.hip) and the batched kernels of hcmvs_filter_sequence (filter_kernels.hip): one source pixel
 * of the splat, one reference pixel of the vote.  The tests pin both against the sequential algorithm, bit for bit.
 */
#ifndef HCMVS_FILTER_DEVICE_H
#define HCMVS_FILTER_DEVICE_H

#include "fuse_device.h"

namespace hcmvs {

// source pixel s of neighbour map nb into the z-buffer plane `key` of the reference view (SceneDensify.cpp:3027-3089): 4-pixel
// footprint; the 64-bit atomicMin on (depth bits, ~sequence number) reproduces "nearest wins, the later writer wins ties"
__device__ __forceinline__ void filter_splat_pixel(const DevMap& ref, const DevMap& nb, unsigned long long* key, int s) {
	const float depth = nb.depth[s];
	if (depth == 0.f) return;
	const int j = s % nb.w, i = s / nb.w;
	double X[3], c[3];
	i2w(nb, (double)j, (double)i, (double)depth, X);
	w2c(ref, X, c);
	if (c[2] <= 0) return;
	const double ix = ref.K[2] + ref.K[0] * (c[0] / c[2]), iy = ref.K[5] + ref.K[4] * (c[1] / c[2]);
	const int fx = (int)floor(ix), fy = (int)floor(iy), cx = (int)ceil(ix), cy = (int)ceil(iy);
	const int xs[4] = {fx, fx, cx, cx}, ys[4] = {fy, cy, fy, cy};
	const float z = (float)c[2];
#pragma unroll
	for (int p = 0; p < 4; ++p) {
		if (xs[p] < 0 || ys[p] < 0 || xs[p] >= ref.w || ys[p] >= ref.h) continue;
		// nearest depth wins; among equal depths the later (source raster, footprint) writer wins
		const unsigned long long k = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)(0xFFFFFFFFu - ((unsigned)s * 4u + (unsigned)p));
		atomicMin(&key[(size_t)ys[p] * ref.w + xs[p]], k);
	}
}

__device__ __forceinline__ float key_depth(unsigned long long k) { return k == ~0ull ? 0.f : __uint_as_float((unsigned)(k >> 32)); }
__device__ __forceinline__ float key_conf(unsigned long long k, const float* conf) {
	return k == ~0ull ? 0.f : conf[(0xFFFFFFFFu - (unsigned)k) >> 2];
}

// reference pixel idx (depth != 0) against the N z-buffer planes: the new depth and confidence; returns whether the estimate is kept
__device__ __forceinline__ bool filter_vote_pixel(const DevMap& ref, const DevMap* nbs, int N, const unsigned long long* keys, int idx, float depth, int adjust,
                                                  int nMinViews, int nMinViewsAdjust, float fDepthDiffThreshold, float& outDepth, float& outConf) {
	const int W = ref.w, H = ref.h;
	const size_t area = (size_t)W * H;
	const int j = idx % W, i = idx / W;
	outDepth = 0.f; outConf = 0.f;
	if (adjust) { // SceneDensify.cpp:3097-3170
		float posConf = ref.conf[idx], negConf = 0.f;
		float avgDepth = depth * posConf;
		unsigned nPos = 0, nNeg = 0;
		int n = N;
		do {
			--n;
			const unsigned long long k = keys[area * n + idx];
			const float d = key_depth(k);
			if (d == 0.f) {
				if (nPos + nNeg + (unsigned)n < (unsigned)nMinViews) return false;
				continue;
			}
			const float cproj = key_conf(k, nbs[n].conf);
			if (is_depth_similar(depth, d, 0.12f)) {
				avgDepth += d * cproj;
				posConf += cproj;
				++nPos;
			} else {
				if (depth > d) {
					negConf += cproj;
				} else {
					const DevMap& nb = nbs[n];
					double X[3], c[3];
					i2w(ref, (double)j, (double)i, (double)depth, X);
					w2c(nb, X, c);
					const int x = (int)floor(nb.K[2] + nb.K[0] * (c[0] / c[2]) + .5);
					const int y = (int)floor(nb.K[5] + nb.K[4] * (c[1] / c[2]) + .5);
					if (x >= 0 && y >= 0 && x < nb.w && y < nb.h) {
						const float cc = nb.conf[(size_t)y * nb.w + x];
						negConf += (cc > 0.f ? cc : cproj);
					} else
						negConf += cproj;
				}
				++nNeg;
			}
		} while (n);
		if (nPos >= (unsigned)nMinViewsAdjust && posConf > negConf) {
			avgDepth /= posConf;
			if (ref.dMin <= avgDepth && avgDepth < ref.dMax) { outDepth = avgDepth; outConf = posConf - negConf; return true; }
		}
		return false;
	}
	// SceneDensify.cpp:3171-3249
	const float thDepthDiff = fDepthDiffThreshold * 1.2f;
	const float thStrict = fDepthDiffThreshold * 0.8f;
	const unsigned nMinViewsDelta = (unsigned)nMinViews * 2u;
	unsigned good = 0, views = 0;
	for (int n = N; n-- > 0;) {
		const float d = key_depth(keys[area * n + idx]);
		if (d > 0.f) { ++views; if (is_depth_similar(depth, d, thStrict)) ++good; }
	}
	if (good < (unsigned)nMinViews || good < views * 75u / 100u) return false;
	good = views = 0;
	const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const int xx = j + dx[q], yy = i + dy[q];
		if (xx < 0 || yy < 0 || xx >= W || yy >= H) continue;
		for (int n = N; n-- > 0;) {
			const float d = key_depth(keys[area * n + (size_t)yy * W + xx]);
			if (d > 0.f) { ++views; if (is_depth_similar(depth, d, thDepthDiff)) ++good; }
		}
	}
	if (good < nMinViewsDelta || good < views * 65u / 100u) return false;
	outDepth = depth; outConf = ref.conf[idx];
	return true;
}

} // namespace hcmvs
#endif

/*
 * hc-mvs_amd/csrc/vis_kernels.hip -- the visibility filter of a finished cloud on the device.
 *
 * Scene::PointCloudFilter (frame_main/libs/MVS/SceneDensify.cpp:4188-4320, DensifyPointCloud --filter-point-cloud < 0) gives every
 * image j a cone: apex Cf = float(C_j), half-angle angle = float(ComputeFOV(0) / width) (Image.cpp:215-226), i.e. about one pixel.
 * For every point X and every view j of X the cone is pointed at X (dir = (X - Cf) / |X - Cf|, height limit 1.02 |X - Cf|) and every
 * point P of the cloud inside it (TConeIntersect::Classify, Ray.inl:986-1002) that is not depth-similar to X (1 %) votes: P behind X
 * gains |views(P)|, P in front of X loses |views(X)|.  The reference finds the P with an octree on the CPU; the set it visits is every
 * point that passes Classify, so the sums are restated here over "all points", with an exact candidate search:
 *
 * View by view, every point is projected from Cf into the gnomonic plane of camera j (u = x/z, v = y/z of R (P - Cf), in double from
 * the float P - Cf that Classify itself uses) and counting-sorted into pixel-sized cells (edge 1 / max(fx, fy)) over the image grown by
 * kMargin cells.  A point P that Classify accepts makes an angle of at most phi with dir, where sin^2(phi) = 1 - cosSq + 32 ulp(1)
 * covers the float rounding of the test (t, |E|^2, |dir| != 1: about 20 ulp); in the plane a direction within phi of X's lies within
 * phi / cos^2(theta_X + phi) of X's projection (the gnomonic stretch is at most sec^2 of the off-axis angle), so the cells within
 * ceil(1.01 r / cell) + 1 of X's cell hold every candidate, one contiguous range per cell row.  The exact test then runs on each of them.
 * A pair whose square of cells leaves the grid, whose X is not in front of the camera or whose theta_X + phi exceeds 1.45 rad takes the
 * exact path over all points (rare on a fused cloud, where X projects into each of its views).  The votes are integer atomics (no-return
 * global_atomic_add), order-free: the sums are the sequential ones exactly.  Device memory: O(points + pairs + one view's cells).
 */
#include "vis_kernels.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

namespace hcmvs {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu; // key of a point outside the view's grid
constexpr int kMargin = 32;             // cells around the image
constexpr double kMaxCells = 268435456.0;
static const dim3 kBlock(256);

struct VisView {
	float C[3];
	float cosSq;
	double R[9];
	double u0, v0, cell; // cell (cu, cv) covers u0 + [cu, cu + 1) * cell, v0 + [cv, cv + 1) * cell of the gnomonic plane
	int gx, gy;          // 0: no grid, every pair of the view takes the exact path
	double phi;          // half-angle the candidate search covers (radians)
};

struct Ray {
	float C[3], d[3], dist, maxH, cosSq;
	int w;
};

__device__ __forceinline__ void make_ray(Ray& r, const float* X, const VisView& v, int w, float* D) {
	D[0] = X[0] - v.C[0]; D[1] = X[1] - v.C[1]; D[2] = X[2] - v.C[2];
	r.dist = sqrtf((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
	r.d[0] = D[0] / r.dist; r.d[1] = D[1] / r.dist; r.d[2] = D[2] / r.dist;
	r.maxH = r.dist * 1.02f; // MaxDepthDifference(distance, 1.02f), Util.inl:650
	r.C[0] = v.C[0]; r.C[1] = v.C[1]; r.C[2] = v.C[2];
	r.cosSq = v.cosSq;
	r.w = w;
}
// TConeIntersect::Classify == VISIBLE and !IsDepthSimilar(dist, t, 0.01f): +1 when P lies behind X, -1 in front, 0 no vote
__device__ __forceinline__ int classify(const Ray& r, float px, float py, float pz) {
	const float ex = px - r.C[0], ey = py - r.C[1], ez = pz - r.C[2];
	const float t = (r.d[0] * ex + r.d[1] * ey) + r.d[2] * ez;
	if (fabsf(t) < 1e-4f || t < 0.f || t > r.maxH) return 0;
	const float e2 = (ex * ex + ey * ey) + ez * ez;
	if (!(t * t > r.cosSq * e2)) return 0;
	if (fabsf(r.dist - t) / r.dist < 0.01f) return 0;
	return t > r.dist ? 1 : -1;
}
__device__ __forceinline__ void add_wave(unsigned long long v, unsigned long long* dst) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

__global__ __launch_bounds__(256) void bin_kernel(unsigned long long n, const float* xyz, VisView v, uint32_t* keys, uint32_t* counts) {
	for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
		const float ex = xyz[3 * i] - v.C[0], ey = xyz[3 * i + 1] - v.C[1], ez = xyz[3 * i + 2] - v.C[2];
		const double x = v.R[0] * ex + v.R[1] * ey + v.R[2] * ez, y = v.R[3] * ex + v.R[4] * ey + v.R[5] * ez, z = v.R[6] * ex + v.R[7] * ey + v.R[8] * ez;
		uint32_t key = kNone;
		if (z > 0) {
			const double cu = floor((x / z - v.u0) / v.cell), cv = floor((y / z - v.v0) / v.cell);
			if (cu >= 0 && cu < v.gx && cv >= 0 && cv < v.gy) {
				key = (uint32_t)cv * (uint32_t)v.gx + (uint32_t)cu;
				atomicAdd(&counts[key], 1u);
			}
		}
		keys[i] = key;
	}
}
__global__ __launch_bounds__(256) void scatter_kernel(unsigned long long n, const float* xyz, const uint32_t* keys, uint32_t* cursor, float4* binned) {
	for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t key = keys[i];
		if (key == kNone) continue;
		const uint32_t pos = atomicAdd(&cursor[key], 1u);
		binned[pos] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __uint_as_float((uint32_t)i));
	}
}
// one thread per pair (X, this view); counters: [0] candidates, [1] hits, [2] fallback pairs, [3] this view's fallback count (u32)
__global__ __launch_bounds__(256) void query_kernel(unsigned long long nPairs, const uint32_t* pairs, const float* xyz, const uint32_t* nViews, VisView v,
                                                    const uint32_t* offsets, const float4* binned, int* vis, uint32_t* fbList, unsigned long long* counters) {
	unsigned long long cand = 0, hits = 0;
	uint32_t* fbCount = (uint32_t*)(counters + 3);
	for (unsigned long long k = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; k < nPairs; k += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t i = pairs[k];
		Ray r;
		float D[3];
		make_ray(r, xyz + 3 * (size_t)i, v, (int)nViews[i], D);
		const double x = v.R[0] * D[0] + v.R[1] * D[1] + v.R[2] * D[2], y = v.R[3] * D[0] + v.R[4] * D[1] + v.R[5] * D[2],
		             z = v.R[6] * D[0] + v.R[7] * D[1] + v.R[8] * D[2];
		bool exact = !(z > 0) || v.gx == 0;
		long long cu0 = 0, cu1 = -1, cv0 = 0, cv1 = -1;
		if (!exact) {
			const double th = acos(fmin(z / sqrt(x * x + y * y + z * z), 1.0)) + v.phi; // off-axis angle the cone reaches
			if (!(th < 1.45)) exact = true;
			else {
				const double c = cos(th), rc = ceil(1.01 * v.phi / (c * c) / v.cell) + 1.0;
				const double cu = floor((x / z - v.u0) / v.cell), cv = floor((y / z - v.v0) / v.cell);
				if (!(cu - rc >= 0 && cu + rc < v.gx && cv - rc >= 0 && cv + rc < v.gy)) exact = true;
				else { cu0 = (long long)(cu - rc); cu1 = (long long)(cu + rc); cv0 = (long long)(cv - rc); cv1 = (long long)(cv + rc); }
			}
		}
		if (exact) { fbList[atomicAdd(fbCount, 1u)] = i; continue; }
		for (long long row = cv0; row <= cv1; ++row) {
			const uint32_t s0 = offsets[row * v.gx + cu0], s1 = offsets[row * v.gx + cu1 + 1];
			cand += s1 - s0;
			for (uint32_t s = s0; s < s1; ++s) {
				const float4 p = binned[s];
				const int c = classify(r, p.x, p.y, p.z);
				if (c) {
					const uint32_t idx = __float_as_uint(p.w);
					atomicAdd(&vis[idx], c > 0 ? (int)nViews[idx] : -r.w);
					++hits;
				}
			}
		}
	}
	add_wave(cand, counters);
	add_wave(hits, counters + 1);
}
// the exact path: every pair the query left goes over all points; blockIdx.y strides over the pairs, x over the points
__global__ __launch_bounds__(256) void fallback_kernel(const uint32_t* fbList, unsigned long long n, const float* xyz, const uint32_t* nViews, VisView v,
                                                       int* vis, unsigned long long* counters) {
	const uint32_t nf = *(const uint32_t*)(counters + 3);
	unsigned long long hits = 0;
	for (uint32_t f = blockIdx.y; f < nf; f += gridDim.y) {
		const uint32_t i = fbList[f];
		Ray r;
		float D[3];
		make_ray(r, xyz + 3 * (size_t)i, v, (int)nViews[i], D);
		for (unsigned long long p = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; p < n; p += (unsigned long long)gridDim.x * blockDim.x) {
			const int c = classify(r, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]);
			if (c) { atomicAdd(&vis[p], c > 0 ? (int)nViews[p] : -r.w); ++hits; }
		}
	}
	add_wave(hits, counters + 1);
	if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && nf) { atomicAdd(&counters[0], (unsigned long long)nf * n); atomicAdd(&counters[2], (unsigned long long)nf); }
}
} // namespace

int point_cloud_visibility_device(unsigned long long n, const float* hXyz, const uint32_t* hNViews, const uint32_t* hViewIds, uint32_t nImages,
                                  const int32_t* wh, const double* K, const double* R, const double* C, int32_t* hVis, VisCounters& st,
                                  DevBuf& scratch, hipStream_t s, std::string& err) {
	st = VisCounters();
	if (n == 0) return 0;
	if (n >= 0xFFFFFFFFull) { err = "point_cloud_filter: 2^32 - 1 points or more"; return 1; }
	// the cones and the gnomonic grids
	std::vector<VisView> views(nImages);
	std::vector<char> calibrated(nImages, 0);
	for (uint32_t j = 0; j < nImages; ++j) {
		const int w = wh[2 * j], h = wh[2 * j + 1];
		if (w <= 0 || h <= 0) continue; // uncalibrated
		calibrated[j] = 1;
		VisView& v = views[j];
		const double* k = K + 9 * (size_t)j;
		const float angle = (float)(2.0 * std::atan((double)w / (k[0] * 2.0)) / (double)w); // Image::ComputeFOV(0) / width
		const float c = (float)std::cos((double)angle);
		v.cosSq = c * c;
		for (int q = 0; q < 3; ++q) v.C[q] = (float)C[3 * (size_t)j + q];
		for (int q = 0; q < 9; ++q) v.R[q] = R[9 * (size_t)j + q];
		const double sin2 = std::min(1.0, (1.0 - (double)v.cosSq) + 32.0 / 16777216.0);
		v.phi = std::asin(std::sqrt(sin2)) + 1e-6;
		const double fx = k[0], fy = k[4], cx = k[2], cy = k[5];
		v.gx = v.gy = 0;
		if (std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy) && fx > 0 && fy > 0) {
			v.cell = 1.0 / std::max(fx, fy);
			v.u0 = (-0.5 - cx) / fx - kMargin * v.cell;
			v.v0 = (-0.5 - cy) / fy - kMargin * v.cell;
			const double gx = std::ceil((double)w / fx / v.cell) + 2 * kMargin, gy = std::ceil((double)h / fy / v.cell) + 2 * kMargin;
			if (gx * gy <= kMaxCells) { v.gx = (int)gx; v.gy = (int)gy; }
		}
	}
	// the pairs, grouped by view (CSR over the images)
	std::vector<size_t> start((size_t)nImages + 1, 0);
	{
		size_t off = 0;
		for (unsigned long long i = 0; i < n; ++i)
			for (uint32_t e = 0; e < hNViews[i]; ++e, ++off) {
				const uint32_t j = hViewIds[off];
				if (j < nImages && calibrated[j]) ++start[(size_t)j + 1];
				else ++st.skipped;
			}
	}
	for (uint32_t j = 0; j < nImages; ++j) start[(size_t)j + 1] += start[j];
	st.pairs = start[nImages];
	std::vector<uint32_t> pairs(std::max<size_t>(st.pairs, 1));
	{
		std::vector<size_t> fill(start.begin(), start.end() - 1);
		size_t off = 0;
		for (unsigned long long i = 0; i < n; ++i)
			for (uint32_t e = 0; e < hNViews[i]; ++e, ++off) {
				const uint32_t j = hViewIds[off];
				if (j < nImages && calibrated[j]) pairs[fill[j]++] = (uint32_t)i;
			}
	}
	size_t maxPairs = 1, maxCells = 1;
	for (uint32_t j = 0; j < nImages; ++j) {
		const size_t np = start[(size_t)j + 1] - start[j];
		maxPairs = std::max(maxPairs, np);
		if (np) maxCells = std::max(maxCells, (size_t)views[j].gx * (size_t)views[j].gy);
	}
	size_t scanBytes = 0;
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(maxCells + 1));
	Carve carve;
	const size_t oXyz = carve(n * 12), oNv = carve(n * 4), oVis = carve(n * 4), oKeys = carve(n * 4), oBinned = carve(n * 16),
	             oPairs = carve(pairs.size() * 4), oFb = carve(maxPairs * 4), oOffsets = carve((maxCells + 1) * 4), oCounts = carve((maxCells + 1) * 4),
	             oCounters = carve(64), oScan = carve(scanBytes);
	if (scratch.reserve(carve.size, s) != hipSuccess) { err = "point_cloud_filter: out of device memory"; return 2; }
	char* b = scratch.get();
	st.deviceBytes = carve.size;
	hipEvent_t ev[2] = {nullptr, nullptr};
	auto fail = [&](const char* what) {
		err = what;
		(void)hipStreamSynchronize(s); // (the caller frees scratch on return)
		for (auto& e : ev) if (e) (void)hipEventDestroy(e);
		return 2;
	};
	if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) return fail("point_cloud_filter: event creation failed");
	float* dXyz = (float*)(b + oXyz);
	uint32_t *dNv = (uint32_t*)(b + oNv), *keys = (uint32_t*)(b + oKeys), *dPairs = (uint32_t*)(b + oPairs), *fb = (uint32_t*)(b + oFb),
	         *offsets = (uint32_t*)(b + oOffsets), *counts = (uint32_t*)(b + oCounts);
	int* dVis = (int*)(b + oVis);
	float4* binned = (float4*)(b + oBinned);
	unsigned long long* counters = (unsigned long long*)(b + oCounters);
	if (hipMemcpyAsync(dXyz, hXyz, n * 12, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(dNv, hNViews, n * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
	    hipMemcpyAsync(dPairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess || hipMemsetAsync(dVis, 0, n * 4, s) != hipSuccess ||
	    hipMemsetAsync(counters, 0, 64, s) != hipSuccess)
		return fail("point_cloud_filter: upload failed");
	(void)hipEventRecord(ev[0], s);
	const unsigned pointBlocks = (unsigned)std::min<unsigned long long>((n + 255) / 256, 4096);
	for (uint32_t j = 0; j < nImages; ++j) {
		const unsigned long long np = start[(size_t)j + 1] - start[j];
		if (!np) continue;
		const VisView& v = views[j];
		if (v.gx) { // counting sort of the points by their cell in this view
			const size_t cells = (size_t)v.gx * v.gy;
			if (hipMemsetAsync(counts, 0, (cells + 1) * 4, s) != hipSuccess) return fail("point_cloud_filter: memset failed");
			hipLaunchKernelGGL(bin_kernel, dim3(pointBlocks), kBlock, 0, s, n, dXyz, v, keys, counts);
			if (hipcub::DeviceScan::ExclusiveSum(b + oScan, scanBytes, counts, offsets, (int)(cells + 1), s) != hipSuccess) return fail("point_cloud_filter: scan failed");
			if (hipMemcpyAsync(counts, offsets, cells * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail("point_cloud_filter: copy failed");
			hipLaunchKernelGGL(scatter_kernel, dim3(pointBlocks), kBlock, 0, s, n, dXyz, keys, counts, binned);
		}
		if (hipMemsetAsync(counters + 3, 0, 8, s) != hipSuccess) return fail("point_cloud_filter: memset failed");
		hipLaunchKernelGGL(query_kernel, dim3((unsigned)std::min<unsigned long long>((np + 255) / 256, 8192)), kBlock, 0, s, np, dPairs + start[j], dXyz, dNv, v,
		                   offsets, binned, dVis, fb, counters);
		hipLaunchKernelGGL(fallback_kernel, dim3((unsigned)std::min<unsigned long long>((n + 255) / 256, 16), 64), kBlock, 0, s, fb, n, dXyz, dNv, v, dVis, counters);
		if (hipGetLastError() != hipSuccess) return fail("point_cloud_filter: launch failed");
	}
	(void)hipEventRecord(ev[1], s);
	unsigned long long hc[4];
	if (hipMemcpyAsync(hVis, dVis, n * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipStreamSynchronize(s) != hipSuccess)
		return fail("point_cloud_filter: device failure");
	st.candidates = hc[0]; st.hits = hc[1]; st.fallback = hc[2];
	(void)hipEventElapsedTime(&st.ms, ev[0], ev[1]);
	for (auto& e : ev) (void)hipEventDestroy(e);
	return 0;
}

} // namespace hcmvs

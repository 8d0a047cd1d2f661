/*
 * hc-mvs_amd/csrc/knn_grid.h -- exact k-nearest-neighbour search over a cloud on the device, shared by cloud_kernels.hip (point normals)
 * and prior_kernels.hip (plane priors).  HIP only: include it from a .hip file.
 *
 * The neighbours of a point are the k smallest by (squared distance in double from the float32 coordinates, original index); the
 * coordinates must be finite (the grid is undefined for others).
 *
 * Layout: the points are binned into a uniform grid (cell edge ~ sqrt(k/2 * surface area / n): a cloud is a surface, so about
 * k/2 points per occupied cell and the k nearest of a surface point lie within one cell of it) and sorted by the Morton code
 * of their cell (hipcub radix sort): a cell of ANY octree level -- 2^L cells on a side -- is then one contiguous range of the
 * sorted array, found by two binary searches.  One thread per point, in sorted order so that neighbouring threads search the
 * same ranges: level 0 looks at the 3 x 3 x 3 cells around the point, and as long as the k-th nearest candidate is farther
 * than one cell edge of the level (the margin inside which the block is complete) the search moves one level up -- exact
 * k-NN for every point, surface or outlier, at a cost that grows with the log of the distance to the k-th neighbour instead
 * of its cube.  The k best are kept sorted in registers.  HBM/L2-bound on the gathers of the candidate points.
 */
#ifndef HCMVS_KNN_GRID_H
#define HCMVS_KNN_GRID_H
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdint.h>

#include "knn_layout.h"

namespace hcmvs {

namespace {

constexpr int kKnnMaxK = 32;
constexpr uint32_t kKnnNone = 0xFFFFFFFFu;
static const dim3 kKnnGrid(2048), kKnnBlock(256);

struct Grid {
	float lo[3];
	double cell;
	long long dim[3];
};

__device__ __forceinline__ void cell_of(const Grid& g, const float* p, long long* c) {
#pragma unroll
	for (int q = 0; q < 3; ++q) {
		long long v = (long long)floor(((double)p[q] - (double)g.lo[q]) / g.cell);
		c[q] = v < 0 ? 0 : (v >= g.dim[q] ? g.dim[q] - 1 : v);
	}
}
__device__ __forceinline__ unsigned long long spread3(unsigned long long v) { // 21 bits -> every third bit
	v &= 0x1fffffull;
	v = (v | v << 32) & 0x1f00000000ffffull;
	v = (v | v << 16) & 0x1f0000ff0000ffull;
	v = (v | v << 8) & 0x100f00f00f00f00full;
	v = (v | v << 4) & 0x10c30c30c30c30c3ull;
	v = (v | v << 2) & 0x1249249249249249ull;
	return v;
}
__device__ __forceinline__ unsigned long long morton3(long long x, long long y, long long z) {
	return spread3((unsigned long long)x) | spread3((unsigned long long)y) << 1 | spread3((unsigned long long)z) << 2;
}
__device__ __forceinline__ unsigned long long lower_bound(const unsigned long long* keys, unsigned long long n, unsigned long long v) {
	unsigned long long lo = 0, hi = n;
	while (lo < hi) { const unsigned long long mid = (lo + hi) >> 1; if (keys[mid] < v) lo = mid + 1; else hi = mid; }
	return lo;
}

// ordered-int encoding of a float for atomicMin / atomicMax
__device__ __forceinline__ int f2ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }

__global__ void bbox_kernel(unsigned long long n, const float* xyz, int* box) { // box: min x y z | max x y z, ordered ints
	int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
	for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
#pragma unroll
		for (int q = 0; q < 3; ++q) { const int v = f2ord(xyz[3 * i + q]); lo[q] = v < lo[q] ? v : lo[q]; hi[q] = v > hi[q] ? v : hi[q]; }
#pragma unroll
	for (int q = 0; q < 3; ++q) {
		for (int o = 32; o > 0; o >>= 1) { const int a = __shfl_xor(lo[q], o, 64), b = __shfl_xor(hi[q], o, 64); lo[q] = a < lo[q] ? a : lo[q]; hi[q] = b > hi[q] ? b : hi[q]; }
		if ((threadIdx.x & 63) == 0) { atomicMin(&box[q], lo[q]); atomicMax(&box[3 + q], hi[q]); }
	}
}
__global__ void keys_kernel(unsigned long long n, const float* xyz, Grid g, unsigned long long* keys, uint32_t* idx) {
	for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
		long long c[3];
		cell_of(g, xyz + 3 * i, c);
		keys[i] = morton3(c[0], c[1], c[2]);
		idx[i] = (uint32_t)i;
	}
}
__global__ void gather_kernel(unsigned long long n, const float* xyz, const uint32_t* idx, float4* sorted) {
	for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t i = idx[j];
		sorted[j] = make_float4(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], __uint_as_float(i));
	}
}
__global__ void positions_kernel(unsigned long long n, const uint32_t* idx, uint32_t* posOf) {
	for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * blockDim.x) posOf[idx[j]] = (uint32_t)j;
}

// Jacobi rotations on a symmetric 3x3 (xx xy xz yy yz zz), double precision: a ends (nearly) diagonal, the columns of e are the eigenvectors
__device__ __forceinline__ void jacobi3(const double cov[6], double a[3][3], double e[3][3]) {
	a[0][0] = cov[0]; a[0][1] = cov[1]; a[0][2] = cov[2]; a[1][0] = cov[1]; a[1][1] = cov[3]; a[1][2] = cov[4]; a[2][0] = cov[2]; a[2][1] = cov[4]; a[2][2] = cov[5];
#pragma unroll
	for (int r = 0; r < 3; ++r)
#pragma unroll
		for (int q = 0; q < 3; ++q) e[r][q] = r == q ? 1 : 0;
	for (int sweep = 0; sweep < 32; ++sweep) {
		const double offd = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
		if (offd < 1e-300) break;
#pragma unroll
		for (int p = 0; p < 2; ++p)
#pragma unroll
			for (int q = p + 1; q < 3; ++q) {
				if (fabs(a[p][q]) < 1e-300) continue;
				const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
				const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
#pragma unroll
				for (int k = 0; k < 3; ++k) { const double akp = a[k][p], akq = a[k][q]; a[k][p] = cs * akp - sn * akq; a[k][q] = sn * akp + cs * akq; }
#pragma unroll
				for (int k = 0; k < 3; ++k) { const double apk = a[p][k], aqk = a[q][k]; a[p][k] = cs * apk - sn * aqk; a[q][k] = sn * apk + cs * aqk; }
#pragma unroll
				for (int k = 0; k < 3; ++k) { const double ekp = e[k][p], ekq = e[k][q]; e[k][p] = cs * ekp - sn * ekq; e[k][q] = sn * ekp + cs * ekq; }
			}
	}
}
__device__ __forceinline__ void smallest_eigenvector(const double cov[6], double* v) {
	double a[3][3], e[3][3];
	jacobi3(cov, a, e);
	const int m = a[1][1] < a[0][0] ? (a[2][2] < a[1][1] ? 2 : 1) : (a[2][2] < a[0][0] ? 2 : 0);
#pragma unroll
	for (int k = 0; k < 3; ++k) v[k] = m == 0 ? e[k][0] : (m == 1 ? e[k][1] : e[k][2]);
}

// The k nearest of p among the n sorted points, skipping the point whose original index is `exclude` (kKnnNone: none is skipped):
// bd / bi hold them ascending by (distance, original index), K is the compile-time capacity (k <= K).  Returns how many candidates the
// last level looked at: min(that, k) entries are valid.
template <int K>
__device__ __forceinline__ int knn_search(unsigned long long n, const float4* sorted, const unsigned long long* keys, const Grid& g, const float p[3], int k,
                                          uint32_t exclude, double (&bd)[K], uint32_t (&bi)[K]) {
	long long c[3];
	cell_of(g, p, c);
	int cnt = 0;
	for (int L = 0;; ++L) { // octree level: cells of 2^L grid cells on a side
		cnt = 0;
#pragma unroll
		for (int t = 0; t < K; ++t) { bd[t] = 1e300; bi[t] = 0xFFFFFFFFu; }
		const long long X = c[0] >> L, Y = c[1] >> L, Z = c[2] >> L;
		const long long DX = (g.dim[0] - 1) >> L, DY = (g.dim[1] - 1) >> L, DZ = (g.dim[2] - 1) >> L; // last cell of the level per axis
		const long long x0 = X > 0 ? X - 1 : 0, x1 = X < DX ? X + 1 : DX, y0 = Y > 0 ? Y - 1 : 0, y1 = Y < DY ? Y + 1 : DY, z0 = Z > 0 ? Z - 1 : 0, z1 = Z < DZ ? Z + 1 : DZ;
		for (long long z = z0; z <= z1; ++z)
			for (long long y = y0; y <= y1; ++y)
				for (long long x = x0; x <= x1; ++x) {
					const unsigned long long mc = morton3(x, y, z);
					const unsigned long long s0 = lower_bound(keys, n, mc << (3 * L)), s1 = lower_bound(keys, n, (mc + 1ull) << (3 * L));
					for (unsigned long long s = s0; s < s1; ++s) {
						const float4 q = sorted[s];
						const double dx = (double)q.x - p[0], dy = (double)q.y - p[1], dz = (double)q.z - p[2];
						const double d = dx * dx + dy * dy + dz * dz;
						const uint32_t qi = __float_as_uint(q.w);
						if (qi == exclude) continue;
						++cnt;
						if (!(d < bd[K - 1] || (d == bd[K - 1] && qi < bi[K - 1]))) continue;
						// sorted insertion with static indices: the newcomer bubbles up from the last place
						bool placed = false;
#pragma unroll
						for (int t = K - 1; t >= 0; --t) {
							const bool before = t > 0 && (d < bd[t > 0 ? t - 1 : 0] || (d == bd[t > 0 ? t - 1 : 0] && qi < bi[t > 0 ? t - 1 : 0]));
							if (!placed) {
								if (before) { bd[t] = bd[t > 0 ? t - 1 : 0]; bi[t] = bi[t > 0 ? t - 1 : 0]; }
								else { bd[t] = d; bi[t] = qi; placed = true; }
							}
						}
					}
				}
		if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == DX && y1 == DY && z1 == DZ) break; // the block was the whole grid
		if (cnt >= k) {
			double kth = bd[0]; // the k-th nearest (k <= K): bd is ascending
#pragma unroll
			for (int t = 0; t < K; ++t) if (t == k - 1) kth = bd[t];
			const double margin = g.cell * (double)(1ll << L); // everything closer than one cell of this level is inside the block
			if (kth <= margin * margin) break;
		}
	}
	return cnt;
}

// what the search reads of the index
struct KnnIndex {
	Grid g;
	const float4* sorted;            // x y z | original index, in cell order
	const unsigned long long* keys;  // the cell codes, ascending
	const uint32_t* posOf;           // original index -> place in sorted
};
inline size_t knn_sort_bytes(size_t n) {
	size_t bytes = 0;
	(void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
	return bytes;
}
inline KnnLayout knn_carve(Carve& carve, size_t n) { return knn_layout(carve, n, knn_sort_bytes(n)); }
// Builds the index of the n points at dXyz (device, 3 floats each, 0 < n < 2^31 - 1) for searches of k neighbours, in the pieces `l` of the
// allocation at b.  Waits for the stream once (the bounding box decides the grid).  Null = ok, otherwise what failed.
inline const char* knn_build(unsigned long long n, const float* dXyz, int k, char* b, const KnnLayout& l, hipStream_t s, KnnIndex& out) {
	unsigned long long *keys = (unsigned long long*)(b + l.keys), *keys2 = (unsigned long long*)(b + l.keys2);
	uint32_t *idx = (uint32_t*)(b + l.idx), *idx2 = (uint32_t*)(b + l.idx2), *posOf = (uint32_t*)(b + l.pos);
	float4* sorted = (float4*)(b + l.sorted);
	int* box = (int*)(b + l.box);
	const int boxInit[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000};
	if (hipMemcpyAsync(box, boxInit, sizeof boxInit, hipMemcpyHostToDevice, s) != hipSuccess) return "upload failed";
	hipLaunchKernelGGL(bbox_kernel, kKnnGrid, kKnnBlock, 0, s, n, dXyz, box);
	int hb[6];
	if (hipMemcpyAsync(hb, box, sizeof hb, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return "bounding box failed";
	auto ord2f = [](int v) { const int i = v >= 0 ? v : v ^ 0x7fffffff; float f; memcpy(&f, &i, 4); return f; };
	Grid g;
	double ext[3];
	for (int q = 0; q < 3; ++q) { g.lo[q] = ord2f(hb[q]); ext[q] = (double)ord2f(hb[3 + q]) - (double)g.lo[q]; }
	// the cloud is a surface: ~k/2 points per occupied cell when the cell edge is about sqrt(k/2 * area / n); area from the box
	const double area = std::max({ext[0] * ext[1], ext[0] * ext[2], ext[1] * ext[2], 1e-30});
	g.cell = std::max(std::sqrt(0.5 * (double)k * area / (double)n), 1e-12);
	const double longest = std::max({ext[0], ext[1], ext[2]});
	if (longest / g.cell > 1048575.0) g.cell = longest / 1048575.0; // 20 bits per axis in the cell key
	for (int q = 0; q < 3; ++q) g.dim[q] = (long long)std::floor(ext[q] / g.cell) + 1;
	hipLaunchKernelGGL(keys_kernel, kKnnGrid, kKnnBlock, 0, s, n, dXyz, g, keys, idx);
	size_t sortBytes = l.sortBytes;
	if (hipcub::DeviceRadixSort::SortPairs(b + l.sort, sortBytes, keys, keys2, idx, idx2, (int)n, 0, 64, s) != hipSuccess) return "sort failed";
	hipLaunchKernelGGL(gather_kernel, kKnnGrid, kKnnBlock, 0, s, n, dXyz, idx2, sorted);
	hipLaunchKernelGGL(positions_kernel, kKnnGrid, kKnnBlock, 0, s, n, idx2, posOf);
	if (hipGetLastError() != hipSuccess) return "launch failed";
	out.g = g; out.sorted = sorted; out.keys = keys2; out.posOf = posOf;
	return nullptr;
}

} // namespace

} // namespace hcmvs
#endif

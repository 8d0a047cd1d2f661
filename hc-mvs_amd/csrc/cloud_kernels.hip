/*
 * hc-mvs_amd/csrc/cloud_kernels.hip -- post-processing of the fused cloud on the device.
 *
 * MVS::EstimatePointNormals (frame_main/libs/MVS/DepthMap.cpp:2221-2269, --estimate-normals 1) calls
 * CGAL::pca_estimate_normals(points, k = 16): for every point the k nearest points (the point itself among them) are fitted
 * with a plane by principal component analysis and the plane normal becomes the point normal; the reference then flips it
 * towards the camera centre of the point's first view.  CGAL is absent: the k-nearest search and the PCA (covariance about
 * the centroid, smallest eigenvector by Jacobi rotations, double precision) are restated here; parity with CGAL unpinned.  The
 * neighbours are the k smallest by (squared distance in double, original index), so the result is defined up to the eigen-solver's
 * rounding; the coordinates are finite (the C-ABI entry refuses others: the grid below is undefined for them).
 *
 * The search itself (grid, Morton sort, level walk) lives in knn_grid.h, which the plane priors share; one thread per point, in sorted
 * order so that neighbouring threads search the same ranges.
 */
#include "cloud_kernels.h"
#include "knn_grid.h"

namespace hcmvs {

namespace {

// K: compile-time capacity of the candidate list (k <= K)
template <int K>
__global__ __launch_bounds__(256) void pca_normals_kernel(unsigned long long n, const float4* sorted, const unsigned long long* keys, const uint32_t* posOf, Grid g,
                                                          int k, const uint32_t* firstView, const double* viewC, float* normal) {
	for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * blockDim.x) {
		const float4 me = sorted[j];
		const float p[3] = {me.x, me.y, me.z};
		const uint32_t self = __float_as_uint(me.w); // original index
		double bd[K]; uint32_t bi[K]; // the best candidates, ascending (distance, index)
		const int cnt = knn_search<K>(n, sorted, keys, g, p, k, kKnnNone, bd, bi);
		const int m = cnt < k ? cnt : k;
		// centroid and covariance of the m nearest, summed in ascending (distance, index) order; bi holds original indices
		// (the tie-break of the order), posOf maps them to positions in the sorted array
		double mean[3] = {0, 0, 0}, cov[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
		for (int t = 0; t < K; ++t) if (t < m) { const float4 q = sorted[posOf[bi[t]]]; mean[0] += (double)q.x; mean[1] += (double)q.y; mean[2] += (double)q.z; }
		for (int q = 0; q < 3; ++q) mean[q] /= (double)m;
#pragma unroll
		for (int t = 0; t < K; ++t) if (t < m) {
			const float4 q = sorted[posOf[bi[t]]];
			const double d0 = (double)q.x - mean[0], d1 = (double)q.y - mean[1], d2 = (double)q.z - mean[2];
			cov[0] += d0 * d0; cov[1] += d0 * d1; cov[2] += d0 * d2; cov[3] += d1 * d1; cov[4] += d1 * d2; cov[5] += d2 * d2;
		}
		double v[3];
		smallest_eigenvector(cov, v);
		float nn[3] = {(float)v[0], (float)v[1], (float)v[2]};
		// correct the orientation: towards the camera of the first view (DepthMap.cpp:2262-2265)
		const double* C = viewC + 3 * (size_t)firstView[self];
		const float tc[3] = {(float)C[0] - p[0], (float)C[1] - p[1], (float)C[2] - p[2]};
		if (nn[0] * tc[0] + nn[1] * tc[1] + nn[2] * tc[2] < 0) { nn[0] = -nn[0]; nn[1] = -nn[1]; nn[2] = -nn[2]; }
		normal[3 * (size_t)self] = nn[0]; normal[3 * (size_t)self + 1] = nn[1]; normal[3 * (size_t)self + 2] = nn[2];
	}
}
} // namespace

int pca_normals_device(unsigned long long n, const float* hXyz, const uint32_t* hFirstView, const double* hViewC, size_t nViews, int k,
                       float* hNormal, DevBuf& scratch, hipStream_t s, std::string& err) {
	if (n == 0) return 0;
	if (k > kKnnMaxK) { err = "estimate_point_normals: k above 32"; return 1; }
	if (n >= 0x7FFFFFFFull) { err = "estimate_point_normals: more than 2^31 - 1 points"; return 1; }
	Carve carve;
	const size_t oXyz = carve(n * 12), oFirst = carve(n * 4), oC = carve(nViews * 24), oN = carve(n * 12);
	const KnnLayout lay = knn_carve(carve, n);
	if (scratch.reserve(carve.size, s) != hipSuccess) { err = "estimate_point_normals: out of device memory"; return 2; }
	char* b = scratch.get();
	auto fail = [&](const char* what) { err = what; return 2; };
	float* dXyz = (float*)(b + oXyz);
	uint32_t* first = (uint32_t*)(b + oFirst);
	double* dC = (double*)(b + oC);
	float* dN = (float*)(b + oN);
	if (hipMemcpyAsync(dXyz, hXyz, n * 12, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(first, hFirstView, n * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
	    hipMemcpyAsync(dC, hViewC, nViews * 24, hipMemcpyHostToDevice, s) != hipSuccess)
		return fail("estimate_point_normals: upload failed");
	KnnIndex ix;
	if (const char* what = knn_build(n, dXyz, k, b, lay, s, ix)) { err = std::string("estimate_point_normals: ") + what; return 2; }
	if (k <= 16) hipLaunchKernelGGL(pca_normals_kernel<16>, kKnnGrid, kKnnBlock, 0, s, n, ix.sorted, ix.keys, ix.posOf, ix.g, k, first, dC, dN);
	else hipLaunchKernelGGL(pca_normals_kernel<32>, kKnnGrid, kKnnBlock, 0, s, n, ix.sorted, ix.keys, ix.posOf, ix.g, k, first, dC, dN);
	if (hipGetLastError() != hipSuccess) return fail("estimate_point_normals: launch failed");
	if (hipMemcpyAsync(hNormal, dN, n * 12, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("estimate_point_normals: device failure");
	return 0;
}

} // namespace hcmvs

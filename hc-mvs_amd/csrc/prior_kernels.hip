/*
 * hc-mvs_amd/csrc/prior_kernels.hip -- depth priors from planes fitted to a labelled region of a half-finished depth map.
 *
 * DepthMapsData::GenerateDepthPrior (frame_main/libs/MVS/SceneDensify.cpp:1550-1950) back-projects the confident pixels of a semantic region,
 * keeps the locally planar ones (CGAL::vcm / pca), removes sparse outliers (CGAL::remove_outliers), detects planes with CGAL's Efficient
 * RANSAC, frames every plane's inliers with a rectangle on the plane and renders, per pixel, the depth of the plane whose projected
 * rectangle holds the pixel.  CGAL is absent and its RANSAC is randomised: the stages are restated, parity with
 * CGAL unpinned.  Everything is in the camera frame of the view (every step is rigid-invariant).
 *
 * S1  samples in raster order: flags, an exclusive scan (hipcub), a gather.
 * S2  planarity over the k nearest samples: the search of knn_grid.h, covariance and Jacobi eigenvalues in double.
 * S3  spacing: mean distance to the k nearest OTHER samples; the averages are sums of round(s * 2^40) in two integer words, so they
 *     do not depend on the order of the atomics.
 * S4  rounds of 256 candidates: one workgroup builds the candidate planes (counter-based draws), the scoring kernel holds one sample per
 *     lane in registers and walks the 4 KiB candidate table, which is uniform across the wave (scalar loads): four ballots and
 *     popcounts per candidate, added by one lane into LDS counters of the workgroup, then one integer global atomic per non-zero
 *     counter and workgroup.  One workgroup ranks the counters; only the winner (a few words) travels to the host.
 * S4r (refit_iters > 0) the winner is refitted by total least squares over its inliers in the eps / 4 band: one kernel gives a plane's four
 *     counts and the nine moment sums of its band as exact integers (registers, wave shuffles, LDS, integer atomics), the host solves the
 *     3 x 3 eigenproblem (prior_gen_plan.h) and the next plane goes back as kernel arguments; at most refit_iters + 1 launches a round.
 * S4c (cluster_mul > 0) the winner's inliers keep their largest connected component on a grid of cells in the plane: cell keys, a radix
 *     sort (hipcub), the distinct cells, a union-find over them (neighbours by binary search), integer sizes, one packed maximum; the
 *     arrays live in the scratch of the neighbour search, which is idle during S4.  A 16-byte record travels to the host.
 * S5  per-plane reductions into integer words (fixed-point coordinate sums, pixel box, then the extent in the plane's frame as ordered
 *     doubles -- min and max do not depend on the order either); the frame and the quad are the host's (prior_gen_plan.h).
 * S6  render: one thread per pixel over the plane table.
 * The scoring kernel is VALU-bound (~20 instructions per sample and candidate); no float atomics anywhere.
 */
#include "prior_kernels.h"
#include "knn_grid.h"

#include <chrono>
#include <vector>

namespace hcmvs {

namespace {

constexpr int kBlockSize = 256;
constexpr int kScoreMaxBlocks = 1024;

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) { // the splitmix64 step (DESIGN.md section 5, D11 of the mesh sampling)
	z += 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ double draw(unsigned long long a, unsigned long long k) { return (double)(mix64(a + k * 0xD1B54A32D192ED03ull) >> 11) * 0x1p-53; }
// floor(U * n) kept below n
__host__ __device__ __forceinline__ unsigned long long draw_below(unsigned long long a, unsigned long long k, unsigned long long n) {
	const unsigned long long v = (unsigned long long)(draw(a, k) * (double)n);
	return v < n ? v : n - 1;
}
__device__ __forceinline__ bool usable_depth(float d) { return d > 0.f && d <= 3.402823466e+38f; } // finite and > 0

struct Kinv { double i[6]; };
__device__ __forceinline__ void ray_of(const Kinv& k, int x, int y, float r[3]) {
	r[0] = (float)((k.i[0] * (double)x + k.i[1] * (double)y) + k.i[2]);
	r[1] = (float)((k.i[3] * (double)x + k.i[4] * (double)y) + k.i[5]);
	r[2] = 1.f;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// ---- S1 ----
// flags[i] = pixel i is a sample; stage[i] = 0 outside the region, 1 region, 2 sample; words[0] += region pixels.  A pixel whose point
// ray * depth is not finite in float32 (a huge depth, which the caller owns) is no sample: the search grid is undefined for such points
__global__ __launch_bounds__(kBlockSize) void sample_flags_kernel(unsigned px, int w, Kinv kinv, const uint8_t* region, const float* depth, const float* conf, float confMax,
                                                                  uint32_t* flags, uint8_t* stage, unsigned long long* words) {
	unsigned long long inside = 0;
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < px; i += gridDim.x * blockDim.x) {
		const bool in = region[i] == 0;
		bool smp = in && usable_depth(depth[i]) && conf[i] < confMax;
		if (smp) {
			float r[3];
			ray_of(kinv, (int)(i % (unsigned)w), (int)(i / (unsigned)w), r);
			const float d = depth[i];
			smp = fabsf(r[0] * d) <= 3.402823466e+38f && fabsf(r[1] * d) <= 3.402823466e+38f; // (r[2] * d = d)
		}
		flags[i] = smp ? 1u : 0u;
		stage[i] = in ? (smp ? 2 : 1) : 0;
		inside += in ? 1 : 0;
	}
	inside = wave_sum(inside);
	if ((threadIdx.x & 63) == 0 && inside) atomicAdd(&words[0], inside);
	if (blockIdx.x == 0 && threadIdx.x == 0) flags[px] = 0; // the scan runs over px + 1 items: scan[px] is the total
}
__global__ __launch_bounds__(kBlockSize) void gather_samples_kernel(unsigned px, int w, Kinv kinv, const float* depth, const float* normal, const uint32_t* flags,
                                                                    const uint32_t* scan, float* xyz, float* nrm, int32_t* pix) {
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < px; i += gridDim.x * blockDim.x) {
		if (!flags[i]) continue;
		const size_t j = scan[i];
		float r[3];
		ray_of(kinv, (int)(i % (unsigned)w), (int)(i / (unsigned)w), r);
		const float d = depth[i];
		xyz[3 * j] = r[0] * d; xyz[3 * j + 1] = r[1] * d; xyz[3 * j + 2] = r[2] * d;
		nrm[3 * j] = normal[3 * (size_t)i]; nrm[3 * j + 1] = normal[3 * (size_t)i + 1]; nrm[3 * j + 2] = normal[3 * (size_t)i + 2];
		pix[j] = (int32_t)i;
	}
}
// the flagged samples of one set move to the other in order; their pixels reach the stage `mark`
__global__ __launch_bounds__(kBlockSize) void compact_kernel(unsigned n, const uint32_t* flags, const uint32_t* scan, const float* sx, const float* sn, const int32_t* sp,
                                                             float* dx, float* dn, int32_t* dp, uint8_t* stage, uint8_t mark) {
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		if (!flags[i]) continue;
		const size_t j = scan[i];
#pragma unroll
		for (int q = 0; q < 3; ++q) { dx[3 * j + q] = sx[3 * (size_t)i + q]; dn[3 * j + q] = sn[3 * (size_t)i + q]; }
		dp[j] = sp[i];
		stage[sp[i]] = mark;
	}
}

// ---- S2 ----
template <int K>
__global__ __launch_bounds__(kBlockSize) void planarity_kernel(unsigned long long n, const float4* sorted, const unsigned long long* keys, const uint32_t* posOf, Grid g, int k,
                                                               double planarityMin, uint32_t* flags) {
	for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * blockDim.x) {
		const float4 me = sorted[j];
		const float p[3] = {me.x, me.y, me.z};
		const uint32_t self = __float_as_uint(me.w);
		double bd[K]; uint32_t bi[K];
		(void)knn_search<K>(n, sorted, keys, g, p, k, kKnnNone, bd, bi); // n > k: all k are found
		double mean[3] = {0, 0, 0}, cov[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
		for (int t = 0; t < K; ++t) if (t < k) { const float4 q = sorted[posOf[bi[t]]]; mean[0] += (double)q.x; mean[1] += (double)q.y; mean[2] += (double)q.z; }
		for (int q = 0; q < 3; ++q) mean[q] /= (double)k;
#pragma unroll
		for (int t = 0; t < K; ++t) if (t < k) {
			const float4 q = sorted[posOf[bi[t]]];
			const double d0 = (double)q.x - mean[0], d1 = (double)q.y - mean[1], d2 = (double)q.z - mean[2];
			cov[0] += d0 * d0; cov[1] += d0 * d1; cov[2] += d0 * d2; cov[3] += d1 * d1; cov[4] += d1 * d2; cov[5] += d2 * d2;
		}
		double a[3][3], e[3][3];
		jacobi3(cov, a, e);
		double l0 = a[0][0], l1 = a[1][1], l2 = a[2][2], t;
		if (l1 < l0) { t = l0; l0 = l1; l1 = t; }
		if (l2 < l1) { t = l1; l1 = l2; l2 = t; }
		if (l1 < l0) { t = l0; l0 = l1; l1 = t; }
		const double pl = l2 > 0.0 ? (l1 - l0) / l2 : 0.0;
		flags[self] = pl >= planarityMin ? 1u : 0u;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = 0;
}

// ---- S3 ----
// spacing[i] = mean distance to the k nearest other samples (sqrt in double, added in ascending (distance, index) order);
// words[0] / words[1] += the high / low parts of round(s * 2^40)
template <int K>
__global__ __launch_bounds__(kBlockSize) void spacing_kernel(unsigned long long n, const float4* sorted, const unsigned long long* keys, Grid g, int k, double* spacing,
                                                             unsigned long long* words) {
	unsigned long long hi = 0, lo = 0;
	for (unsigned long long j = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; j < n; j += (unsigned long long)gridDim.x * blockDim.x) {
		const float4 me = sorted[j];
		const float p[3] = {me.x, me.y, me.z};
		const uint32_t self = __float_as_uint(me.w);
		double bd[K]; uint32_t bi[K];
		(void)knn_search<K>(n, sorted, keys, g, p, k, self, bd, bi); // n > k: k others exist
		double sum = 0;
#pragma unroll
		for (int t = 0; t < K; ++t) if (t < k) sum += sqrt(bd[t]);
		const double sp = sum / (double)k;
		spacing[self] = sp;
		const double scaled = (sp < 8388608.0 ? sp : 8388607.0) * 0x1p40; // saturated below 2^23
		const unsigned long long q = (unsigned long long)rint(scaled);
		hi += q >> 32; lo += q & 0xffffffffull;
	}
	hi = wave_sum(hi); lo = wave_sum(lo);
	if ((threadIdx.x & 63) == 0) { if (hi) atomicAdd(&words[0], hi); if (lo) atomicAdd(&words[1], lo); }
}
__global__ __launch_bounds__(kBlockSize) void outlier_flags_kernel(unsigned n, const double* spacing, double avg, uint32_t* flags) {
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) flags[i] = spacing[i] > avg ? 0u : 1u;
	if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = 0;
}

// ---- S4 ----
__global__ __launch_bounds__(kBlockSize) void fill_i32_kernel(unsigned n, int32_t* a, int32_t v) {
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) a[i] = v;
}
__global__ __launch_bounds__(kBlockSize) void index_samples_kernel(unsigned n, const int32_t* pix, int32_t* sampleAt) {
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) sampleAt[pix[i]] = (int32_t)i;
}
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// one workgroup, candidate c = threadIdx.x of the round: cand[c] = (n, d), d = NaN when the candidate is invalid; zeroes the counters
__global__ __launch_bounds__(kPriorCandidates) void candidate_kernel(unsigned round, unsigned long long seed, unsigned n0, int w, int h, const int32_t* levels, int nLevels,
                                                                     const float* xyz, const float* nrm, const int32_t* pix, const int32_t* sampleAt,
                                                                     const int32_t* assigned, float normalThr, float4* cand, uint32_t* counts) {
	const unsigned c = threadIdx.x;
#pragma unroll
	for (int q = 0; q < 4; ++q) counts[4 * c + q] = 0;
	const float nan = __int_as_float(0x7fc00000);
	float4 out = make_float4(0.f, 0.f, 0.f, nan);
	const unsigned long long a = mix64(seed ^ mix64((unsigned long long)round * kPriorCandidates + c));
	const unsigned ia = (unsigned)draw_below(a, 0, n0);
	const int rho = levels[(int)draw_below(a, 1, (unsigned long long)nLevels)];
	const unsigned long long span = 2ull * (unsigned long long)rho + 1ull;
	int off[4];
#pragma unroll
	for (int q = 0; q < 4; ++q) off[q] = (int)draw_below(a, 2 + q, span) - rho;
	const int pa = pix[ia], ax = pa % w, ay = pa / w;
	const int bx = ax + off[0], by = ay + off[1], cx = ax + off[2], cy = ay + off[3];
	bool ok = assigned[ia] < 0 && bx >= 0 && bx < w && by >= 0 && by < h && cx >= 0 && cx < w && cy >= 0 && cy < h;
	int ib = -1, ic = -1;
	if (ok) {
		ib = sampleAt[(size_t)by * w + bx]; ic = sampleAt[(size_t)cy * w + cx];
		ok = ib >= 0 && ic >= 0 && ib != (int)ia && ic != (int)ia && ib != ic;
		if (ok) ok = assigned[ib] < 0 && assigned[ic] < 0;
	}
	if (ok) {
		const float* A = xyz + 3 * (size_t)ia; const float* B = xyz + 3 * (size_t)ib; const float* Cc = xyz + 3 * (size_t)ic;
		const float u0 = B[0] - A[0], u1 = B[1] - A[1], u2 = B[2] - A[2], v0 = Cc[0] - A[0], v1 = Cc[1] - A[1], v2 = Cc[2] - A[2];
		float nx = u1 * v2 - u2 * v1, ny = u2 * v0 - u0 * v2, nz = u0 * v1 - u1 * v0;
		const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
		ok = len > 0.f && len <= 3.402823466e+38f;
		if (ok) {
			nx = nx / len; ny = ny / len; nz = nz / len;
			const float d = dot3(nx, ny, nz, A[0], A[1], A[2]);
			ok = fabsf(d) <= 3.402823466e+38f;
			const int ids[3] = {(int)ia, ib, ic};
#pragma unroll
			for (int q = 0; q < 3; ++q) {
				const float* N = nrm + 3 * (size_t)ids[q];
				ok = ok && fabsf(dot3(nx, ny, nz, N[0], N[1], N[2])) >= normalThr;
			}
			if (ok) out = make_float4(nx, ny, nz, d);
		}
	}
	cand[c] = out;
}

// The hot loop: every unassigned sample against the 256 candidates of the round.  One sample per lane in registers; the candidate is
// uniform across the wave; cnt_k = samples with |n . N| >= normalThr and |n . P - d| <= eps / 2^k
__global__ __launch_bounds__(kBlockSize) void score_kernel(unsigned n0, const float* __restrict__ xyz, const float* __restrict__ nrm, const int32_t* __restrict__ assigned,
                                                           const float4* __restrict__ cand, float normalThr, float eps, uint32_t* counts) {
	__shared__ uint32_t acc[kPriorCandidates * 4];
	for (int t = threadIdx.x; t < kPriorCandidates * 4; t += kBlockSize) acc[t] = 0;
	__syncthreads();
	const float e0 = eps, e1 = eps * 0.5f, e2 = eps * 0.25f, e3 = eps * 0.125f;
	const bool first = (threadIdx.x & 63) == 0;
	for (unsigned base = blockIdx.x * kBlockSize; base < n0; base += gridDim.x * kBlockSize) { // uniform per workgroup
		const unsigned i = base + threadIdx.x;
		const bool live = i < n0 && assigned[i] < 0;
		float px = 0.f, py = 0.f, pz = 0.f, qx = 0.f, qy = 0.f, qz = 0.f;
		if (live) { px = xyz[3 * (size_t)i]; py = xyz[3 * (size_t)i + 1]; pz = xyz[3 * (size_t)i + 2]; qx = nrm[3 * (size_t)i]; qy = nrm[3 * (size_t)i + 1]; qz = nrm[3 * (size_t)i + 2]; }
		if (__ballot(live) == 0ull) continue; // (per wave)
		for (int c = 0; c < kPriorCandidates; ++c) {
			const float4 pl = cand[c];
			if (pl.w != pl.w) continue; // invalid candidate: uniform
			const bool facing = live && fabsf(dot3(pl.x, pl.y, pl.z, qx, qy, qz)) >= normalThr;
			const float r = fabsf(dot3(pl.x, pl.y, pl.z, px, py, pz) - pl.w);
			const unsigned long long b0 = __ballot(facing && r <= e0);
			if (b0 == 0ull) continue; // the narrower bands are subsets
			const unsigned long long b1 = __ballot(facing && r <= e1), b2 = __ballot(facing && r <= e2), b3 = __ballot(facing && r <= e3);
			if (first) {
				atomicAdd(&acc[4 * c], (uint32_t)__popcll(b0));
				if (b1) atomicAdd(&acc[4 * c + 1], (uint32_t)__popcll(b1));
				if (b2) atomicAdd(&acc[4 * c + 2], (uint32_t)__popcll(b2));
				if (b3) atomicAdd(&acc[4 * c + 3], (uint32_t)__popcll(b3));
			}
		}
	}
	__syncthreads();
	for (int t = threadIdx.x; t < kPriorCandidates * 4; t += kBlockSize) if (acc[t]) atomicAdd(&counts[t], acc[t]);
}

// one workgroup: the qualifying candidate with the largest cnt_0 + .. + cnt_3, the lowest index on ties.
// winner: int32 [0] candidate or -1, [1..4] its counts, [5] valid candidates of the round, [8..11] its plane (float4)
__global__ __launch_bounds__(kPriorCandidates) void winner_kernel(const float4* cand, const uint32_t* counts, unsigned long long minPoints, int32_t* winner) {
	__shared__ unsigned long long best;
	__shared__ unsigned valid;
	const unsigned c = threadIdx.x;
	if (c == 0) { best = 0; valid = 0; }
	__syncthreads();
	const float4 pl = cand[c];
	const bool ok = pl.w == pl.w;
	if (ok) atomicAdd(&valid, 1u);
	const unsigned long long c0 = counts[4 * c];
	if (ok && c0 >= minPoints) {
		const unsigned long long sum = (c0 + counts[4 * c + 1]) + ((unsigned long long)counts[4 * c + 2] + counts[4 * c + 3]);
		atomicMax(&best, ((sum + 1ull) << 8) | (unsigned long long)(255u - c));
	}
	__syncthreads();
	if (c == 0) {
		const int win = best ? (int)(255u - (unsigned)(best & 255ull)) : -1;
		winner[0] = win; winner[5] = (int32_t)valid;
		for (int q = 0; q < 4; ++q) winner[1 + q] = win >= 0 ? (int32_t)counts[4 * win + q] : 0;
		const float4 w4 = win >= 0 ? cand[win] : make_float4(0.f, 0.f, 0.f, 0.f);
		((float*)winner)[8] = w4.x; ((float*)winner)[9] = w4.y; ((float*)winner)[10] = w4.z; ((float*)winner)[11] = w4.w;
	}
}
// the cnt_0 inliers of the round's winner leave the pool (the plane is read from the winner record: no host value is waited for)
__global__ __launch_bounds__(kBlockSize) void assign_kernel(unsigned n0, const float* xyz, const float* nrm, const int32_t* winner, float normalThr, float eps, int32_t plane,
                                                            int32_t* assigned) {
	if (winner[0] < 0) return;
	const float nx = ((const float*)winner)[8], ny = ((const float*)winner)[9], nz = ((const float*)winner)[10], d = ((const float*)winner)[11];
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += gridDim.x * blockDim.x) {
		if (assigned[i] >= 0) continue;
		const float* N = nrm + 3 * (size_t)i; const float* P = xyz + 3 * (size_t)i;
		if (fabsf(dot3(nx, ny, nz, N[0], N[1], N[2])) >= normalThr && fabsf(dot3(nx, ny, nz, P[0], P[1], P[2]) - d) <= eps) assigned[i] = plane;
	}
}

// ---- S4r ----
// One pass over the fitting set for one plane: its four counts, as score_kernel counts them, and the nine moment sums of its e2 band about
// the anchor O at the scale 2^-E, as exact integers (two words each: high and low part of every addend).  Registers, wave shuffles of
// 64-bit integers, LDS, one integer global atomic per non-zero word and workgroup: the result does not depend on the order.
// rec: kPriorRefitWords words -- 0..3 cnt_0 .. cnt_3, 4..21 hi / lo of the sums x y z xx xy xz yy yz zz, 22 / 23 the anchor as the host
// reads it (the float32 bits of x | y << 32, of z): the host knows the anchor's index from the counter stream, not its position.
// inv = 2^-E
constexpr int kRefitUsed = 22;
__global__ void refit_reset_kernel(unsigned long long* rec) {
	if (threadIdx.x < kPriorRefitWords) rec[threadIdx.x] = 0ull;
}
__global__ __launch_bounds__(kBlockSize) void refit_moments_kernel(unsigned n0, const float* __restrict__ xyz, const float* __restrict__ nrm, const int32_t* __restrict__ assigned,
                                                                   float4 pl, float normalThr, float eps, unsigned anchor, double inv, unsigned long long* rec) {
	__shared__ unsigned long long sh[kRefitUsed];
	if (threadIdx.x < kRefitUsed) sh[threadIdx.x] = 0ull;
	__syncthreads();
	const float ax = xyz[3 * (size_t)anchor], ay = xyz[3 * (size_t)anchor + 1], az = xyz[3 * (size_t)anchor + 2]; // anchor < n0 (draw_below)
	const double o[3] = {(double)ax, (double)ay, (double)az};
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		rec[22] = (unsigned long long)__float_as_uint(ax) | (unsigned long long)__float_as_uint(ay) << 32;
		rec[23] = (unsigned long long)__float_as_uint(az);
	}
	const float e0 = eps, e1 = eps * 0.5f, e2 = eps * 0.25f, e3 = eps * 0.125f;
	unsigned long long acc[kRefitUsed];
#pragma unroll
	for (int q = 0; q < kRefitUsed; ++q) acc[q] = 0ull;
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += gridDim.x * blockDim.x) {
		if (assigned[i] >= 0) continue;
		const float* N = nrm + 3 * (size_t)i; const float* P = xyz + 3 * (size_t)i;
		if (!(fabsf(dot3(pl.x, pl.y, pl.z, N[0], N[1], N[2])) >= normalThr)) continue;
		const float r = fabsf(dot3(pl.x, pl.y, pl.z, P[0], P[1], P[2]) - pl.w);
		if (!(r <= e0)) continue;
		acc[0] += 1ull; acc[1] += r <= e1 ? 1ull : 0ull; acc[3] += r <= e3 ? 1ull : 0ull;
		if (!(r <= e2)) continue;
		acc[2] += 1ull;
		double sv[3];
#pragma unroll
		for (int q = 0; q < 3; ++q) {
			const double v = ((double)P[q] - o[q]) * inv;
			sv[q] = v < 1048576.0 ? (v > -1048576.0 ? v : -1048575.0) : 1048575.0; // saturated inside (-2^20, 2^20)
			const long long fx = (long long)rint(sv[q] * 0x1p24);
			acc[4 + 2 * q] += (unsigned long long)(fx >> 32); acc[5 + 2 * q] += (unsigned long long)fx & 0xffffffffull;
		}
		const double pr[6] = {sv[0] * sv[0], sv[0] * sv[1], sv[0] * sv[2], sv[1] * sv[1], sv[1] * sv[2], sv[2] * sv[2]};
#pragma unroll
		for (int q = 0; q < 6; ++q) {
			const long long fx = (long long)rint(pr[q] * 0x1p20); // |s_a s_b| < 2^40: below 2^60
			acc[10 + 2 * q] += (unsigned long long)(fx >> 32); acc[11 + 2 * q] += (unsigned long long)fx & 0xffffffffull;
		}
	}
#pragma unroll
	for (int q = 0; q < kRefitUsed; ++q) {
		const unsigned long long v = wave_sum(acc[q]);
		if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh[q], v);
	}
	__syncthreads();
	if (threadIdx.x < kRefitUsed && sh[threadIdx.x]) atomicAdd(&rec[threadIdx.x], sh[threadIdx.x]);
}

__device__ __forceinline__ unsigned long long ordered(double v) {
	const unsigned long long b = (unsigned long long)__double_as_longlong(v);
	return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_ordered_dev(unsigned long long k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k)); }

// ---- S4c ----
// The winner's inliers on a grid of cells in the plane's frame; the largest 8-connected component is the plane.  Sparse: every array is
// bounded by the number of samples, whatever the extent of the plane in cells.  Nothing depends on the order the threads run in: the
// origin is a minimum of ordered doubles, a component's label is the smallest index among its cells (the distinct cell keys ascending:
// (cv, cu) lexicographically), sizes are integer sums, the pick is one packed maximum.
// rec (unsigned long long words): 0 / 1 ordered u0 / v0; 2 the pick (size << 32 | ~label); 3 inliers; 4 components;
// then, as int32 from word 8: occupied cells, components, size of the pick, accepted
struct ClusterFrame { double b1[3], b2[3], cell; };
constexpr int kClusterRecOut = 8;

struct WinnerPlane { float nx, ny, nz, d; };
__device__ __forceinline__ WinnerPlane winner_plane(const int32_t* winner) {
	const float* f = (const float*)winner;
	return {f[8], f[9], f[10], f[11]};
}
// the set assign_kernel takes
__device__ __forceinline__ bool is_inlier(const WinnerPlane& pl, const float* xyz, const float* nrm, const int32_t* assigned, unsigned i, float normalThr, float eps) {
	if (assigned[i] >= 0) return false;
	const float* N = nrm + 3 * (size_t)i; const float* P = xyz + 3 * (size_t)i;
	return fabsf(dot3(pl.nx, pl.ny, pl.nz, N[0], N[1], N[2])) >= normalThr && fabsf(dot3(pl.nx, pl.ny, pl.nz, P[0], P[1], P[2]) - pl.d) <= eps;
}
__device__ __forceinline__ void plane_coords(const ClusterFrame& f, const float* P, double& u, double& v) {
	const double x = (double)P[0], y = (double)P[1], z = (double)P[2];
	u = (x * f.b1[0] + y * f.b1[1]) + z * f.b1[2];
	v = (x * f.b2[0] + y * f.b2[1]) + z * f.b2[2];
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
	for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o, 64); v = t < v ? t : v; }
	return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
	for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
	return v;
}
__global__ void cluster_reset_kernel(unsigned long long* rec) {
	if (threadIdx.x < 16) rec[threadIdx.x] = threadIdx.x < 2 ? ~0ull : 0ull;
}
__global__ __launch_bounds__(kBlockSize) void cluster_origin_kernel(unsigned n0, const float* xyz, const float* nrm, const int32_t* assigned, const int32_t* winner, float normalThr,
                                                                    float eps, ClusterFrame f, unsigned long long* rec) {
	__shared__ unsigned long long sh[2];
	if (threadIdx.x < 2) sh[threadIdx.x] = ~0ull;
	__syncthreads();
	const WinnerPlane pl = winner_plane(winner);
	unsigned long long mu = ~0ull, mv = ~0ull;
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += gridDim.x * blockDim.x) {
		if (!is_inlier(pl, xyz, nrm, assigned, i, normalThr, eps)) continue;
		double u, v;
		plane_coords(f, xyz + 3 * (size_t)i, u, v);
		const unsigned long long ou = ordered(u), ov = ordered(v);
		mu = ou < mu ? ou : mu; mv = ov < mv ? ov : mv;
	}
	mu = wave_min(mu); mv = wave_min(mv);
	if ((threadIdx.x & 63) == 0) { if (mu != ~0ull) atomicMin(&sh[0], mu); if (mv != ~0ull) atomicMin(&sh[1], mv); }
	__syncthreads();
	if (threadIdx.x < 2 && sh[threadIdx.x] != ~0ull) atomicMin(&rec[threadIdx.x], sh[threadIdx.x]);
}
// keys[i] = cv << 32 | cu of an inlier, all ones otherwise; idx[i] = i
__global__ __launch_bounds__(kBlockSize) void cluster_keys_kernel(unsigned n0, const float* xyz, const float* nrm, const int32_t* assigned, const int32_t* winner, float normalThr,
                                                                  float eps, ClusterFrame f, const unsigned long long* rec, unsigned long long* keys, uint32_t* idx) {
	const WinnerPlane pl = winner_plane(winner);
	const double u0 = from_ordered_dev(rec[0]), v0 = from_ordered_dev(rec[1]);
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += gridDim.x * blockDim.x) {
		unsigned long long key = ~0ull;
		if (is_inlier(pl, xyz, nrm, assigned, i, normalThr, eps)) {
			double u, v;
			plane_coords(f, xyz + 3 * (size_t)i, u, v);
			const double cu = fmin(floor((u - u0) / f.cell), (double)kPriorClusterCellCap), cv = fmin(floor((v - v0) / f.cell), (double)kPriorClusterCellCap); // >= 0: u0, v0 are minima
			key = (unsigned long long)cv << 32 | (unsigned long long)cu;
		}
		keys[i] = key; idx[i] = i;
	}
}
// over the sorted keys: marks[j] = entry j is the first of its cell; rec[3] = the inliers (they sort before the others)
__global__ __launch_bounds__(kBlockSize) void cluster_marks_kernel(unsigned n0, const unsigned long long* keys, uint32_t* marks, unsigned long long* rec) {
	for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < n0; j += gridDim.x * blockDim.x) {
		const unsigned long long k = keys[j];
		const bool in = k != ~0ull;
		marks[j] = in && (j == 0 || keys[j - 1] != k) ? 1u : 0u;
		if (in && (j + 1 == n0 || keys[j + 1] == ~0ull)) rec[3] = (unsigned long long)j + 1ull;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) marks[n0] = 0;
}
// the distinct cells: key, first entry, a union-find node of its own, an empty size
__global__ __launch_bounds__(kBlockSize) void cluster_cells_kernel(unsigned n0, const unsigned long long* keys, const uint32_t* marks, const uint32_t* scan, unsigned long long* cells,
                                                                   uint32_t* start, uint32_t* parent, uint32_t* sizes) {
	for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < n0; j += gridDim.x * blockDim.x) {
		if (!marks[j]) continue;
		const uint32_t d = scan[j];
		cells[d] = keys[j]; start[d] = j; parent[d] = d; sizes[d] = 0;
	}
}
// Union-find over the cells while other workgroups hook: a parent only ever decreases, so a value read late is still an ancestor; the
// reads go to the device's coherent level (another XCD's hook is seen), and a hook is a compare-and-swap on a node that is its own parent
__device__ __forceinline__ uint32_t uf_root(uint32_t* parent, uint32_t x) {
	for (;;) {
		const uint32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (p == x) return x;
		x = p;
	}
}
__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
	for (;;) {
		a = uf_root(parent, a); b = uf_root(parent, b);
		if (a == b) return;
		if (a < b) { const uint32_t t = a; a = b; b = t; } // the larger root goes under the smaller
		const uint32_t old = atomicCAS(&parent[a], a, b);
		if (old == a) return;
		a = old; // someone hooked a first: go on from where it points (strictly smaller: the loop ends)
	}
}
// every cell unites with its neighbours that come later in key order -- (cv, cu + 1) is the next cell if it exists, (cv + 1, cu - 1 .. cu + 1)
// are contiguous: one binary search -- which covers all 8 directions
__global__ __launch_bounds__(kBlockSize) void cluster_union_kernel(unsigned n0, const uint32_t* scan, const unsigned long long* cells, uint32_t* parent) {
	const uint32_t m = scan[n0];
	for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < m; d += gridDim.x * blockDim.x) {
		const unsigned long long key = cells[d], cu = key & 0xffffffffull, row = (key >> 32) + 1ull;
		if (d + 1 < m && cells[d + 1] == key + 1ull) uf_unite(parent, d, d + 1); // (cu <= 2^30: no carry into cv)
		const unsigned long long first = row << 32 | (cu > 0 ? cu - 1ull : 0ull), last = row << 32 | (cu + 1ull);
		for (unsigned long long e = lower_bound(cells, m, first); e < m && cells[e] <= last; ++e) uf_unite(parent, d, (uint32_t)e);
	}
}
// parent[d] = the root; the samples of the cell are added to the root's size
__global__ __launch_bounds__(kBlockSize) void cluster_sizes_kernel(unsigned n0, const uint32_t* scan, const uint32_t* start, const unsigned long long* rec, uint32_t* parent,
                                                                   uint32_t* sizes) {
	const uint32_t m = scan[n0], nIn = (uint32_t)rec[3];
	for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < m; d += gridDim.x * blockDim.x) {
		const uint32_t r = uf_root(parent, d);
		parent[d] = r; // (whoever walks through d meets an ancestor either way)
		atomicAdd(&sizes[r], (d + 1 < m ? start[d + 1] : nIn) - start[d]);
	}
}
__global__ __launch_bounds__(kBlockSize) void cluster_pick_kernel(unsigned n0, const uint32_t* scan, const uint32_t* parent, const uint32_t* sizes, unsigned long long* rec) {
	const uint32_t m = scan[n0];
	unsigned long long best = 0, roots = 0;
	for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < m; d += gridDim.x * blockDim.x) {
		if (parent[d] != d) continue;
		const unsigned long long cand = (unsigned long long)sizes[d] << 32 | (unsigned long long)(~d); // equal sizes: the smallest label
		best = cand > best ? cand : best; ++roots;
	}
	best = wave_max(best); roots = wave_sum(roots);
	if ((threadIdx.x & 63) == 0 && roots) { atomicMax(&rec[2], best); atomicAdd(&rec[4], roots); }
}
// the samples of the picked component get the plane when it is large enough; the record of the round
__global__ __launch_bounds__(kBlockSize) void cluster_assign_kernel(unsigned n0, const uint32_t* marks, const uint32_t* scan, const uint32_t* idx, const uint32_t* parent,
                                                                    unsigned long long minPoints, int32_t plane, unsigned long long* rec, int32_t* assigned) {
	const unsigned long long pick = rec[2], size = pick >> 32;
	const uint32_t label = ~(uint32_t)pick, nIn = (uint32_t)rec[3];
	const bool accepted = size >= minPoints;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		int32_t* out = (int32_t*)(rec + kClusterRecOut);
		out[0] = (int32_t)scan[n0]; out[1] = (int32_t)rec[4]; out[2] = (int32_t)size; out[3] = accepted ? 1 : 0;
	}
	if (!accepted) return;
	for (unsigned j = blockIdx.x * blockDim.x + threadIdx.x; j < nIn; j += gridDim.x * blockDim.x)
		if (parent[scan[j] + marks[j] - 1u] == label) assigned[idx[j]] = plane;
}

// ---- S5 ----
// words of a plane: 0..5 hi / lo of the x, y, z sums of round(P * 2^32); 6 count; 7 / 8 min / max pixel x; 9 / 10 min / max pixel y;
// 11 / 12 min / max u; 13 / 14 min / max v (ordered doubles)
__global__ void init_acc_kernel(unsigned long long* acc) {
	const int t = threadIdx.x + blockIdx.x * blockDim.x;
	if (t >= HCMVS_MAX_PRIOR_PLANES * kPriorAccWords) return;
	const int wd = t % kPriorAccWords;
	acc[t] = (wd == 7 || wd == 9 || wd == 11 || wd == 13) ? ~0ull : 0ull;
}
__global__ __launch_bounds__(kBlockSize) void plane_sums_kernel(unsigned n0, int w, const float* xyz, const int32_t* pix, const int32_t* assigned, unsigned long long* acc) {
	__shared__ unsigned long long sh[HCMVS_MAX_PRIOR_PLANES * kPriorAccWords];
	for (int t = threadIdx.x; t < HCMVS_MAX_PRIOR_PLANES * kPriorAccWords; t += kBlockSize) { const int wd = t % kPriorAccWords; sh[t] = (wd == 7 || wd == 9) ? ~0ull : 0ull; }
	__syncthreads();
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += gridDim.x * blockDim.x) {
		const int pl = assigned[i];
		if (pl < 0) continue;
		unsigned long long* a = sh + (size_t)pl * kPriorAccWords;
#pragma unroll
		for (int q = 0; q < 3; ++q) {
			double v = (double)xyz[3 * (size_t)i + q];
			v = v < 1073741824.0 ? (v > -1073741824.0 ? v : -1073741823.0) : 1073741823.0; // |P| saturated below 2^30
			const long long fx = (long long)rint(v * 0x1p32);
			atomicAdd(&a[2 * q], (unsigned long long)(fx >> 32));
			atomicAdd(&a[2 * q + 1], (unsigned long long)fx & 0xffffffffull);
		}
		atomicAdd(&a[6], 1ull);
		const unsigned long long x = (unsigned long long)(pix[i] % w), y = (unsigned long long)(pix[i] / w);
		atomicMin(&a[7], x); atomicMax(&a[8], x); atomicMin(&a[9], y); atomicMax(&a[10], y);
	}
	__syncthreads();
	for (int t = threadIdx.x; t < HCMVS_MAX_PRIOR_PLANES * kPriorAccWords; t += kBlockSize) {
		const int wd = t % kPriorAccWords;
		if (sh[(t / kPriorAccWords) * kPriorAccWords + 6] == 0) continue; // no sample of the plane here
		if (wd <= 6) { if (sh[t]) atomicAdd(&acc[t], sh[t]); }
		else if (wd == 7 || wd == 9) atomicMin(&acc[t], sh[t]);
		else if (wd == 8 || wd == 10) atomicMax(&acc[t], sh[t]);
	}
}
// frames: per plane centre (3), b1 (3), b2 (3) doubles
__global__ __launch_bounds__(kBlockSize) void plane_extent_kernel(unsigned n0, const float* xyz, const int32_t* assigned, const double* frames, unsigned long long* acc) {
	__shared__ unsigned long long sh[HCMVS_MAX_PRIOR_PLANES * 4];
	for (int t = threadIdx.x; t < HCMVS_MAX_PRIOR_PLANES * 4; t += kBlockSize) sh[t] = (t & 1) ? 0ull : ~0ull;
	__syncthreads();
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n0; i += gridDim.x * blockDim.x) {
		const int pl = assigned[i];
		if (pl < 0) continue;
		const double* f = frames + 9 * (size_t)pl;
		const double dx = (double)xyz[3 * (size_t)i] - f[0], dy = (double)xyz[3 * (size_t)i + 1] - f[1], dz = (double)xyz[3 * (size_t)i + 2] - f[2];
		const unsigned long long u = ordered((dx * f[3] + dy * f[4]) + dz * f[5]), v = ordered((dx * f[6] + dy * f[7]) + dz * f[8]);
		atomicMin(&sh[4 * pl], u); atomicMax(&sh[4 * pl + 1], u); atomicMin(&sh[4 * pl + 2], v); atomicMax(&sh[4 * pl + 3], v);
	}
	__syncthreads();
	for (int t = threadIdx.x; t < HCMVS_MAX_PRIOR_PLANES * 4; t += kBlockSize) {
		unsigned long long* dst = &acc[(size_t)(t / 4) * kPriorAccWords + 11 + (t & 3)];
		if (t & 1) { if (sh[t] != 0ull) atomicMax(dst, sh[t]); }
		else if (sh[t] != ~0ull) atomicMin(dst, sh[t]);
	}
}

// ---- S6 ----
__global__ __launch_bounds__(kBlockSize) void render_kernel(unsigned px, int w, Kinv kinv, const uint8_t* region, const float* depth, const PriorPlaneDev* planes, int nPlanes,
                                                            float* prior, float* priorNormal, unsigned long long* words) {
	unsigned long long written = 0;
	for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < px; i += gridDim.x * blockDim.x) {
		float out = 0.f, on[3] = {0.f, 0.f, 0.f};
		if (region[i] == 0) {
			const int x = (int)(i % (unsigned)w), y = (int)(i / (unsigned)w);
			float r[3];
			ray_of(kinv, x, y, r);
			const float d = depth[i];
			const bool has = usable_depth(d) && fabsf(r[0] * d) <= 3.402823466e+38f && fabsf(r[1] * d) <= 3.402823466e+38f; // (else: as without a depth)
			const float X[3] = {has ? r[0] * d : 0.f, has ? r[1] * d : 0.f, has ? r[2] * d : 0.f};
			int best = -1;
			double bestDist = 0.0;
			for (int pl = 0; pl < nPlanes; ++pl) { // uniform across the wave
				const PriorPlaneDev& P = planes[pl];
				int pos = 0, neg = 0;
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const double ax = P.quad[2 * e], ay = P.quad[2 * e + 1], bx = P.quad[2 * ((e + 1) & 3)], by = P.quad[2 * ((e + 1) & 3) + 1];
					const double cr = (bx - ax) * ((double)y - ay) - (by - ay) * ((double)x - ax);
					pos += cr > 0.0 ? 1 : 0; neg += cr < 0.0 ? 1 : 0;
				}
				if (pos != 4 && neg != 4) continue;
				const double dist = fabs((((double)P.n[0] * (double)X[0] + (double)P.n[1] * (double)X[1]) + (double)P.n[2] * (double)X[2]) - P.nc);
				if (best < 0 || dist < bestDist) { best = pl; bestDist = dist; }
			}
			if (best >= 0) {
				const PriorPlaneDev& P = planes[best];
				const double den = ((double)P.n[0] * (double)r[0] + (double)P.n[1] * (double)r[1]) + (double)P.n[2] * (double)r[2];
				const float v = (float)(P.nc / den);
				if (usable_depth(v)) {
					out = v;
					const float sg = den > 0.0 ? -1.f : 1.f; // towards the camera: n . ray < 0
					on[0] = sg * P.n[0]; on[1] = sg * P.n[1]; on[2] = sg * P.n[2];
				}
			}
		}
		prior[i] = out;
		if (priorNormal) { priorNormal[3 * (size_t)i] = on[0]; priorNormal[3 * (size_t)i + 1] = on[1]; priorNormal[3 * (size_t)i + 2] = on[2]; }
		written += out > 0.f ? 1 : 0;
	}
	written = wave_sum(written);
	if ((threadIdx.x & 63) == 0 && written) atomicAdd(&words[0], written);
}

inline unsigned blocks_for(size_t n, unsigned cap) { const size_t b = (n + kBlockSize - 1) / kBlockSize; return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b)); }
inline double from_ordered(unsigned long long k) {
	const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
	double v; memcpy(&v, &b, 8); return v;
}

} // namespace

int generate_plane_prior_device(int w, int h, const double K[9], const uint8_t* region, const float* depth, const float* normal, const float* conf,
                                const hcmvs_plane_prior_params& p, float* prior, float* priorNormal, hcmvs_prior_plane* planes, hcmvs_plane_prior_stats& st,
                                DevBuf& scratch, PriorGenTrace& trace, hipStream_t s, std::string& err) {
	const size_t px = (size_t)w * h;
	st = hcmvs_plane_prior_stats();
	trace = PriorGenTrace();
	if (planes) memset(planes, 0, sizeof(hcmvs_prior_plane) * HCMVS_MAX_PRIOR_PLANES);
	auto fail = [&](const char* what) { err = std::string("generate_plane_prior: ") + what; (void)hipStreamSynchronize(s); (void)hipGetLastError(); return 2; };
	auto zero_out = [&]() {
		return hipMemsetAsync(prior, 0, px * 4, s) == hipSuccess && (!priorNormal || hipMemsetAsync(priorNormal, 0, px * 12, s) == hipSuccess) &&
		       hipStreamSynchronize(s) == hipSuccess;
	};
	if (!region) return zero_out() ? 0 : fail("device failure");

	Kinv kinv;
	(void)prior_gen_kinv(K, kinv.i); // (checked by the caller)
	// the temporary storage of the scan and of the sort is asked for once, for px (+ 1) items, and serves every smaller stage: what hipcub
	// needs does not shrink with more items (the calls below get the size they may use and fail, not overrun, if that ever changes)
	size_t scanBytes = 0;
	(void)hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(px + 1));
	const PriorGenLayout lay = prior_gen_layout(px, scanBytes, knn_sort_bytes(px));
	if (scratch.reserve(lay.bytes, s) != hipSuccess) return fail("out of device memory");
	st.device_bytes = lay.bytes;
	char* b = scratch.get();
	uint32_t *flags = (uint32_t*)(b + lay.flags), *scan = (uint32_t*)(b + lay.scan);
	float *xyzA = (float*)(b + lay.xyzA), *nrmA = (float*)(b + lay.nrmA), *xyzB = (float*)(b + lay.xyzB), *nrmB = (float*)(b + lay.nrmB);
	int32_t *pixA = (int32_t*)(b + lay.pixA), *pixB = (int32_t*)(b + lay.pixB), *sampleAt = (int32_t*)(b + lay.sampleAt), *assigned = (int32_t*)(b + lay.assigned);
	double* spacing = (double*)(b + lay.spacing);
	uint8_t* stage = (uint8_t*)(b + lay.stage);
	float4* cand = (float4*)(b + lay.cand);
	uint32_t* counts = (uint32_t*)(b + lay.counts);
	int32_t* winner = (int32_t*)(b + lay.winner);
	unsigned long long *acc = (unsigned long long*)(b + lay.acc), *words = (unsigned long long*)(b + lay.words);
	PriorPlaneDev* dPlanes = (PriorPlaneDev*)(b + lay.planes);
	int32_t* dLevels = (int32_t*)(b + lay.levels);

	Event ev0, ev1;
	if (ev0.ensure() != hipSuccess || ev1.ensure() != hipSuccess) return fail("event creation failed");
	(void)hipEventRecord(ev0.get(), s);
	trace.valid = true; trace.w = w; trace.h = h; trace.lay = lay;
	const int k = p.n_neighbors;
	auto finish = [&](bool ok) {
		if (!ok) return fail("device failure");
		(void)hipEventRecord(ev1.get(), s);
		if (hipEventSynchronize(ev1.get()) != hipSuccess) return fail("device failure");
		(void)hipEventElapsedTime(&st.ms_device, ev0.get(), ev1.get());
		return 0;
	};
	// exclusive scan of the n + 1 flags; returns the total through the host
	auto scan_total = [&](size_t n, uint32_t& total) {
		size_t tmp = scanBytes;
		if (hipcub::DeviceScan::ExclusiveSum(b + lay.scanTmp, tmp, flags, scan, (int)(n + 1), s) != hipSuccess) return false;
		return hipMemcpyAsync(&total, scan + n, 4, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
	};
	auto read_words = [&](unsigned long long* out, int n) {
		return hipMemcpyAsync(out, words, 8 * (size_t)n, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
	};

	auto clock = std::chrono::steady_clock::now();
	auto lap = [&](float& ms) { // (called where the stream has just been waited for)
		const auto now = std::chrono::steady_clock::now();
		ms = std::chrono::duration<float, std::milli>(now - clock).count();
		clock = now;
	};
	// S1
	if (hipMemsetAsync(words, 0, 256, s) != hipSuccess) return fail("device failure");
	hipLaunchKernelGGL(sample_flags_kernel, dim3(blocks_for(px, 2048)), dim3(kBlockSize), 0, s, (unsigned)px, w, kinv, region, depth, conf, p.conf_max, flags, stage, words);
	uint32_t nS = 0;
	if (!scan_total(px, nS)) return fail("scan failed");
	unsigned long long hw[4];
	if (!read_words(hw, 1)) return fail("device failure");
	st.region_pixels = hw[0]; st.samples = nS;
	lap(st.ms_gather);
	if (nS < (uint32_t)k + 1) return finish(zero_out());
	hipLaunchKernelGGL(gather_samples_kernel, dim3(blocks_for(px, 2048)), dim3(kBlockSize), 0, s, (unsigned)px, w, kinv, depth, normal, flags, scan, xyzA, nrmA, pixA);

	// S2
	KnnIndex ix;
	if (const char* what = knn_build(nS, xyzA, k, b, lay.knn, s, ix)) return fail(what);
	if (k <= 16) hipLaunchKernelGGL(planarity_kernel<16>, kKnnGrid, kKnnBlock, 0, s, (unsigned long long)nS, ix.sorted, ix.keys, ix.posOf, ix.g, k, (double)p.planarity_min, flags);
	else hipLaunchKernelGGL(planarity_kernel<32>, kKnnGrid, kKnnBlock, 0, s, (unsigned long long)nS, ix.sorted, ix.keys, ix.posOf, ix.g, k, (double)p.planarity_min, flags);
	uint32_t nP = 0;
	if (!scan_total(nS, nP)) return fail("scan failed");
	st.planar_samples = nP;
	if (nP < (uint32_t)k + 1) return finish(zero_out());
	hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(nS, 2048)), dim3(kBlockSize), 0, s, nS, flags, scan, xyzA, nrmA, pixA, xyzB, nrmB, pixB, stage, (uint8_t)3);

	// S3
	auto spacing_pass = [&](uint32_t n, const float* xyz, double& avg) {
		if (hipMemsetAsync(words, 0, 256, s) != hipSuccess) return false;
		if (knn_build(n, xyz, k, b, lay.knn, s, ix)) return false;
		if (k <= 16) hipLaunchKernelGGL(spacing_kernel<16>, kKnnGrid, kKnnBlock, 0, s, (unsigned long long)n, ix.sorted, ix.keys, ix.g, k, spacing, words);
		else hipLaunchKernelGGL(spacing_kernel<32>, kKnnGrid, kKnnBlock, 0, s, (unsigned long long)n, ix.sorted, ix.keys, ix.g, k, spacing, words);
		if (!read_words(hw, 2)) return false;
		avg = prior_gen_mean((int64_t)hw[0], hw[1], n, kPriorSpacingShift);
		return true;
	};
	double avgAll = 0, avg = 0;
	if (!spacing_pass(nP, xyzB, avgAll)) return fail("spacing pass failed");
	st.avg_spacing_all = avgAll;
	hipLaunchKernelGGL(outlier_flags_kernel, dim3(blocks_for(nP, 2048)), dim3(kBlockSize), 0, s, nP, spacing, avgAll, flags);
	uint32_t n0 = 0;
	if (!scan_total(nP, n0)) return fail("scan failed");
	st.fitting_samples = n0;
	if (n0 < (uint32_t)k + 1) return finish(zero_out());
	hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(nP, 2048)), dim3(kBlockSize), 0, s, nP, flags, scan, xyzB, nrmB, pixB, xyzA, nrmA, pixA, stage, (uint8_t)4);
	if (!spacing_pass(n0, xyzA, avg)) return fail("spacing pass failed");
	st.avg_spacing = avg;
	lap(st.ms_search);
	const float eps = prior_gen_eps(avg, p.epsilon_mul);
	const int64_t minPoints = prior_gen_min_points(n0, p.min_points_div);
	st.eps = eps; st.min_points = (int32_t)(minPoints > INT32_MAX ? INT32_MAX : minPoints);

	// S4
	int32_t levels[kPriorMaxLevels] = {};
	const int nLevels = prior_gen_levels(w, h, levels);
	if (hipMemcpyAsync(dLevels, levels, sizeof levels, hipMemcpyHostToDevice, s) != hipSuccess) return fail("upload failed");
	hipLaunchKernelGGL(fill_i32_kernel, dim3(blocks_for(px, 2048)), dim3(kBlockSize), 0, s, (unsigned)px, sampleAt, -1);
	hipLaunchKernelGGL(fill_i32_kernel, dim3(blocks_for(n0, 2048)), dim3(kBlockSize), 0, s, n0, assigned, -1);
	hipLaunchKernelGGL(index_samples_kernel, dim3(blocks_for(n0, 2048)), dim3(kBlockSize), 0, s, n0, pixA, sampleAt);
	trace.n0 = n0;
	const int failLimit = prior_gen_fail_limit(p.probability, minPoints, n0, p.max_rounds);
	struct Found { float n[3]; uint32_t cnt0; };
	std::vector<Found> found;
	int64_t unassigned = n0;
	int fails = 0, rounds = 0;
	// S4c: with a usable cell the winner's inliers are clustered before anything is assigned (one more wait per round that has a winner);
	// otherwise the round is what it was, assign_kernel behind the winner without a wait in between
	const bool clustering = p.cluster_mul > 0.f;
	const float cellF = clustering ? prior_gen_cluster_cell(avg, p.cluster_mul) : 0.f;
	const bool chain = clustering && prior_gen_cluster_cell_usable(cellF);
	st.cluster_eps = cellF;
	const PriorClusterScratch cs = prior_gen_cluster_scratch(lay, px, n0, scanBytes); // (pieces that are idle during S4)
	unsigned long long *cKeys = (unsigned long long*)(b + cs.keys.off), *cKeys2 = (unsigned long long*)(b + cs.keys2.off), *cCells = (unsigned long long*)(b + cs.cells.off);
	unsigned long long* cRec = (unsigned long long*)(b + cs.rec.off);
	uint32_t *cIdx = (uint32_t*)(b + cs.idx.off), *cIdx2 = (uint32_t*)(b + cs.idx2.off), *cStart = (uint32_t*)(b + cs.start.off);
	uint32_t *cParent = (uint32_t*)(b + cs.parent.off), *cSizes = (uint32_t*)(b + cs.sizes.off), *cMarks = (uint32_t*)(b + cs.marks.off), *cScan = (uint32_t*)(b + cs.scan.off);
	auto cluster_round = [&](const float n[3], int32_t plane, int32_t row[4]) {
		ClusterFrame fr;
		prior_gen_frame(n, fr.b1, fr.b2);
		fr.cell = (double)cellF;
		const dim3 grid(blocks_for(n0, 2048)), block(kBlockSize);
		hipLaunchKernelGGL(cluster_reset_kernel, dim3(1), dim3(64), 0, s, cRec);
		hipLaunchKernelGGL(cluster_origin_kernel, grid, block, 0, s, n0, xyzA, nrmA, assigned, winner, p.normal_threshold, eps, fr, cRec);
		hipLaunchKernelGGL(cluster_keys_kernel, grid, block, 0, s, n0, xyzA, nrmA, assigned, winner, p.normal_threshold, eps, fr, cRec, cKeys, cIdx);
		size_t sortBytes = cs.sortTmp.bytes, tmp = cs.scanTmp.bytes;
		if (hipcub::DeviceRadixSort::SortPairs(b + cs.sortTmp.off, sortBytes, cKeys, cKeys2, cIdx, cIdx2, (int)n0, 0, 64, s) != hipSuccess) return false;
		hipLaunchKernelGGL(cluster_marks_kernel, grid, block, 0, s, n0, cKeys2, cMarks, cRec);
		if (hipcub::DeviceScan::ExclusiveSum(b + cs.scanTmp.off, tmp, cMarks, cScan, (int)(n0 + 1), s) != hipSuccess) return false;
		hipLaunchKernelGGL(cluster_cells_kernel, grid, block, 0, s, n0, cKeys2, cMarks, cScan, cCells, cStart, cParent, cSizes);
		hipLaunchKernelGGL(cluster_union_kernel, grid, block, 0, s, n0, cScan, cCells, cParent);
		hipLaunchKernelGGL(cluster_sizes_kernel, grid, block, 0, s, n0, cScan, cStart, cRec, cParent, cSizes);
		hipLaunchKernelGGL(cluster_pick_kernel, grid, block, 0, s, n0, cScan, cParent, cSizes, cRec);
		hipLaunchKernelGGL(cluster_assign_kernel, grid, block, 0, s, n0, cMarks, cScan, cIdx2, cParent, (unsigned long long)minPoints, plane, cRec, assigned);
		if (hipGetLastError() != hipSuccess) return false;
		return hipMemcpyAsync(row, cRec + kClusterRecOut, 16, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
	};
	// S4r: with refit_iters > 0 the winner is refitted before S4c and before anything is assigned: at most refit_iters + 1 launches of the
	// refit kernel and as many waits per round that has a winner, then the final plane goes into the winner record and the round ends as it
	// does without (assign_kernel, or the chain of S4c).  With refit_iters = 0 nothing of this is launched
	const int refitIters = p.refit_iters;
	const int refitE = prior_gen_refit_scale(eps);
	unsigned long long* rRec = (unsigned long long*)(b + prior_gen_refit_scratch(lay).rec.off);
	std::vector<float> finalPlanes; // what the winner record is overwritten from: alive until the stream has been waited for
	if (refitIters > 0) finalPlanes.resize((size_t)4 * p.max_rounds);
	auto refit_round = [&](int round, const int32_t hwin[12], PriorRefit& rf) {
		float wp[4];
		memcpy(wp, hwin + 8, 16);
		const unsigned anchor = (unsigned)draw_below(mix64((unsigned long long)p.seed ^ mix64((unsigned long long)round * kPriorCandidates + (unsigned long long)hwin[0])), 0, n0);
		const double none[3] = {0, 0, 0}; // (the anchor's position comes back with every record, the first included)
		rf = prior_refit_begin(refitIters, minPoints, none, refitE, wp, hwin + 1);
		const double inv = std::ldexp(1.0, -refitE);
		unsigned long long rec[kPriorRefitWords];
		for (;;) {
			hipLaunchKernelGGL(refit_reset_kernel, dim3(1), dim3(64), 0, s, rRec);
			hipLaunchKernelGGL(refit_moments_kernel, dim3(blocks_for(n0, kScoreMaxBlocks)), dim3(kBlockSize), 0, s, n0, xyzA, nrmA, assigned,
			                   make_float4(rf.launch[0], rf.launch[1], rf.launch[2], rf.launch[3]), p.normal_threshold, eps, anchor, inv, rRec);
			if (hipGetLastError() != hipSuccess) return false;
			if (hipMemcpyAsync(rec, rRec, sizeof rec, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return false;
			const uint32_t ob[3] = {(uint32_t)rec[22], (uint32_t)(rec[22] >> 32), (uint32_t)rec[23]};
			for (int q = 0; q < 3; ++q) { float v; memcpy(&v, &ob[q], 4); rf.O[q] = (double)v; }
			if (!prior_refit_step(rf, rec)) break;
		}
		if (rf.kept > 0) { // the record holds the candidate's plane: the rest of the round reads the final one
			float* fp = finalPlanes.data() + 4 * (size_t)round;
			memcpy(fp, rf.plane, 16);
			if (hipMemcpyAsync((float*)winner + 8, fp, 16, hipMemcpyHostToDevice, s) != hipSuccess) return false;
		}
		return true;
	};
	const bool deferred = chain || refitIters > 0; // the round's winner is waited for before anything is assigned
	while (unassigned >= minPoints && (int)found.size() < HCMVS_MAX_PRIOR_PLANES && rounds < p.max_rounds && fails < failLimit) {
		hipLaunchKernelGGL(candidate_kernel, dim3(1), dim3(kPriorCandidates), 0, s, (unsigned)rounds, (unsigned long long)p.seed, n0, w, h, dLevels, nLevels, xyzA, nrmA, pixA,
		                   sampleAt, assigned, p.normal_threshold, cand, counts);
		hipLaunchKernelGGL(score_kernel, dim3(blocks_for(n0, kScoreMaxBlocks)), dim3(kBlockSize), 0, s, n0, xyzA, nrmA, assigned, cand, p.normal_threshold, eps, counts);
		hipLaunchKernelGGL(winner_kernel, dim3(1), dim3(kPriorCandidates), 0, s, cand, counts, (unsigned long long)minPoints, winner);
		if (!deferred) hipLaunchKernelGGL(assign_kernel, dim3(blocks_for(n0, 2048)), dim3(kBlockSize), 0, s, n0, xyzA, nrmA, winner, p.normal_threshold, eps, (int32_t)found.size(), assigned);
		int32_t hwin[12];
		if (hipMemcpyAsync(hwin, winner, sizeof hwin, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("a round failed");
		for (int q = 0; q < 6; ++q) trace.rounds.push_back(hwin[q]);
		st.candidates_valid += (uint64_t)hwin[5];
		const int round = rounds++;
		int32_t row[4] = {0, 0, 0, 0}; // occupied cells, components, the largest size, accepted
		int32_t rrow[6] = {0, 0, 0, 0, 0, 0}; // S4r: steps solved, steps kept, the final plane's counts
		float fin[4] = {0.f, 0.f, 0.f, 0.f};  // the round's final plane
		if (hwin[0] >= 0) {
			memcpy(fin, hwin + 8, 16);
			for (int q = 0; q < 4; ++q) rrow[2 + q] = hwin[1 + q];
			if (refitIters > 0) {
				PriorRefit rf;
				if (!refit_round(round, hwin, rf)) return fail("refitting a round's winner failed");
				memcpy(fin, rf.plane, 16);
				rrow[0] = rf.solved; rrow[1] = rf.kept;
				for (int q = 0; q < 4; ++q) rrow[2 + q] = (int32_t)rf.cnt[q];
				if (rf.kept > 0) { ++trace.refitStats.refit_rounds; trace.refitStats.refit_steps += rf.kept; }
			}
			row[1] = clustering ? 1 : 0; row[2] = rrow[2]; row[3] = 1; // unclustered: all inliers are the plane
			if (chain) { if (!cluster_round(fin, (int32_t)found.size(), row)) return fail("clustering a round's winner failed"); }
			else if (deferred) hipLaunchKernelGGL(assign_kernel, dim3(blocks_for(n0, 2048)), dim3(kBlockSize), 0, s, n0, xyzA, nrmA, winner, p.normal_threshold, eps, (int32_t)found.size(), assigned);
		}
		for (int q = 0; q < 4; ++q) trace.clusters.push_back(row[q]);
		for (int q = 0; q < 6; ++q) trace.refits.push_back(rrow[q]);
		for (int q = 0; q < 4; ++q) trace.refitPlanes.push_back(fin[q]);
		if (row[3]) {
			Found f;
			memcpy(f.n, fin, 12);
			f.cnt0 = (uint32_t)row[2];
			found.push_back(f);
			unassigned -= row[2];
			st.cluster_left += (uint64_t)(rrow[2] - row[2]);
			fails = 0;
		} else {
			if (hwin[0] >= 0) ++st.cluster_rejects;
			++fails;
		}
	}
	st.rounds = rounds; st.planes = (int32_t)found.size();
	lap(st.ms_rounds);
	if (found.empty()) return finish(zero_out());

	// S5
	const int nPl = (int)found.size();
	std::vector<unsigned long long> hacc((size_t)HCMVS_MAX_PRIOR_PLANES * kPriorAccWords);
	hipLaunchKernelGGL(init_acc_kernel, dim3((HCMVS_MAX_PRIOR_PLANES * kPriorAccWords + kBlockSize - 1) / kBlockSize), dim3(kBlockSize), 0, s, acc);
	hipLaunchKernelGGL(plane_sums_kernel, dim3(blocks_for(n0, 1024)), dim3(kBlockSize), 0, s, n0, w, xyzA, pixA, assigned, acc);
	if (hipMemcpyAsync(hacc.data(), acc, hacc.size() * 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("plane sums failed");
	std::vector<double> frames((size_t)HCMVS_MAX_PRIOR_PLANES * 9, 0.0);
	for (int i = 0; i < nPl; ++i) {
		const unsigned long long* a = hacc.data() + (size_t)i * kPriorAccWords;
		double* f = frames.data() + 9 * (size_t)i;
		for (int q = 0; q < 3; ++q) f[q] = prior_gen_mean((int64_t)a[2 * q], a[2 * q + 1], a[6], kPriorCoordShift);
		prior_gen_frame(found[i].n, f + 3, f + 6);
	}
	double* dFrames = (double*)(b + lay.spacing); // (the spacings have served)
	if (hipMemcpyAsync(dFrames, frames.data(), frames.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess) return fail("upload failed");
	hipLaunchKernelGGL(plane_extent_kernel, dim3(blocks_for(n0, 1024)), dim3(kBlockSize), 0, s, n0, xyzA, assigned, dFrames, acc);
	if (hipMemcpyAsync(hacc.data(), acc, hacc.size() * 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail("plane extents failed");
	std::vector<PriorPlaneDev> hp((size_t)HCMVS_MAX_PRIOR_PLANES);
	memset(hp.data(), 0, hp.size() * sizeof(PriorPlaneDev));
	for (int i = 0; i < nPl; ++i) {
		const unsigned long long* a = hacc.data() + (size_t)i * kPriorAccWords;
		const double* f = frames.data() + 9 * (size_t)i;
		const double uv[4] = {from_ordered(a[11]), from_ordered(a[12]), from_ordered(a[13]), from_ordered(a[14])};
		const int32_t box[4] = {(int32_t)a[7], (int32_t)a[8], (int32_t)a[9], (int32_t)a[10]};
		PriorPlaneDev& d = hp[(size_t)i];
		const int fb = prior_gen_quad(K, f, f + 3, f + 6, uv, box, d.quad);
		for (int q = 0; q < 3; ++q) d.n[q] = found[i].n[q];
		d.nc = ((double)d.n[0] * f[0] + (double)d.n[1] * f[1]) + (double)d.n[2] * f[2];
		if (planes) {
			hcmvs_prior_plane& o = planes[i];
			for (int q = 0; q < 3; ++q) { o.normal[q] = d.n[q]; o.centre[q] = f[q]; }
			for (int q = 0; q < 8; ++q) o.quad[q] = d.quad[q];
			o.n_inliers = found[i].cnt0; o.box_fallback = fb;
		}
	}
	if (hipMemcpyAsync(dPlanes, hp.data(), hp.size() * sizeof(PriorPlaneDev), hipMemcpyHostToDevice, s) != hipSuccess) return fail("upload failed");

	// S6
	if (hipMemsetAsync(words, 0, 256, s) != hipSuccess) return fail("device failure");
	hipLaunchKernelGGL(render_kernel, dim3(blocks_for(px, 4096)), dim3(kBlockSize), 0, s, (unsigned)px, w, kinv, region, depth, dPlanes, nPl, prior, priorNormal, words);
	if (hipGetLastError() != hipSuccess) return fail("launch failed");
	if (!read_words(hw, 1)) return fail("render failed"); // (hp, frames and levels have left: the stream is idle)
	st.prior_pixels = hw[0];
	lap(st.ms_render);
	return finish(true);
}

} // namespace hcmvs

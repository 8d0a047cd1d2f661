/* hc-mvs_amd/csrc/prior_gen_plan.h -- the host half of hcmvs_generate_plane_prior_device: what the call
 * refuses before any work, the inverse of K, the level table, min_points and the stop rule of the plane detection, the decoding of the
 * fixed-point sums, the frame and image quad of a plane from its reduced values (tiny, double precision), the scratch layout, and the
 * least-squares refit of a round's winner (S4r): its scale, its solver and its decision sequence.
 * Plain C++ (no HIP); every product is rounded on its own (built with -ffp-contract=off, as the library is). */
#ifndef HCMVS_PRIOR_GEN_PLAN_H
#define HCMVS_PRIOR_GEN_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include "../../include/hcmvs_hip.h"
#include "carve.h"
#include "knn_layout.h"
namespace hcmvs {

constexpr int kPriorCandidates = 256;   // M: candidates of a round
constexpr int kPriorMaxLevels = 16;
constexpr int kPriorMaxRounds = 4096;
constexpr int kPriorSpacingShift = 40;  // a spacing is summed as round(s * 2^40), s saturated below 2^23
constexpr int kPriorCoordShift = 32;    // a coordinate is summed as round(P * 2^32), |P| saturated below 2^30
constexpr int kPriorAccWords = 16;      // unsigned long long words a plane reduces into (prior_kernels.hip)
constexpr uint32_t kPriorClusterCellCap = 1u << 30; // S4c: a cell coordinate is min(floor((u - u0) / cell), this); the cells at the cap merge (degenerate)
constexpr int kPriorMaxRefitIters = 16; // S4r: refit_iters at the most
constexpr int kPriorRefitFirstShift = 24;  // S4r: a first moment is summed as rint(s * 2^24), s = (P - O) / 2^E saturated inside (-2^20, 2^20)
constexpr int kPriorRefitSecondShift = 20; // S4r: a second moment is summed as rint((s_a * s_b) * 2^20)
constexpr int kPriorRefitWords = 24;       // unsigned long long words of the refit record: 0..3 cnt_0 .. cnt_3, 4..21 hi / lo of the nine sums (x y z xx xy xz yy yz zz)

struct PriorGenArgs {
	uintptr_t depth, normal, conf, prior, priorNormal; // device addresses as integers (the checks do not read them); priorNormal may be 0
	int32_t w, h;
	const double* K;
	const hcmvs_plane_prior_params* p;
};

// Kinv of a K whose last row is 0 0 1, in double: i = {i00 i01 i02 i10 i11 i12}, the last row stays 0 0 1.  False: such a K is not supported
inline bool prior_gen_kinv(const double K[9], double i[6]) {
	if (!K || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0) return false;
	const double det = K[0] * K[4] - K[1] * K[3];
	if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
	i[0] = K[4] / det; i[1] = -K[1] / det; i[3] = -K[3] / det; i[4] = K[0] / det;
	i[2] = -(i[0] * K[2] + i[1] * K[5]);
	i[5] = -(i[3] * K[2] + i[4] * K[5]);
	for (int q = 0; q < 6; ++q) if (!std::isfinite(i[q])) return false;
	return true;
}
// ray(x, y) = Kinv (x, y, 1), each component rounded to float32; the association the kernels use as well
inline void prior_gen_ray(const double i[6], int x, int y, float r[3]) {
	r[0] = (float)((i[0] * (double)x + i[1] * (double)y) + i[2]);
	r[1] = (float)((i[3] * (double)x + i[4] * (double)y) + i[5]);
	r[2] = 1.f;
}

inline bool prior_gen_overlap(uintptr_t a, uint64_t aBytes, uintptr_t b, uint64_t bBytes) { return a < b + bBytes && b < a + aBytes; }

// Empty string: the call may run.  Otherwise the reason it is refused (nothing has reached the device).
inline std::string prior_gen_check(const PriorGenArgs& a) {
	char buf[200];
	if (!a.depth || !a.normal || !a.conf || !a.prior || !a.p || !a.K) return "null pointer";
	if (a.w < 1 || a.h < 1 || (int64_t)a.w * a.h >= ((int64_t)1 << 29)) { snprintf(buf, sizeof buf, "unusable size %dx%d", a.w, a.h); return buf; }
	double inv[6];
	if (!prior_gen_kinv(a.K, inv)) return "unsupported K (last row not 0 0 1, or not invertible)";
	const hcmvs_plane_prior_params& p = *a.p;
	if (!(p.probability > 0.f && p.probability < 1.f)) { snprintf(buf, sizeof buf, "probability %g is not inside (0, 1)", (double)p.probability); return buf; }
	if (!(p.min_points_div > 0.f) || !std::isfinite(p.min_points_div)) { snprintf(buf, sizeof buf, "min_points_div %g is not a finite number > 0", (double)p.min_points_div); return buf; }
	if (!(p.epsilon_mul > 0.f) || !std::isfinite(p.epsilon_mul)) { snprintf(buf, sizeof buf, "epsilon_mul %g is not a finite number > 0", (double)p.epsilon_mul); return buf; }
	if (p.n_neighbors < 3 || p.n_neighbors > 31) { snprintf(buf, sizeof buf, "n_neighbors %d outside 3..31", p.n_neighbors); return buf; }
	if (p.max_rounds < 1 || p.max_rounds > kPriorMaxRounds) { snprintf(buf, sizeof buf, "max_rounds %d outside 1..%d", p.max_rounds, kPriorMaxRounds); return buf; }
	if (p.conf_max != p.conf_max || p.planarity_min != p.planarity_min || p.normal_threshold != p.normal_threshold) return "a threshold is NaN";
	if (!(p.cluster_mul >= 0.f) || !std::isfinite(p.cluster_mul)) { snprintf(buf, sizeof buf, "cluster_mul %g is not a finite number >= 0", (double)p.cluster_mul); return buf; }
	if (p.refit_iters < 0 || p.refit_iters > kPriorMaxRefitIters) { snprintf(buf, sizeof buf, "refit_iters %d outside 0..%d", p.refit_iters, kPriorMaxRefitIters); return buf; }
	const uint64_t px = (uint64_t)a.w * a.h;
	const struct { uintptr_t at; uint64_t bytes; const char* what; } in[3] = {{a.depth, px * 4, "depth"}, {a.normal, px * 12, "normal"}, {a.conf, px * 4, "conf"}};
	for (const auto& m : in) {
		if (prior_gen_overlap(a.prior, px * 4, m.at, m.bytes)) { snprintf(buf, sizeof buf, "the prior map overlaps the %s map", m.what); return buf; }
		if (a.priorNormal && prior_gen_overlap(a.priorNormal, px * 12, m.at, m.bytes)) { snprintf(buf, sizeof buf, "the prior normal map overlaps the %s map", m.what); return buf; }
	}
	if (a.priorNormal && prior_gen_overlap(a.priorNormal, px * 12, a.prior, px * 4)) return "the prior normal map overlaps the prior map";
	return std::string();
}

// the levels a candidate draws its two offsets at: 2, 4, 8, ... up to max(w, h) / 2 (at least the level 2)
inline int prior_gen_levels(int w, int h, int32_t levels[kPriorMaxLevels]) {
	const int top = (w > h ? w : h) / 2;
	int n = 0;
	for (int l = 2; l <= top && n < kPriorMaxLevels; l *= 2) levels[n++] = l;
	if (n == 0) levels[n++] = 2;
	return n;
}
inline int64_t prior_gen_min_points(uint64_t n0, float minPointsDiv) {
	const double v = std::floor((double)n0 / (double)minPointsDiv);
	const int64_t m = v >= 9e18 ? INT64_MAX : (int64_t)v;
	return m < 3 ? 3 : m;
}
// the consecutive failed rounds that end the detection: ceil(ceil(ln(probability) / ln(1 - min_points / n0)) / M), within 1 .. maxRounds
inline int prior_gen_fail_limit(float probability, int64_t minPoints, uint64_t n0, int maxRounds) {
	const double share = (double)minPoints / (double)n0;
	double cands = 1.0;
	if (share < 1.0) cands = std::ceil(std::log((double)probability) / std::log(1.0 - share));
	double rounds = std::ceil(cands / (double)kPriorCandidates);
	if (!(rounds >= 1.0)) rounds = 1.0;
	if (rounds > (double)maxRounds) rounds = (double)maxRounds;
	return (int)rounds;
}
inline float prior_gen_eps(double avg, float epsilonMul) { return (float)(avg * (double)epsilonMul); }
// S4c: the cell edge of the clustering, rounded to float32 as eps is.  A cell that is not a finite number > 0 (the product underflowed, or
// overflowed) clusters nothing: all inliers of a winner are one component
inline float prior_gen_cluster_cell(double avg, float clusterMul) { return (float)(avg * (double)clusterMul); }
inline bool prior_gen_cluster_cell_usable(float cell) { return cell > 0.f && std::isfinite(cell); }

// a fixed-point sum that came back as two words: sum of the (signed) high parts q >> 32 and of the low parts q & 0xffffffff of the
// addends q = round(v * 2^shift).  The mean of the n values: (double)(hi * 2^32 + lo) / ((double)n * 2^shift), the integer exact
inline double prior_gen_mean(int64_t hi, uint64_t lo, uint64_t n, int shift) {
	const __int128 t = (__int128)hi * ((__int128)1 << 32) + (__int128)lo;
	return (double)t / ((double)n * std::ldexp(1.0, shift));
}

// the frame of a plane (S5): b1 = normalise(n x e_k), e_k the axis where |n_k| is smallest (lowest k on ties), b2 = n x b1, in double
inline void prior_gen_frame(const float nf[3], double b1[3], double b2[3]) {
	const double n[3] = {(double)nf[0], (double)nf[1], (double)nf[2]};
	int k = 0;
	if (std::fabs(n[1]) < std::fabs(n[k])) k = 1;
	if (std::fabs(n[2]) < std::fabs(n[k])) k = 2;
	double a[3];
	if (k == 0) { a[0] = 0.0; a[1] = n[2]; a[2] = -n[1]; }
	else if (k == 1) { a[0] = -n[2]; a[1] = 0.0; a[2] = n[0]; }
	else { a[0] = n[1]; a[1] = -n[0]; a[2] = 0.0; }
	const double len = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
	for (int q = 0; q < 3; ++q) b1[q] = a[q] / len;
	b2[0] = n[1] * b1[2] - n[2] * b1[1];
	b2[1] = n[2] * b1[0] - n[0] * b1[2];
	b2[2] = n[0] * b1[1] - n[1] * b1[0];
}
// the image quad of a plane (S5) from the extent uv = {umin, umax, vmin, vmax} of its inliers in the frame and box = {xmin, xmax, ymin,
// ymax} of their pixels: the corners (umin vmin) (umax vmin) (umax vmax) (umin vmax) projected with K; when one has z <= 0 (or does
// not project to finite numbers) the pixel box widened by half a pixel instead.  Returns the fall-back flag
inline int prior_gen_quad(const double K[9], const double c[3], const double b1[3], const double b2[3], const double uv[4], const int32_t box[4], double quad[8]) {
	const double us[4] = {uv[0], uv[1], uv[1], uv[0]}, vs[4] = {uv[2], uv[2], uv[3], uv[3]};
	bool ok = true;
	for (int i = 0; i < 4; ++i) {
		double X[3];
		for (int q = 0; q < 3; ++q) X[q] = (c[q] + us[i] * b1[q]) + vs[i] * b2[q];
		if (!(X[2] > 0.0)) { ok = false; break; }
		quad[2 * i] = ((K[0] * X[0] + K[1] * X[1]) + K[2] * X[2]) / X[2];
		quad[2 * i + 1] = ((K[3] * X[0] + K[4] * X[1]) + K[5] * X[2]) / X[2];
		if (!std::isfinite(quad[2 * i]) || !std::isfinite(quad[2 * i + 1])) { ok = false; break; }
	}
	if (ok) return 0;
	const double x0 = (double)box[0] - 0.5, x1 = (double)box[1] + 0.5, y0 = (double)box[2] - 0.5, y1 = (double)box[3] + 0.5;
	quad[0] = x0; quad[1] = y0; quad[2] = x1; quad[3] = y0; quad[4] = x1; quad[5] = y1; quad[6] = x0; quad[7] = y1;
	return 1;
}

// a plane as the render kernel reads it
struct PriorPlaneDev {
	double quad[8];
	double nc;      // n . centre: (n0 c0 + n1 c1) + n2 c2 in double
	float n[3];
	int32_t pad;
};

// The one device buffer of a call.  px = w * h bounds every stage (a stage never has more samples than pixels); the two sets A and B
// take the stages in turn (samples -> A, planar -> B, fitting set -> A).  The clustering of S4c adds no piece: it borrows pieces that are
// idle during S4 (prior_gen_cluster_scratch below)
struct PriorGenLayout {
	size_t flags = 0, scan = 0, scanTmp = 0;             // uint32 per pixel / sample: keep flags, their exclusive scan, the scan's temporary
	size_t xyzA = 0, nrmA = 0, pixA = 0, xyzB = 0, nrmB = 0, pixB = 0; // float3, float3, int32 per sample
	size_t spacing = 0;                                   // double per sample
	size_t sampleAt = 0, assigned = 0;                    // int32 per pixel, int32 per sample
	size_t stage = 0;                                     // uint8 per pixel
	size_t cand = 0, counts = 0, winner = 0, acc = 0, planes = 0, words = 0, levels = 0;
	KnnLayout knn;
	size_t bytes = 0;
};
inline PriorGenLayout prior_gen_layout(size_t px, size_t scanBytes, size_t sortBytes) {
	Carve cv;
	PriorGenLayout l;
	l.flags = cv((px + 1) * 4); l.scan = cv((px + 1) * 4); l.scanTmp = cv(scanBytes);
	l.xyzA = cv(px * 12); l.nrmA = cv(px * 12); l.pixA = cv(px * 4);
	l.xyzB = cv(px * 12); l.nrmB = cv(px * 12); l.pixB = cv(px * 4);
	l.spacing = cv(px * 8 > (size_t)HCMVS_MAX_PRIOR_PLANES * 72 ? px * 8 : (size_t)HCMVS_MAX_PRIOR_PLANES * 72); // (later: the planes' frames, 9 doubles each)
	l.sampleAt = cv(px * 4); l.assigned = cv(px * 4);
	l.stage = cv(px);
	l.cand = cv((size_t)kPriorCandidates * 16);          // float4: n, d (d = NaN: invalid)
	l.counts = cv((size_t)kPriorCandidates * 4 * 4);     // uint32 cnt_0 .. cnt_3 per candidate
	l.winner = cv(64);
	l.acc = cv((size_t)HCMVS_MAX_PRIOR_PLANES * kPriorAccWords * 8);
	l.planes = cv((size_t)HCMVS_MAX_PRIOR_PLANES * sizeof(PriorPlaneDev));
	l.words = cv(256);
	l.levels = cv((size_t)kPriorMaxLevels * 4);
	l.knn = knn_layout(cv, px, sortBytes);
	l.bytes = cv.size;
	return l;
}

// The pieces S4 needs as they are, from its first round to the trace that is read after the call: the fitting set, the two maps of the
// samples, the round's candidates and winner, and `stage` (written by S1 .. S3, read by the trace).  `acc` and `planes` are not among them:
// S5 initialises both before it reads them.  Whatever S4c borrows must stay clear of these
constexpr size_t PriorGenLayout::*kPriorLiveInS4[] = {&PriorGenLayout::xyzA, &PriorGenLayout::nrmA, &PriorGenLayout::pixA, &PriorGenLayout::sampleAt, &PriorGenLayout::assigned,
                                                      &PriorGenLayout::stage, &PriorGenLayout::cand, &PriorGenLayout::counts, &PriorGenLayout::winner, &PriorGenLayout::levels};

// The arrays of S4c inside the layout: where each starts and the bytes it needs for the n0 <= px samples of the fitting set.  keys / idx are
// sorted into keys2 / idx2; cells, parent and sizes (one entry per distinct cell, at most n0) share knn.sorted, whose 16 bytes per pixel
// they fill exactly; start borrows knn.pos; marks, scan and scanTmp are the layout's flags, scan and scanTmp doing what they do in S1 .. S3
// (n0 + 1 words: the scan's total is read at n0); sortTmp is knn.sort; rec, the 16 words of the round's record, is `words`
struct PriorScratchPiece { size_t off = 0, bytes = 0; };
struct PriorClusterScratch { PriorScratchPiece keys, keys2, idx, idx2, cells, start, parent, sizes, marks, scan, scanTmp, sortTmp, rec; };
inline PriorClusterScratch prior_gen_cluster_scratch(const PriorGenLayout& l, size_t px, size_t n0, size_t scanBytes) {
	PriorClusterScratch c;
	c.keys = {l.knn.keys, n0 * 8}; c.keys2 = {l.knn.keys2, n0 * 8}; c.idx = {l.knn.idx, n0 * 4}; c.idx2 = {l.knn.idx2, n0 * 4};
	c.cells = {l.knn.sorted, n0 * 8}; c.parent = {l.knn.sorted + px * 8, n0 * 4}; c.sizes = {l.knn.sorted + px * 12, n0 * 4};
	c.start = {l.knn.pos, n0 * 4};
	c.marks = {l.flags, (n0 + 1) * 4}; c.scan = {l.scan, (n0 + 1) * 4}; c.scanTmp = {l.scanTmp, scanBytes};
	c.sortTmp = {l.knn.sort, l.knn.sortBytes};
	c.rec = {l.words, 16 * 8};
	return c;
}

// ---- S4r: the least-squares refit of a round's winner ----
// The record of a refit launch lives in `acc`, which is idle during S4 (S5 initialises it before it reads it) and is none of the pieces
// S4c borrows
struct PriorRefitScratch { PriorScratchPiece rec; };
inline PriorRefitScratch prior_gen_refit_scratch(const PriorGenLayout& l) {
	PriorRefitScratch r;
	r.rec = {l.acc, (size_t)kPriorRefitWords * 8};
	return r;
}
// E of eps = f * 2^E, f in [0.5, 1); 0 for an eps that is not a finite number > 0
inline int prior_gen_refit_scale(float eps) {
	if (!(eps > 0.f) || !std::isfinite(eps)) return 0;
	int e = 0;
	(void)std::frexp((double)eps, &e);
	return e;
}
// The eigenvector of the smallest eigenvalue of the symmetric C = (c00 c01 c02 c11 c12 c22): cyclic Jacobi over the pairs (0,1) (0,2) (1,2),
// a pair whose off-diagonal is exactly 0 skipped, at most 16 sweeps, ending when all three off-diagonals are 0; the smallest diagonal
// entry wins, the lowest index on ties.  Every operation is rounded on its own, in the order written.  Returns the sweeps used
inline int prior_gen_refit_eigvec(const double C[6], double vec[3]) {
	double a[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
	double v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
	static const int pairs[3][2] = {{0, 1}, {0, 2}, {1, 2}};
	int sweeps = 0;
	while (sweeps < 16 && !(a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0)) {
		++sweeps;
		for (const auto& pq : pairs) {
			const int p = pq[0], q = pq[1], r = 3 - p - q;
			const double apq = a[p][q];
			if (apq == 0.0) continue;
			const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
			const double t = std::copysign(1.0, theta) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
			const double c = 1.0 / std::sqrt(t * t + 1.0);
			const double s = t * c;
			a[p][p] = a[p][p] - t * apq;
			a[q][q] = a[q][q] + t * apq;
			a[p][q] = a[q][p] = 0.0;
			const double arp = a[r][p], arq = a[r][q];
			a[r][p] = a[p][r] = c * arp - s * arq;
			a[r][q] = a[q][r] = s * arp + c * arq;
			for (int k = 0; k < 3; ++k) {
				const double vkp = v[k][p], vkq = v[k][q];
				v[k][p] = c * vkp - s * vkq;
				v[k][q] = s * vkp + c * vkq;
			}
		}
	}
	int k = 0;
	if (a[1][1] < a[k][k]) k = 1;
	if (a[2][2] < a[k][k]) k = 2;
	for (int q = 0; q < 3; ++q) vec[q] = v[q][k];
	return sweeps;
}
// mu (3) and C (6: 00 01 02 11 12 22) of the m band samples from the nine sums as they come back: words[2 i] / words[2 i + 1] the high /
// low parts of sum i (x y z xx xy xz yy yz zz)
inline void prior_gen_refit_cov(const unsigned long long words[18], uint64_t m, double mu[3], double C[6]) {
	static const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {0, 1, 2, 1, 2, 2};
	for (int q = 0; q < 3; ++q) mu[q] = prior_gen_mean((int64_t)words[2 * q], words[2 * q + 1], m, kPriorRefitFirstShift);
	for (int i = 0; i < 6; ++i) C[i] = prior_gen_mean((int64_t)words[6 + 2 * i], words[7 + 2 * i], m, kPriorRefitSecondShift) - mu[pa[i]] * mu[pb[i]];
}
// Step 4: the plane (n, d) of the m band samples about the anchor O at the scale E, its normal on the side of prev's.  False: the length
// is zero or not finite, or d is not finite
inline bool prior_gen_refit_solve(const unsigned long long words[18], uint64_t m, const double O[3], int E, const float prev[4], float out[4]) {
	double mu[3], C[6], vec[3];
	prior_gen_refit_cov(words, m, mu, C);
	(void)prior_gen_refit_eigvec(C, vec);
	float x = (float)vec[0], y = (float)vec[1], z = (float)vec[2];
	const float len = std::sqrt((x * x + y * y) + z * z);
	if (!(len > 0.f) || !std::isfinite(len)) return false;
	x = x / len; y = y / len; z = z / len;
	if ((x * prev[0] + y * prev[1]) + z * prev[2] < 0.f) { x = -x; y = -y; z = -z; }
	double c[3];
	for (int q = 0; q < 3; ++q) c[q] = O[q] + std::ldexp(mu[q], E);
	const float d = (float)(((double)x * c[0] + (double)y * c[1]) + (double)z * c[2]);
	if (!std::isfinite(d)) return false;
	out[0] = x; out[1] = y; out[2] = z; out[3] = d;
	return true;
}

// The decision sequence of S4r for one round.  The host loop launches the refit kernel for `launch` (at first the winner's plane), reads its
// record -- the four counts of that plane over the free samples and the nine sums of its e2 band -- and hands it to prior_refit_step, which
// says whether `launch` now holds a plane to count: R + 1 launches at the most.  Afterwards plane / cnt are the last kept step's (the
// winner's when none was kept)
enum PriorRefitStop { kRefitGoesOn = -1, kRefitIters = 0, kRefitBand = 1, kRefitDegenerate = 2, kRefitFixed = 3, kRefitCount = 4 };
struct PriorRefit {
	int R = 0, E = 0;
	int64_t minPoints = 0;
	double O[3] = {0, 0, 0};
	float plane[4] = {0, 0, 0, 0}, launch[4] = {0, 0, 0, 0};
	uint32_t cnt[4] = {0, 0, 0, 0};
	int solved = 0, kept = 0;
	bool trial = false; // `launch` is a step's plane that waits for its counts
	int stop = kRefitGoesOn;
};
inline PriorRefit prior_refit_begin(int R, int64_t minPoints, const double O[3], int E, const float winner[4], const int32_t counts[4]) {
	PriorRefit r;
	r.R = R; r.E = E; r.minPoints = minPoints;
	for (int q = 0; q < 3; ++q) r.O[q] = O[q];
	for (int q = 0; q < 4; ++q) { r.plane[q] = r.launch[q] = winner[q]; r.cnt[q] = (uint32_t)counts[q]; }
	return r;
}
// rec: the kPriorRefitWords words of the launch for r.launch.  True: r.launch holds the next plane to launch for
inline bool prior_refit_step(PriorRefit& r, const unsigned long long* rec) {
	if (r.trial) { // step 6
		if ((int64_t)rec[0] < r.minPoints) { r.stop = kRefitCount; return false; }
		for (int q = 0; q < 4; ++q) { r.plane[q] = r.launch[q]; r.cnt[q] = (uint32_t)rec[q]; }
		++r.kept;
		r.trial = false;
	}
	if (r.solved >= r.R) { r.stop = kRefitIters; return false; }
	const uint64_t m = rec[2]; // step 1: the band is what cnt_2 counts
	if (m < 3) { r.stop = kRefitBand; return false; }
	float next[4];
	if (!prior_gen_refit_solve(rec + 4, m, r.O, r.E, r.plane, next)) { r.stop = kRefitDegenerate; return false; }
	++r.solved;
	if (memcmp(next, r.plane, sizeof next) == 0) { r.stop = kRefitFixed; return false; } // step 5
	for (int q = 0; q < 4; ++q) r.launch[q] = next[q];
	r.trial = true;
	return true;
}

} // namespace hcmvs
#endif

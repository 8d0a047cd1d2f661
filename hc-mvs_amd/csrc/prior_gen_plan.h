/* hc-mvs_amd/csrc/prior_gen_plan.h -- the host half of hcmvs_generate_plane_prior_device: what the call
 * refuses before any work, the inverse of K, the level table, min_points and the stop rule of the plane detection, the decoding of the
 * fixed-point sums, the frame and image quad of a plane from its reduced values (tiny, double precision), and the scratch layout.
 * Plain C++ (no HIP); every product is rounded on its own (built with -ffp-contract=off, as the library is). */
#ifndef HCMVS_PRIOR_GEN_PLAN_H
#define HCMVS_PRIOR_GEN_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <cstdio>
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

} // namespace hcmvs
#endif

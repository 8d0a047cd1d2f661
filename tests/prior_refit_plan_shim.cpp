// C face of the refit entries (S4r) of hc-mvs_amd/csrc/prior_gen_plan.h for tests/test_prior_refit_plan.py (ctypes).  Links nothing of the
// library and nothing of HIP; built with -ffp-contract=off as the library is.  With -DPRP_MAIN the file is a stand-alone program that walks
// every entry once (built with the host sanitizers by the test).
#include "../hc-mvs_amd/csrc/prior_gen_plan.h"
#include <cstring>

using namespace hcmvs;

extern "C" {

int prp_check(const uint64_t addr[5], int w, int h, const double* K, const hcmvs_plane_prior_params* p, char* why, int cap) {
	const PriorGenArgs a = {(uintptr_t)addr[0], (uintptr_t)addr[1], (uintptr_t)addr[2], (uintptr_t)addr[3], (uintptr_t)addr[4], w, h, K, p};
	const std::string s = prior_gen_check(a);
	snprintf(why, (size_t)cap, "%s", s.c_str());
	return (int)s.size();
}
int prp_scale(float eps) { return prior_gen_refit_scale(eps); }
int prp_eigvec(const double* C, double* vec) { return prior_gen_refit_eigvec(C, vec); }
void prp_cov(const unsigned long long* words, unsigned long long m, double* mu, double* C) { prior_gen_refit_cov(words, m, mu, C); }
int prp_solve(const unsigned long long* words, unsigned long long m, const double* O, int E, const float* prev, float* out) {
	return prior_gen_refit_solve(words, m, O, E, prev, out) ? 1 : 0;
}
// One round of the decision sequence on records given up front: recs holds nRecs records of kPriorRefitWords words, record i being what
// the launch for the i-th plane asked for returned.  out: solved, kept, stop, records read, cnt_0 .. cnt_3; plane: the final plane;
// asked (nRecs + 1 planes of 4 floats): the planes launched for, the winner first
void prp_round(int R, long long minPoints, const double* O, int E, const float* winner, const int32_t* counts, const unsigned long long* recs, int nRecs, int32_t* out,
               float* plane, float* asked) {
	PriorRefit r = prior_refit_begin(R, minPoints, O, E, winner, counts);
	int used = 0;
	while (used < nRecs) {
		memcpy(asked + 4 * used, r.launch, 16);
		const bool more = prior_refit_step(r, recs + (size_t)used * kPriorRefitWords);
		++used;
		if (!more) break;
	}
	if (r.stop == kRefitGoesOn) memcpy(asked + 4 * used, r.launch, 16); // the records ran out: the plane the next launch is for
	out[0] = r.solved; out[1] = r.kept; out[2] = r.stop; out[3] = used;
	for (int q = 0; q < 4; ++q) { out[4 + q] = (int32_t)r.cnt[q]; plane[q] = r.plane[q]; }
}
// (offset, bytes) of the refit record and of the arrays of S4c, then the offsets of the pieces live in S4; returns how many pairs came first
int prp_scratch(unsigned long long px, unsigned long long scanBytes, unsigned long long sortBytes, unsigned long long n0, unsigned long long* pairs, unsigned long long* live,
                unsigned long long* layout) {
	const PriorGenLayout l = prior_gen_layout((size_t)px, (size_t)scanBytes, (size_t)sortBytes);
	const PriorRefitScratch r = prior_gen_refit_scratch(l);
	const PriorClusterScratch c = prior_gen_cluster_scratch(l, (size_t)px, (size_t)n0, (size_t)scanBytes);
	const PriorScratchPiece v[] = {r.rec, c.keys, c.keys2, c.idx, c.idx2, c.cells, c.start, c.parent, c.sizes, c.marks, c.scan, c.scanTmp, c.sortTmp, c.rec};
	const int n = (int)(sizeof v / sizeof v[0]);
	for (int i = 0; i < n; ++i) { pairs[2 * i] = v[i].off; pairs[2 * i + 1] = v[i].bytes; }
	int k = 0;
	for (const auto piece : kPriorLiveInS4) { live[2 * k] = l.*piece; ++k; }
	// where every live piece ends: the start of the piece that follows it in the layout
	const size_t all[] = {l.flags, l.scan, l.scanTmp, l.xyzA, l.nrmA, l.pixA, l.xyzB, l.nrmB, l.pixB, l.spacing, l.sampleAt, l.assigned, l.stage, l.cand, l.counts, l.winner,
	                      l.acc, l.planes, l.words, l.levels, l.knn.keys, l.bytes};
	for (int i = 0; i < k; ++i) {
		size_t end = l.bytes;
		for (const size_t o : all) if (o > live[2 * i] && o < end) end = o;
		live[2 * i + 1] = end;
	}
	layout[0] = l.acc; layout[1] = l.planes; layout[2] = l.bytes; layout[3] = (unsigned long long)k;
	return n;
}
// 0 the largest refit_iters, 1 / 2 the shifts, 3 the words of a record, 4 / 5 sizeof params / stats, 6 offsetof refit_iters in the params,
// 7 sizeof the refit's own stats, 8 / 9 offsetof refit_rounds / refit_steps in them
void prp_constants(long long* out) {
	out[0] = kPriorMaxRefitIters; out[1] = kPriorRefitFirstShift; out[2] = kPriorRefitSecondShift; out[3] = kPriorRefitWords;
	out[4] = (long long)sizeof(hcmvs_plane_prior_params); out[5] = (long long)sizeof(hcmvs_plane_prior_stats);
	out[6] = (long long)offsetof(hcmvs_plane_prior_params, refit_iters); out[7] = (long long)sizeof(hcmvs_plane_prior_refit_stats);
	out[8] = (long long)offsetof(hcmvs_plane_prior_refit_stats, refit_rounds); out[9] = (long long)offsetof(hcmvs_plane_prior_refit_stats, refit_steps);
}
// what a params struct filled through the binding holds in refit_iters, as C reads it
int prp_read_refit_iters(const hcmvs_plane_prior_params* p) { return p->refit_iters; }

} // extern "C"

#ifdef PRP_MAIN
int main() {
	const double K[9] = {90, 0, 47.5, 0, 90, 39.5, 0, 0, 1};
	hcmvs_plane_prior_params p;
	memset(&p, 0, sizeof p);
	p.conf_max = 0.18f; p.planarity_min = 0.3f; p.n_neighbors = 10; p.probability = 0.01f; p.min_points_div = 80.f; p.epsilon_mul = 2.f; p.normal_threshold = 0.25f;
	p.max_rounds = 256;
	char why[256];
	const uint64_t px = 96 * 80;
	const uint64_t good[5] = {0x10000, 0x10000 + px * 4, 0x10000 + px * 16, 0x10000 + px * 20, 0x10000 + px * 24};
	for (int r = 0; r <= 16; ++r) { p.refit_iters = r; if (prp_check(good, 96, 80, K, &p, why, (int)sizeof why) != 0) return 1; }
	p.refit_iters = 17;
	if (prp_check(good, 96, 80, K, &p, why, (int)sizeof why) == 0 || !strstr(why, "refit_iters")) return 2;
	p.refit_iters = -1;
	if (prp_check(good, 96, 80, K, &p, why, 8) == 0) return 3; // (a short buffer: the message is cut, not overrun)
	if (prp_scale(0.75f) != 0 || prp_scale(1.f) != 1 || prp_scale(0.5f) != 0 || prp_scale(0.49f) != -1 || prp_scale(0.f) != 0 || prp_scale(INFINITY) != 0 || prp_scale(NAN) != 0) return 4;
	double vec[3];
	const double diag[6] = {3, 0, 0, 1, 0, 2}, zero[6] = {0, 0, 0, 0, 0, 0}, full[6] = {2, 0.5, -0.25, 1, 0.125, 3};
	if (prp_eigvec(diag, vec) != 0 || vec[1] != 1.0) return 5;
	if (prp_eigvec(zero, vec) != 0 || vec[0] != 1.0) return 6;
	const int sweeps = prp_eigvec(full, vec);
	if (sweeps < 1 || sweeps > 16 || !(std::fabs(((vec[0] * vec[0] + vec[1] * vec[1]) + vec[2] * vec[2]) - 1.0) < 1e-12)) return 7;
	// four samples of the plane z = 1 about the anchor (0, 0, 1), E = 0: s = (+-1, +-1, 0)
	unsigned long long rec[kPriorRefitWords] = {};
	rec[0] = rec[1] = rec[2] = rec[3] = 4;
	rec[4 + 6 + 1] = 4ull << kPriorRefitSecondShift;     // xx, low word
	rec[4 + 12 + 1] = 4ull << kPriorRefitSecondShift;    // yy
	const double O[3] = {0, 0, 1};
	const float winner[4] = {0.01f, 0.f, 0.99995f, 1.f};
	const int32_t counts[4] = {4, 4, 4, 4};
	int32_t out[8];
	float plane[4], asked[4 * 4];
	unsigned long long recs[3 * kPriorRefitWords];
	for (int i = 0; i < 3; ++i) memcpy(recs + i * kPriorRefitWords, rec, sizeof rec);
	prp_round(4, 3, O, 0, winner, counts, recs, 3, out, plane, asked);
	if (out[0] != 2 || out[1] != 1 || out[2] != kRefitFixed || out[3] != 2 || plane[2] != 1.f || plane[3] != 1.f || plane[0] != 0.f) return 8;
	prp_round(1, 3, O, 0, winner, counts, recs, 3, out, plane, asked);
	if (out[0] != 1 || out[1] != 1 || out[2] != kRefitIters || out[3] != 2) return 9;
	prp_round(4, 5, O, 0, winner, counts, recs, 3, out, plane, asked);
	if (out[0] != 1 || out[1] != 0 || out[2] != kRefitCount || plane[0] != 0.01f) return 10;
	recs[2] = 2;
	prp_round(4, 3, O, 0, winner, counts, recs, 3, out, plane, asked);
	if (out[0] != 0 || out[2] != kRefitBand || out[3] != 1) return 11;
	unsigned long long pairs[28], live[32], lay[4];
	if (prp_scratch(px, 1000, 3000, px, pairs, live, lay) != 14) return 12;
	if (pairs[0] != lay[0] || pairs[0] + pairs[1] > lay[1]) return 13;
	long long k[10];
	prp_constants(k);
	p.refit_iters = 7;
	if (prp_read_refit_iters(&p) != 7 || k[7] != 8) return 15;
	if (k[0] != 16 || k[3] * 8 != (long long)pairs[1]) return 14;
	printf("prior_refit_plan ok %d %lld %lld\n", sweeps, k[4], k[5]);
	return 0;
}
#endif

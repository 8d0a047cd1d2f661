// C face of hc-mvs_amd/csrc/prior_gen_plan.h for tests/test_prior_gen_plan.py (ctypes).  Links nothing of the library and nothing of HIP.
// Addresses come in as plain integers: nothing here is dereferenced or allocated on a device.  With -DPGP_MAIN the file is a stand-alone
// program that walks every entry once (built with the host sanitizers by the test).
#include "../hc-mvs_amd/csrc/prior_gen_plan.h"
#include <cstring>

using namespace hcmvs;

extern "C" {

// the reason a call is refused into `why` (empty: it may run); returns its length
int pgp_check(const uint64_t addr[5], int w, int h, const double* K, const hcmvs_plane_prior_params* p, char* why, int cap) {
	const PriorGenArgs a = {(uintptr_t)addr[0], (uintptr_t)addr[1], (uintptr_t)addr[2], (uintptr_t)addr[3], (uintptr_t)addr[4], w, h, K, p};
	const std::string s = prior_gen_check(a);
	snprintf(why, (size_t)cap, "%s", s.c_str());
	return (int)s.size();
}
int pgp_kinv(const double* K, double* inv) { return prior_gen_kinv(K, inv) ? 1 : 0; }
void pgp_ray(const double* inv, int x, int y, float* r) { prior_gen_ray(inv, x, y, r); }
int pgp_levels(int w, int h, int32_t* levels) { return prior_gen_levels(w, h, levels); }
long long pgp_min_points(unsigned long long n0, float div) { return (long long)prior_gen_min_points(n0, div); }
int pgp_fail_limit(float probability, long long minPoints, unsigned long long n0, int maxRounds) { return prior_gen_fail_limit(probability, minPoints, n0, maxRounds); }
float pgp_eps(double avg, float mul) { return prior_gen_eps(avg, mul); }
float pgp_cell(double avg, float mul) { return prior_gen_cluster_cell(avg, mul); }
int pgp_cell_usable(float cell) { return prior_gen_cluster_cell_usable(cell) ? 1 : 0; }
double pgp_mean(long long hi, unsigned long long lo, unsigned long long n, int shift) { return prior_gen_mean(hi, lo, n, shift); }
void pgp_frame(const float* n, double* b1, double* b2) { prior_gen_frame(n, b1, b2); }
int pgp_quad(const double* K, const double* c, const double* b1, const double* b2, const double* uv, const int32_t* box, double* quad) {
	return prior_gen_quad(K, c, b1, b2, uv, box, quad);
}
// the offsets of the layout in declaration order, then the knn pieces, then the total; returns how many
int pgp_layout(unsigned long long px, unsigned long long scanBytes, unsigned long long sortBytes, unsigned long long* out) {
	const PriorGenLayout l = prior_gen_layout((size_t)px, (size_t)scanBytes, (size_t)sortBytes);
	const size_t v[] = {l.flags, l.scan, l.scanTmp, l.xyzA, l.nrmA, l.pixA, l.xyzB, l.nrmB, l.pixB, l.spacing, l.sampleAt, l.assigned, l.stage, l.cand, l.counts, l.winner,
	                    l.acc, l.planes, l.words, l.levels, l.knn.keys, l.knn.keys2, l.knn.idx, l.knn.idx2, l.knn.sorted, l.knn.pos, l.knn.box, l.knn.sort, l.bytes};
	const int n = (int)(sizeof v / sizeof v[0]);
	for (int i = 0; i < n; ++i) out[i] = v[i];
	return n;
}
// (offset, bytes) of the arrays of S4c for n0 samples, in the order of PriorClusterScratch; returns how many arrays
int pgp_cluster_scratch(unsigned long long px, unsigned long long scanBytes, unsigned long long sortBytes, unsigned long long n0, unsigned long long* out) {
	const PriorClusterScratch c = prior_gen_cluster_scratch(prior_gen_layout((size_t)px, (size_t)scanBytes, (size_t)sortBytes), (size_t)px, (size_t)n0, (size_t)scanBytes);
	const PriorScratchPiece v[] = {c.keys, c.keys2, c.idx, c.idx2, c.cells, c.start, c.parent, c.sizes, c.marks, c.scan, c.scanTmp, c.sortTmp, c.rec};
	const int n = (int)(sizeof v / sizeof v[0]);
	for (int i = 0; i < n; ++i) { out[2 * i] = v[i].off; out[2 * i + 1] = v[i].bytes; }
	return n;
}
// the offsets of the pieces that are live during S4; returns how many
int pgp_live_in_s4(unsigned long long px, unsigned long long scanBytes, unsigned long long sortBytes, unsigned long long* out) {
	const PriorGenLayout l = prior_gen_layout((size_t)px, (size_t)scanBytes, (size_t)sortBytes);
	int n = 0;
	for (const auto piece : kPriorLiveInS4) out[n++] = l.*piece;
	return n;
}
// 0..5 the constants, 6..9 struct sizes, 10 the cap of a cell coordinate, 11..14 offsetof cluster_mul / cluster_eps / cluster_rejects / cluster_left
void pgp_constants(long long* out) {
	out[0] = kPriorCandidates; out[1] = kPriorMaxLevels; out[2] = kPriorMaxRounds; out[3] = kPriorSpacingShift; out[4] = kPriorCoordShift; out[5] = HCMVS_MAX_PRIOR_PLANES;
	out[6] = (long long)sizeof(PriorPlaneDev); out[7] = (long long)sizeof(hcmvs_prior_plane); out[8] = (long long)sizeof(hcmvs_plane_prior_params);
	out[9] = (long long)sizeof(hcmvs_plane_prior_stats); out[10] = (long long)kPriorClusterCellCap;
	out[11] = (long long)offsetof(hcmvs_plane_prior_params, cluster_mul); out[12] = (long long)offsetof(hcmvs_plane_prior_stats, cluster_eps);
	out[13] = (long long)offsetof(hcmvs_plane_prior_stats, cluster_rejects); out[14] = (long long)offsetof(hcmvs_plane_prior_stats, cluster_left);
}

} // extern "C"

#ifdef PGP_MAIN
int main() {
	const double K[9] = {90, 0, 47.5, 0, 90, 39.5, 0, 0, 1};
	hcmvs_plane_prior_params p;
	memset(&p, 0, sizeof p);
	p.conf_max = 0.18f; p.planarity_min = 0.3f; p.n_neighbors = 10; p.probability = 0.01f; p.min_points_div = 80.f; p.epsilon_mul = 2.f; p.normal_threshold = 0.25f;
	p.max_rounds = 256;
	char why[256];
	const uint64_t px = 96 * 80;
	const uint64_t good[5] = {0x10000, 0x10000 + px * 4, 0x10000 + px * 16, 0x10000 + px * 20, 0x10000 + px * 24}, bad[5] = {0x10000, 0x10000 + px * 4, 0x10000 + px * 16, 0x10000, 0};
	if (pgp_check(good, 96, 80, K, &p, why, (int)sizeof why) != 0) return 1;
	if (pgp_check(bad, 96, 80, K, &p, why, (int)sizeof why) == 0) return 2;
	p.n_neighbors = 40;
	if (pgp_check(good, 96, 80, K, &p, why, 8) == 0) return 3; // (a short buffer: the message is cut, not overrun)
	double inv[6], b1[3], b2[3], quad[8];
	float r[3];
	if (!pgp_kinv(K, inv)) return 4;
	pgp_ray(inv, 95, 79, r);
	int32_t levels[kPriorMaxLevels];
	if (pgp_levels(1920, 1080, levels) != 9 || pgp_levels(96, 80, levels) != 5 || pgp_levels(2, 2, levels) != 1 || pgp_levels(1 << 20, 8, levels) != kPriorMaxLevels) return 5;
	if (pgp_min_points(4597, 80.f) != 57 || pgp_min_points(7, 80.f) != 3 || pgp_min_points(~0ull, 1e-30f) < 3) return 6;
	if (pgp_fail_limit(0.01f, 57, 4597, 256) != 2 || pgp_fail_limit(0.01f, 5, 4, 256) != 1 || pgp_fail_limit(1e-30f, 3, 1u << 30, 7) != 7) return 7;
	if (pgp_eps(0.5, 2.f) != 1.f) return 8;
	if (pgp_mean(-1, 0xffffffffull, 1, 32) >= 0 || pgp_mean(3, 1ull << 31, 7, 32) != 0.5) return 9;
	const float n[3] = {0.6f, 0.f, 0.8f};
	pgp_frame(n, b1, b2);
	const double c[3] = {0, 0, 5}, uv[4] = {-1, 1, -1, 1}, wide[4] = {-100, 100, -100, 100};
	const int32_t box[4] = {3, 9, 4, 8};
	if (pgp_quad(K, c, b1, b2, uv, box, quad) != 0 || pgp_quad(K, c, b1, b2, wide, box, quad) != 1) return 10;
	unsigned long long lay[40];
	const int m = pgp_layout(px, 1000, 3000, lay);
	for (int i = 1; i < m; ++i) if (lay[i] <= lay[i - 1] || lay[i] % 256) return 11;
	p.n_neighbors = 10;
	if (pgp_check(good, 96, 80, K, &p, why, (int)sizeof why) != 0) return 12;
	p.cluster_mul = 7.f;
	if (pgp_check(good, 96, 80, K, &p, why, (int)sizeof why) != 0) return 13;
	p.cluster_mul = -1.f;
	if (pgp_check(good, 96, 80, K, &p, why, (int)sizeof why) == 0 || !strstr(why, "cluster_mul")) return 14;
	p.cluster_mul = NAN;
	if (pgp_check(good, 96, 80, K, &p, why, 8) == 0) return 15; // (a short buffer again)
	p.cluster_mul = INFINITY;
	if (pgp_check(good, 96, 80, K, &p, why, (int)sizeof why) == 0) return 16;
	if (pgp_cell(0.5, 2.f) != 1.f || !pgp_cell_usable(pgp_cell(0.05, 7.f))) return 17;
	if (pgp_cell(0.05, 1e-45f) != 0.f || pgp_cell_usable(pgp_cell(0.05, 1e-45f)) || pgp_cell_usable(pgp_cell(1e30, 1e30f)) || pgp_cell_usable(-1.f)) return 18;
	unsigned long long cl[26], live[16];
	if (pgp_cluster_scratch(px, 1000, 3000, px, cl) != 13 || pgp_live_in_s4(px, 1000, 3000, live) != 10) return 19;
	for (int i = 0; i < 13; ++i) if (cl[2 * i] + cl[2 * i + 1] > lay[m - 1]) return 20;
	long long k[15];
	pgp_constants(k);
	if (k[10] != (1ll << 30)) return 21;
	printf("prior_gen_plan ok %d %llu\n", m, lay[m - 1]);
	printf("prior_cluster_plan ok %lld %lld\n", k[8], k[9]);
	return 0;
}
#endif

// C face of what the inlier clustering adds to hc-mvs_amd/csrc/prior_gen_plan.h, for tests/test_prior_cluster_plan.py (ctypes).  Links nothing
// of the library and nothing of HIP.  With -DPCP_MAIN the file is a stand-alone program that walks every entry once (built with the host
// sanitizers by the test).
#include "../hc-mvs_amd/csrc/prior_gen_plan.h"
#include <cstring>

using namespace hcmvs;

extern "C" {

// prior_gen_check of an otherwise good call with these parameters: the reason into `why` (empty: it may run); returns its length
int pcp_check(const hcmvs_plane_prior_params* p, char* why, int cap) {
	static const double K[9] = {90, 0, 47.5, 0, 90, 39.5, 0, 0, 1};
	const uint64_t px = 96 * 80, base = 0x100000;
	const PriorGenArgs a = {(uintptr_t)base, (uintptr_t)(base + px * 4), (uintptr_t)(base + px * 16), (uintptr_t)(base + px * 20), (uintptr_t)(base + px * 24), 96, 80, K, p};
	const std::string s = prior_gen_check(a);
	snprintf(why, (size_t)cap, "%s", s.c_str());
	return (int)s.size();
}
float pcp_cell(double avg, float mul) { return prior_gen_cluster_cell(avg, mul); }
int pcp_cell_usable(float cell) { return prior_gen_cluster_cell_usable(cell) ? 1 : 0; }
// the cap of a cell coordinate, sizeof the parameters and the stats, offsetof cluster_mul / cluster_eps / cluster_rejects / cluster_left
void pcp_constants(long long* out) {
	out[0] = (long long)kPriorClusterCellCap; out[1] = (long long)sizeof(hcmvs_plane_prior_params); out[2] = (long long)sizeof(hcmvs_plane_prior_stats);
	out[3] = (long long)offsetof(hcmvs_plane_prior_params, cluster_mul); out[4] = (long long)offsetof(hcmvs_plane_prior_stats, cluster_eps);
	out[5] = (long long)offsetof(hcmvs_plane_prior_stats, cluster_rejects); out[6] = (long long)offsetof(hcmvs_plane_prior_stats, cluster_left);
}

} // extern "C"

#ifdef PCP_MAIN
int main() {
	hcmvs_plane_prior_params p;
	memset(&p, 0, sizeof p);
	p.conf_max = 0.18f; p.planarity_min = 0.3f; p.n_neighbors = 10; p.probability = 0.01f; p.min_points_div = 80.f; p.epsilon_mul = 2.f; p.normal_threshold = 0.25f;
	p.max_rounds = 256;
	char why[256];
	if (pcp_check(&p, why, (int)sizeof why) != 0) return 1;
	p.cluster_mul = 7.f;
	if (pcp_check(&p, why, (int)sizeof why) != 0) return 2;
	p.cluster_mul = -1.f;
	if (pcp_check(&p, why, (int)sizeof why) == 0 || !strstr(why, "cluster_mul")) return 3;
	p.cluster_mul = NAN;
	if (pcp_check(&p, why, 8) == 0) return 4; // (a short buffer: the message is cut, not overrun)
	p.cluster_mul = INFINITY;
	if (pcp_check(&p, why, (int)sizeof why) == 0) return 5;
	if (pcp_cell(0.5, 2.f) != 1.f || !pcp_cell_usable(pcp_cell(0.05, 7.f))) return 6;
	if (pcp_cell(0.05, 1e-45f) != 0.f || pcp_cell_usable(pcp_cell(0.05, 1e-45f)) || pcp_cell_usable(pcp_cell(1e30, 1e30f)) || pcp_cell_usable(-1.f)) return 7;
	long long k[7];
	pcp_constants(k);
	if (k[0] != (1ll << 30)) return 8;
	printf("prior_cluster_plan ok %lld %lld\n", k[1], k[2]);
	return 0;
}
#endif

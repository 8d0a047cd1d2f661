// C face of what --plane-refit adds to hc-mvs_amd/host/driver_plan.h, for tests/test_driver_plane_refit_plan.py (ctypes).  Links nothing of the
// library and nothing of HIP.
#include "../hc-mvs_amd/host/driver_plan.h"

using namespace driverplan;

extern "C" {
// parse_options on argv[0 .. argc): "key=value" lines of the option, of what it reaches in the detection's parameters, "result" and "err"
const char* dpr_parse(int argc, char** argv) {
	static std::string text;
	Options o;
	std::string err;
	const ParseResult res = parse_options(argc, argv, o, err);
	hcmvs_plane_prior_params base = {};
	base.conf_max = 0.18f; base.n_neighbors = 10; base.max_rounds = 256;
	const hcmvs_plane_prior_params p = plane_prior_params(o, base);
	std::ostringstream s;
	s << "result=" << (int)res << "\nerr=" << err << "\nplaneRefit=" << o.planeRefit << "\nplanePriors=" << o.planePriors << "\nrefit_iters=" << p.refit_iters
	  << "\ncluster_mul=" << p.cluster_mul << "\nnotes=" << o.notes.size() << "\n";
	text = s.str();
	return text.c_str();
}
// the option tables, one name per line: 0 the refit's own, 1 the clustering's, 2 the priors'
const char* dpr_tables(int which) {
	static std::string text;
	text.clear();
	if (which == 0) for (const char* k : kPlaneRefitOptions) text += std::string(k) + "\n";
	else if (which == 1) for (const char* k : kPlaneClusterOptions) text += std::string(k) + "\n";
	else for (const char* k : kPriorOptions) text += std::string(k) + "\n";
	return text.c_str();
}
const char* dpr_usage() { return kUsage; }
}

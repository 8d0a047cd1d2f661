// C face of what --plane-clusters adds to hc-mvs_amd/host/driver_plan.h, for tests/test_driver_plane_cluster_plan.py (ctypes).  Links nothing
// of the library and nothing of HIP.
#include "../hc-mvs_amd/host/driver_plan.h"

using namespace driverplan;

extern "C" {
// parse_options on argv[0 .. argc): "key=value" lines of the options of the clustering, "result", "err" and the notes
const char* dpc_parse(int argc, char** argv) {
	static std::string text;
	Options o;
	std::string err;
	const ParseResult res = parse_options(argc, argv, o, err);
	hcmvs_plane_prior_params base = {};
	base.cluster_mul = 123.f; // (the plan sets the field in every case)
	const hcmvs_plane_prior_params p = plane_prior_params(o, base);
	std::ostringstream s;
	s << "result=" << (int)res << "\nerr=" << err << "\nplanePriors=" << o.planePriors << "\nplaneClusters=" << o.planeClusters << "\nransacCluster=" << o.ransacCluster
	  << "\ncluster_mul=" << p.cluster_mul << "\nepsilon_mul=" << p.epsilon_mul << "\n";
	for (const auto& note : o.notes) s << "note=" << note << "\n";
	text = s.str();
	return text.c_str();
}
// the three option tables, one name per line
const char* dpc_tables(int which) {
	static std::string text;
	text.clear();
	if (which == 0) for (const char* k : kKnownOptions) text += std::string(k) + "\n";
	else if (which == 1) for (const char* k : kPriorOptions) text += std::string(k) + "\n";
	else for (const char* k : kPlaneClusterOptions) text += std::string(k) + "\n";
	return text.c_str();
}
const char* dpc_usage() { return kUsage; }
}

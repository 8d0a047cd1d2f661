// C face of what the depth priors add to hc-mvs_amd/host/driver_plan.h, for tests/test_driver_prior_plan.py (ctypes).  Links nothing of
// the library and nothing of HIP.
#include "../hc-mvs_amd/host/driver_plan.h"

using namespace driverplan;

extern "C" {
// parse_options on argv[0 .. argc): "key=value" lines of the prior options, "result", "err" and the notes
const char* dq_parse(int argc, char** argv) {
	static std::string text;
	Options o;
	std::string err;
	const ParseResult res = parse_options(argc, argv, o, err);
	std::ostringstream s;
	s << "result=" << (int)res << "\nerr=" << err << "\ndepthPriors=" << o.depthPriors << "\nparaPrior=" << o.paraPrior << "\nsigmaPrior=" << o.sigmaPrior
	  << "\nphoto2geo=" << o.photo2geo << "\nviewspread=" << o.viewspread << "\nrestoreHypothesis=" << o.restoreHypothesis << "\n";
	for (const auto& note : o.notes) s << "note=" << note << "\n";
	text = s.str();
	return text.c_str();
}
// out[2]: the extra sweeps follow the estimates of iteration `it`; the priors are never used
void dq_schedule(const char* folder, int nExternal, int it, int* out) {
	Options o;
	o.depthPriors = folder; o.estimationItersExternal = nExternal;
	out[0] = prior_sweeps_after(o, it); out[1] = priors_never_used(o);
}
const char* dq_path(const char* folder, unsigned id) {
	static std::string text;
	Options o;
	o.depthPriors = folder;
	text = prior_path(o, id);
	return text.c_str();
}
}

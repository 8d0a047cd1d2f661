// C face of what the plane priors add to hc-mvs_amd/host/driver_plan.h, for tests/test_driver_plane_prior_plan.py (ctypes).  Links nothing
// of the library and nothing of HIP.
#include "../hc-mvs_amd/host/driver_plan.h"

using namespace driverplan;

extern "C" {
// parse_options on argv[0 .. argc): "key=value" lines of the plane-prior options, "result", "err" and the notes
const char* dpp_parse(int argc, char** argv) {
	static std::string text;
	Options o;
	std::string err;
	const ParseResult res = parse_options(argc, argv, o, err);
	hcmvs_plane_prior_params base = {};
	base.conf_max = 0.18f; base.n_neighbors = 10; base.max_rounds = 256; // (what the options do not touch comes through)
	const hcmvs_plane_prior_params p = plane_prior_params(o, base);
	std::ostringstream s;
	s << "result=" << (int)res << "\nerr=" << err << "\nplanePriors=" << o.planePriors << "\nexportPriors=" << o.exportPriors << "\ndepthPriors=" << o.depthPriors
	  << "\nprobability=" << p.probability << "\nepsilon_mul=" << p.epsilon_mul << "\nmin_points_div=" << p.min_points_div << "\nseed=" << p.seed
	  << "\nregion_label=" << p.region_label << "\nn_neighbors=" << p.n_neighbors << "\nmax_rounds=" << p.max_rounds << "\n";
	for (const auto& note : o.notes) s << "note=" << note << "\n";
	text = s.str();
	return text.c_str();
}
// out[2]: the priors are generated (and the extra sweeps run) after the estimates of iteration `it`; no prior is ever generated
void dpp_schedule(int planePriors, int nExternal, int it, int* out) {
	Options o;
	o.planePriors = planePriors; o.estimationItersExternal = nExternal;
	out[0] = prior_sweeps_after(o, it); out[1] = priors_never_used(o);
}
const char* dpp_path(const char* folder, unsigned id) {
	static std::string text;
	Options o;
	o.exportPriors = folder;
	text = export_prior_path(o, id);
	return text.c_str();
}
// the two option tables, one name per line
const char* dpp_tables(int which) {
	static std::string text;
	text.clear();
	if (which == 0) for (const char* k : kKnownOptions) text += std::string(k) + "\n";
	else for (const char* k : kPriorOptions) text += std::string(k) + "\n";
	return text.c_str();
}
}

// C face of what the geometric-consistency term adds to hc-mvs_amd/host/driver_plan.h, for tests/test_driver_geo_plan.py (ctypes).  Links
// nothing of the library and nothing of HIP.
#include "../hc-mvs_amd/host/driver_plan.h"

using namespace driverplan;

extern "C" {
// parse_options on argv[0 .. argc): "key=value" lines of the term's options, "result", "err" and the notes
const char* dg_parse(int argc, char** argv) {
	static std::string text;
	Options o;
	std::string err;
	const ParseResult res = parse_options(argc, argv, o, err);
	const hcmvs_geo_params gp = geo_params(o);
	std::ostringstream s;
	s << "result=" << (int)res << "\nerr=" << err << "\non=" << gp.on << "\npara_tapa=" << gp.para_tapa << "\npara_tapa2=" << gp.para_tapa2
	  << "\ntxthreshold=" << gp.txthreshold << "\ntxthreshold2=" << gp.txthreshold2 << "\nphoto2geo=" << gp.photo2geo << "\nmax_px=" << gp.max_px << "\n";
	for (const auto& note : o.notes) s << "note=" << note << "\n";
	text = s.str();
	return text.c_str();
}
// out[3]: snapshotSpread, liveSpread, serial of outer iteration `it` (the source views offer their maps as for view spread)
void dg_iteration(int geo, int interleave, int nExternal, int it, int* out) {
	Options o;
	o.geoConsistency = geo; o.postFilterInterleave = interleave; o.estimationItersExternal = nExternal;
	const IterPlan p = plan_iteration(o, it, true);
	out[0] = p.snapshotSpread; out[1] = p.liveSpread; out[2] = p.serial;
}
const char* dg_usage() { return kUsage; }
}

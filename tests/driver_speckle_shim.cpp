// C face of what --speckle-size and --speckle-diff add to hc-mvs_amd/host/driver_plan.h, for tests/test_driver_speckle_plan.py (ctypes).
// Links nothing of the library and nothing of HIP.
#include "../hc-mvs_amd/host/driver_plan.h"
#include <cstring>

using namespace driverplan;

extern "C" {
// parse_options on argv[0 .. argc): "key=value" lines of the two options (the threshold also as its bits), "result" and "err"
const char* dps_parse(int argc, char** argv) {
	static std::string text;
	Options o;
	std::string err;
	const ParseResult res = parse_options(argc, argv, o, err);
	uint32_t bits;
	memcpy(&bits, &o.speckleDiff, 4);
	std::ostringstream s;
	s << "result=" << (int)res << "\nerr=" << err << "\nspeckleSize=" << o.speckleSize << "\nspeckleDiffBits=" << bits << "\npostFilter=" << o.postFilter
	  << "\nnFilter=" << o.nFilter << "\nnotes=" << o.notes.size() << "\n";
	text = s.str();
	return text.c_str();
}
// the option tables, one name per line: 0 the speckle filter's own, 1 the first table, 2 the refit's
const char* dps_tables(int which) {
	static std::string text;
	text.clear();
	if (which == 0) for (const char* k : kSpeckleOptions) text += std::string(k) + "\n";
	else if (which == 1) for (const char* k : kKnownOptions) text += std::string(k) + "\n";
	else for (const char* k : kPlaneRefitOptions) text += std::string(k) + "\n";
	return text.c_str();
}
const char* dps_usage() { return kUsage; }
}

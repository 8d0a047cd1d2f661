// C face of hc-mvs_amd/csrc/speckle_plan.h (the rule, the refusals, the tile table and the scratch layout of the speckle filter) for
// tests/test_speckle_plan.py (ctypes, through tests/speckle_lib.py).  Built with g++ alone: nothing of the library, nothing of HIP.
// Addresses handed to the plan are plain integers; nothing there is read.
#include "../hc-mvs_amd/csrc/speckle_plan.h"
#include <cstring>

using namespace hcmvs;

extern "C" {

void ss_constants(int* out) {
	out[0] = (int)sizeof(SpeckleArgs); out[1] = kSpeckleTileW; out[2] = kSpeckleTileH; out[3] = kSpeckleBlock; out[4] = kSpeckleMaxItems;
	out[5] = (int)sizeof(SpeckleItem); out[6] = (int)sizeof(SpecklePartial); out[7] = (int)sizeof(SpeckleResult); out[8] = (int)kSpeckleScratchPerPixel;
}

float ss_default_threshold() { return speckle_default_threshold(); }

// 0: the call may run; 1: refused, the reason in why
int ss_check(const SpeckleArgs* items, int n, float thr, char* why, int cap) {
	const std::string s = speckle_check(items, n, thr);
	if (why && cap > 0) { strncpy(why, s.c_str(), (size_t)cap - 1); why[cap - 1] = 0; }
	return s.empty() ? 0 : 1;
}

// first, pixel0: n + 1 entries each.  Returns whether the grid fits a launch
int ss_tiles(const SpeckleArgs* items, int n, int64_t* first, int64_t* pixel0) {
	const SpeckleTiles t = speckle_tiles(items, n);
	for (int i = 0; i <= n; ++i) { first[i] = t.first[(size_t)i]; pixel0[i] = t.pixel0[(size_t)i]; }
	return speckle_grid_fits(t) ? 1 : 0;
}

// out: result, items, first, staged, partials, labels, sizes, bytes
void ss_layout(int n, uint64_t nTiles, uint64_t nPixels, uint64_t* out) {
	const SpeckleLayout l = speckle_layout(n, (size_t)nTiles, (size_t)nPixels);
	out[0] = l.result; out[1] = l.items; out[2] = l.first; out[3] = l.staged; out[4] = l.partials; out[5] = l.labels; out[6] = l.sizes; out[7] = l.bytes;
}

int ss_joined(float dp, float dq, float thr) { return speckle_valid(dp) && speckle_valid(dq) && speckle_joined(dp, dq, thr) ? 1 : 0; }

} // extern "C"

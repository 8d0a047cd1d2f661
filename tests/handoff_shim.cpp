// C face of hc-mvs_amd/csrc/handoff_plan.h (the refusals and the launch plan of the hand-off) and of the stand-alone driver's own
// hand-off (hc-mvs_amd/host/scene_io.h resize_cubic + the clean-up loop of its loader) for tests/test_handoff_host.py (ctypes).  Built
// with g++ alone: nothing of the library, nothing of HIP.  Addresses handed to the plan are plain integers; nothing there is read.
#include "../hc-mvs_amd/csrc/handoff_plan.h"
#include "../hc-mvs_amd/host/scene_io.h"
#include <cstring>

using namespace hcmvs;

extern "C" {

void hs_layout(int* out) {
	out[0] = (int)sizeof(HandoffArgs); out[1] = kHandoffBlock; out[2] = kHandoffChunk; out[3] = kHandoffMaxItems;
	out[4] = (int)sizeof(HandoffResult); out[5] = (int)sizeof(HandoffItem);
}

// 0: the call may run; 1: refused, the reason in why
int hs_check(const HandoffArgs* items, int n, int mode, char* why, int cap) {
	const std::string s = handoff_check(items, n, mode);
	if (why && cap > 0) { strncpy(why, s.c_str(), (size_t)cap - 1); why[cap - 1] = 0; }
	return s.empty() ? 0 : 1;
}

// first: n + 1 entries
void hs_first(const HandoffArgs* items, int n, int32_t* first) {
	const std::vector<int32_t> f = handoff_first(items, n);
	for (int i = 0; i <= n; ++i) first[i] = f[(size_t)i];
}

void hs_geom(int sw, int sh, int dw, int dh, double* ratios) {
	const HandoffGeom g = handoff_geom(sw, sh, dw, dh);
	ratios[0] = g.rx; ratios[1] = g.ry; ratios[2] = g.ix; ratios[3] = g.iy;
}

// what the stand-alone driver does with the previous level's maps today (Loader::hand_over): swap when the sizes agree, else
// sceneio::resize_cubic of both maps; then its clean-up loop.  range: lo * 0.9f, hi * 1.1f (left alone when no depth is valid).
// Returns 0, or 3 (the driver's "holds no valid depth")
int hs_driver_hand_over(const float* sd, const float* sn, int sw, int sh, float* dd, float* dn, int dw, int dh, float* range) {
	const size_t n = (size_t)dw * dh;
	std::vector<float> pd(sd, sd + (size_t)sw * sh), pn(sn, sn + (size_t)sw * sh * 3), Md, Mn;
	if (sw == dw && sh == dh) { Md.swap(pd); Mn.swap(pn); }
	else { sceneio::resize_cubic(pd, sw, sh, 1, Md, dw, dh); sceneio::resize_cubic(pn, sw, sh, 3, Mn, dw, dh); }
	float lo = 3.402823466e+38f, hi = 0.f;
	for (size_t q_ = 0; q_ < n; ++q_) {
		if (!(Md[q_] > 0.f)) Md[q_] = 0.f;
		lo = std::min(lo, Md[q_]); hi = std::max(hi, Md[q_]);
		if (Md[q_] == 0.f) continue;
		float* q = &Mn[3 * q_];
		const float len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
		if (len > 0.f) { q[0] /= len; q[1] /= len; q[2] /= len; }
	}
	memcpy(dd, Md.data(), n * 4); memcpy(dn, Mn.data(), n * 12);
	if (!(hi > 0.f)) return 3;
	range[0] = lo * 0.9f; range[1] = hi * 1.1f;
	return 0;
}

} // extern "C"

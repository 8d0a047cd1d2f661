/* hc-mvs_amd/csrc/handoff_host.cpp -- the hand-off between two pyramid levels on the host: the rule of handoff_device.h in a plain loop
 * over the destination pixels, the comparisons of the range as they stand.  Plain C++ (no HIP, no context): what hcmvs_handoff_maps runs,
 * and what the device form (handoff_kernels.hip) is pinned to. */
#include "handoff_host.h"
#include <algorithm>

namespace hcmvs {

bool handoff_host(int mode, const HandoffGeom& g, const float* srcDepth, const float* srcNormal, float* dstDepth, float* dstNormal, float* dMin, float* dMax,
                  HandoffResult& r) {
	r = HandoffResult();
	HandoffPixel p;
	if (mode == kHandoffInit) {
		float lo = 3.402823466e+38f, hi = 0.f;
		for (int y = 0; y < g.dh; ++y)
			for (int x = 0; x < g.dw; ++x) {
				handoff_init_pixel(g, srcDepth, srcNormal, x, y, p);
				const size_t at = (size_t)y * g.dw + x;
				dstDepth[at] = p.d;
				dstNormal[3 * at] = p.n[0]; dstNormal[3 * at + 1] = p.n[1]; dstNormal[3 * at + 2] = p.n[2];
				lo = std::min(lo, p.d); hi = std::max(hi, p.d);
				r.valid += p.valid; r.clamped += p.clamped; r.rescaled += p.rescaled;
			}
		if (!(hi > 0.f)) return false; // "no valid depth": the range stays as it was
		*dMin = lo * 0.9f; *dMax = hi * 1.1f;
		return true;
	}
	float lo = *dMin, hi = *dMax;
	for (int y = 0; y < g.dh; ++y)
		for (int x = 0; x < g.dw; ++x) {
			handoff_hint_pixel(g, srcDepth, srcNormal, x, y, p);
			const size_t at = (size_t)y * g.dw + x;
			const float hd = p.raw; // before the clean-up
			lo = lo > hd ? hd : lo; hi = hi > hd ? hi : hd;
			dstDepth[at] = p.d;
			dstNormal[3 * at] = p.n[0]; dstNormal[3 * at + 1] = p.n[1]; dstNormal[3 * at + 2] = p.n[2];
			r.valid += p.valid; r.clamped += p.clamped; r.rescaled += p.rescaled;
		}
	*dMin = lo > 0.f ? lo : 0.f;  // max(lo, 0), a zero of either sign as +0
	*dMax = hi == 0.f ? 0.f : hi;
	return true;
}

} // namespace hcmvs

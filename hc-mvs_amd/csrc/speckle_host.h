/* hc-mvs_amd/csrc/speckle_host.h -- the speckle filter as a sequential flood fill: the library's CPU form (hcmvs_remove_speckles), plain
 * C++ (no HIP).  It restates upstream's speckle removal (SceneDensify.cpp:1973-2041) with the symmetric edge rule of speckle_plan.h
 * (DESIGN.md section 5, D15): the map is scanned in raster order; an unlabelled valid pixel opens a segment, which is grown over an
 * explicit stack through joined 4-neighbours; the opening pixel is the first of its segment in raster order, hence its canonical label.
 * A segment smaller than speckle_size is cleared once it is complete.  Because the edges are symmetric the segments are the components
 * of an undirected graph, whatever the visiting order. */
#ifndef HCMVS_SPECKLE_HOST_H
#define HCMVS_SPECKLE_HOST_H
#include <vector>
#include "speckle_plan.h"
namespace hcmvs {

// depth: w * h, in/out.  normal (w * h * 3), conf (w * h): in/out, or null.  labelsOut (w * h): out, or null -- the canonical label of
// every pixel as BEFORE the removal, -1 where the depth is not valid.  Counters are added to r (error stays as it is).
inline void speckle_host(int w, int h, float* depth, float* normal, float* conf, int32_t* labelsOut, float thr, uint32_t speckleSize, SpeckleResult& r) {
	const size_t n = (size_t)w * (size_t)h;
	std::vector<int32_t> own;
	if (!labelsOut) { own.resize(n); labelsOut = own.data(); }
	for (size_t i = 0; i < n; ++i) labelsOut[i] = -1;
	std::vector<int32_t> stack, members;
	for (size_t seed = 0; seed < n; ++seed) {
		if (labelsOut[seed] >= 0 || !speckle_valid(depth[seed])) continue;
		const int32_t label = (int32_t)seed;
		labelsOut[seed] = label;
		stack.assign(1, label);
		members.clear();
		while (!stack.empty()) {
			const int32_t p = stack.back();
			stack.pop_back();
			members.push_back(p);
			const int x = p % w, y = p / w;
			const float dp = depth[p];
			const int32_t nb[4] = {x > 0 ? p - 1 : -1, x + 1 < w ? p + 1 : -1, y > 0 ? p - w : -1, y + 1 < h ? p + w : -1};
			for (int k = 0; k < 4; ++k) {
				const int32_t q = nb[k];
				if (q < 0 || labelsOut[q] >= 0) continue;
				const float dq = depth[q];
				if (!speckle_valid(dq) || !speckle_joined(dp, dq, thr)) continue;
				labelsOut[q] = label;
				stack.push_back(q);
			}
		}
		const uint32_t size = (uint32_t)members.size();
		r.valid += size; r.segments += 1;
		if (size > r.largest) r.largest = size;
		if (size >= speckleSize) continue;
		r.small += 1; r.removed += size;
		for (const int32_t p : members) {
			depth[p] = 0.f;
			if (normal) { normal[3 * (size_t)p] = 0.f; normal[3 * (size_t)p + 1] = 0.f; normal[3 * (size_t)p + 2] = 0.f; }
			if (conf) conf[p] = 0.f;
		}
	}
}

} // namespace hcmvs
#endif

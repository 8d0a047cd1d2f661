/* hc-mvs_amd/csrc/handoff_plan.h -- what a hand-off call (hcmvs_handoff_maps, hcmvs_handoff_maps_device) refuses before any work, and the
 * launch plan of the device form: plain C++ (no HIP).  One launch serves all items; a workgroup of kHandoffBlock threads owns
 * kHandoffChunk consecutive destination pixels (raster order) of one item and finds the item in the prefix table `first`. */
#ifndef HCMVS_HANDOFF_PLAN_H
#define HCMVS_HANDOFF_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <cstdio>
#include <string>
#include <vector>
#include "carve.h"
#include "handoff_device.h"
namespace hcmvs {

constexpr int kHandoffBlock = 256;
constexpr int kHandoffChunk = 2048;                 // destination pixels of a workgroup: eight per thread
constexpr int kHandoffMaxItems = 64;                 // HCMVS_MAX_BATCH
constexpr int64_t kHandoffMaxPixels = (int64_t)1 << 29; // a map has fewer pixels than this (its normal map stays below 2^31 floats)

// one item as the checks see it: addresses as integers (host or device, the checks do not read them)
struct HandoffArgs {
	uintptr_t srcDepth, srcNormal, dstDepth, dstNormal;
	int32_t sw, sh, dw, dh;
	float dMin, dMax; // hint mode: the range taken in
};

inline bool handoff_overlap(uintptr_t a, uint64_t aBytes, uintptr_t b, uint64_t bBytes) { return a < b + bBytes && b < a + aBytes; }

// Empty string: the call may run.  Otherwise the reason it is refused (nothing has been read or written).
inline std::string handoff_check(const HandoffArgs* it, int n, int mode) {
	char buf[160];
	if (mode != kHandoffInit && mode != kHandoffHint) { snprintf(buf, sizeof buf, "unknown mode %d", mode); return buf; }
	if (!it) return "null items";
	if (n < 1 || n > kHandoffMaxItems) { snprintf(buf, sizeof buf, "n_items %d outside 1..%d", n, kHandoffMaxItems); return buf; }
	for (int i = 0; i < n; ++i) {
		const HandoffArgs& a = it[i];
		if (!a.srcDepth || !a.srcNormal || !a.dstDepth || !a.dstNormal) { snprintf(buf, sizeof buf, "item %d: null pointer", i); return buf; }
		if (a.sw < 1 || a.sh < 1 || a.dw < 1 || a.dh < 1) { snprintf(buf, sizeof buf, "item %d: size below 1 (%dx%d -> %dx%d)", i, a.sw, a.sh, a.dw, a.dh); return buf; }
		if ((int64_t)a.sw * a.sh >= kHandoffMaxPixels || (int64_t)a.dw * a.dh >= kHandoffMaxPixels) {
			snprintf(buf, sizeof buf, "item %d: a map of 2^29 pixels or more (%dx%d -> %dx%d)", i, a.sw, a.sh, a.dw, a.dh);
			return buf;
		}
		if (mode == kHandoffHint && (a.dw < a.sw || a.dh < a.sh)) {
			snprintf(buf, sizeof buf, "item %d: a hint is enlarged, never shrunk (%dx%d -> %dx%d)", i, a.sw, a.sh, a.dw, a.dh);
			return buf;
		}
		if (mode == kHandoffHint && (a.dMin != a.dMin || a.dMax != a.dMax)) { snprintf(buf, sizeof buf, "item %d: the range taken in is NaN", i); return buf; }
	}
	// a destination may share no byte with a source or with another destination, its own item's included (in place is not supported)
	struct Span { uintptr_t p; uint64_t bytes; int item; bool dst; const char* what; };
	std::vector<Span> spans;
	for (int i = 0; i < n; ++i) {
		const uint64_t s = (uint64_t)it[i].sw * it[i].sh, d = (uint64_t)it[i].dw * it[i].dh;
		spans.push_back({it[i].srcDepth, s * 4, i, false, "source depth"});
		spans.push_back({it[i].srcNormal, s * 12, i, false, "source normal"});
		spans.push_back({it[i].dstDepth, d * 4, i, true, "destination depth"});
		spans.push_back({it[i].dstNormal, d * 12, i, true, "destination normal"});
	}
	for (size_t a = 0; a < spans.size(); ++a) {
		if (!spans[a].dst) continue;
		for (size_t b = 0; b < spans.size(); ++b) {
			if (a == b || (spans[b].dst && b < a)) continue; // a pair of destinations is looked at once
			if (handoff_overlap(spans[a].p, spans[a].bytes, spans[b].p, spans[b].bytes)) {
				snprintf(buf, sizeof buf, "the %s of item %d overlaps the %s of item %d", spans[a].what, spans[a].item, spans[b].what, spans[b].item);
				return buf;
			}
		}
	}
	return std::string();
}

// first[i] .. first[i + 1]: the workgroups of item i; first[n] is the grid
inline std::vector<int32_t> handoff_first(const HandoffArgs* it, int n) {
	std::vector<int32_t> first((size_t)n + 1, 0);
	for (int i = 0; i < n; ++i) {
		const int64_t px = (int64_t)it[i].dw * it[i].dh;
		first[(size_t)i + 1] = first[(size_t)i] + (int32_t)((px + kHandoffChunk - 1) / kHandoffChunk); // < 2^18 each, 64 items: < 2^24
	}
	return first;
}

// one item as the kernels read it
struct HandoffItem {
	const float *srcDepth, *srcNormal;
	float *dstDepth, *dstNormal;
	HandoffGeom g;
};

// the one device buffer of a call: the result slots, the items, the prefix table (these three travel through the page-locked staging),
// then one partial result per workgroup, which never leaves the device
struct HandoffLayout {
	size_t results = 0, items = 0, first = 0, staged = 0, partials = 0, bytes = 0;
};
inline HandoffLayout handoff_layout(int n, size_t nBlocks) {
	Carve cv;
	HandoffLayout l;
	l.results = cv((size_t)n * sizeof(HandoffResult));
	l.items = cv((size_t)n * sizeof(HandoffItem));
	l.first = cv(((size_t)n + 1) * sizeof(int32_t));
	l.staged = cv.size;
	l.partials = cv(nBlocks * sizeof(HandoffResult));
	l.bytes = cv.size;
	return l;
}

} // namespace hcmvs
#endif

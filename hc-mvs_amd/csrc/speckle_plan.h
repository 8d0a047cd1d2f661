/* hc-mvs_amd/csrc/speckle_plan.h -- what a speckle-filter call (hcmvs_remove_speckles, hcmvs_remove_speckles_batch_device) refuses before
 * any work, the tile table of the device form and the layout of its one scratch buffer: plain C++ (no HIP).  The rule is DESIGN.md
 * section 5, D15.  One set of launches serves all maps of a batch: a workgroup owns one kSpeckleTileW x kSpeckleTileH tile of one map and
 * finds the map by bisection in the prefix table `first` of tile counts. */
#ifndef HCMVS_SPECKLE_PLAN_H
#define HCMVS_SPECKLE_PLAN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <cstdio>
#include <string>
#include <vector>
#include "carve.h"
namespace hcmvs {

constexpr int kSpeckleTileW = 64;                        // a wave is one row of a tile
constexpr int kSpeckleTileH = 16;
constexpr int kSpeckleBlock = 256;                       // four pixels of a tile per thread
constexpr int kSpeckleMaxItems = 64;                     // HCMVS_MAX_BATCH
constexpr int64_t kSpeckleMaxPixels = (int64_t)1 << 31;  // a map has fewer pixels than this: a label is a raster index in an int32_t
constexpr size_t kSpeckleScratchPerPixel = 8;            // a label and a size, int32_t each

// upstream's fDepthDiffThreshold * 0.7f, the product taken in float
inline float speckle_default_threshold() { return 0.01f * 0.7f; }

#if defined(__HIPCC__)
#define HCMVS_SPECKLE_FN __host__ __device__ __forceinline__
#else
#define HCMVS_SPECKLE_FN inline
#endif
// The rule, shared by the host form and the kernels (both are built with -ffp-contract=off; there is nothing to fuse anyway).
HCMVS_SPECKLE_FN bool speckle_valid(float d) { return d > 0.f; } // a NaN is not
// two valid 4-neighbours are joined when each is similar to the other as seen from itself (IsDepthSimilar both ways); an infinite
// depth gives inf / inf or inf / d: NaN or inf, never below thr
HCMVS_SPECKLE_FN bool speckle_joined(float dp, float dq, float thr) {
	const float diff = fabsf(dp - dq);
	return diff / dp < thr && diff / dq < thr;
}

// one map as the checks see it: addresses as integers (host or device, the checks do not read them); 0 = not given
struct SpeckleArgs {
	uintptr_t depth, normal, conf, labels;
	int32_t w, h;
};

inline bool speckle_overlap(uintptr_t a, uint64_t aBytes, uintptr_t b, uint64_t bBytes) { return a < b + bBytes && b < a + aBytes; }

// Empty string: the call may run.  Otherwise the reason it is refused (nothing has been read or written).
inline std::string speckle_check(const SpeckleArgs* it, int n, float thr) {
	char buf[160];
	if (!it) return "null items";
	if (n < 1 || n > kSpeckleMaxItems) { snprintf(buf, sizeof buf, "n_items %d outside 1..%d", n, kSpeckleMaxItems); return buf; }
	if (!(thr > 0.f) || !(thr <= 3.402823466e+38f)) { snprintf(buf, sizeof buf, "depth_diff_threshold %g is not a finite number > 0", (double)thr); return buf; }
	for (int i = 0; i < n; ++i) {
		const SpeckleArgs& a = it[i];
		if (a.w < 1 || a.h < 1) { snprintf(buf, sizeof buf, "item %d: size below 1 (%dx%d)", i, a.w, a.h); return buf; }
		if ((int64_t)a.w * a.h >= kSpeckleMaxPixels) { snprintf(buf, sizeof buf, "item %d: a map of 2^31 pixels or more (%dx%d)", i, a.w, a.h); return buf; }
		if (!a.depth) { snprintf(buf, sizeof buf, "item %d: null depth", i); return buf; }
	}
	// every buffer of the call is written (or may be): no two of them may share a byte
	struct Span { uintptr_t p; uint64_t bytes; int item; const char* what; };
	std::vector<Span> spans;
	for (int i = 0; i < n; ++i) {
		const uint64_t px = (uint64_t)it[i].w * it[i].h;
		spans.push_back({it[i].depth, px * 4, i, "depth"});
		if (it[i].normal) spans.push_back({it[i].normal, px * 12, i, "normal"});
		if (it[i].conf) spans.push_back({it[i].conf, px * 4, i, "conf"});
		if (it[i].labels) spans.push_back({it[i].labels, px * 4, i, "labels"});
	}
	for (size_t a = 0; a < spans.size(); ++a)
		for (size_t b = a + 1; b < spans.size(); ++b)
			if (speckle_overlap(spans[a].p, spans[a].bytes, spans[b].p, spans[b].bytes)) {
				snprintf(buf, sizeof buf, "the %s of item %d overlaps the %s of item %d", spans[a].what, spans[a].item, spans[b].what, spans[b].item);
				return buf;
			}
	return std::string();
}

inline int speckle_tiles_x(int w) { return (w + kSpeckleTileW - 1) / kSpeckleTileW; }
inline int speckle_tiles_y(int h) { return (h + kSpeckleTileH - 1) / kSpeckleTileH; }

// The tile table.  first[i] .. first[i + 1]: the tiles (workgroups) of item i, row-major over the item's grid of tiles; first[n] is
// the launch grid.  pixel0[i]: where the item's labels and sizes start in the scratch, in pixels; pixel0[n] is the batch's pixel count.
struct SpeckleTiles {
	std::vector<int64_t> first, pixel0;
};
inline SpeckleTiles speckle_tiles(const SpeckleArgs* it, int n) {
	SpeckleTiles t;
	t.first.assign((size_t)n + 1, 0); t.pixel0.assign((size_t)n + 1, 0);
	for (int i = 0; i < n; ++i) {
		t.first[(size_t)i + 1] = t.first[(size_t)i] + (int64_t)speckle_tiles_x(it[i].w) * speckle_tiles_y(it[i].h);
		t.pixel0[(size_t)i + 1] = t.pixel0[(size_t)i] + (int64_t)it[i].w * it[i].h;
	}
	return t;
}
// a grid is an unsigned 32-bit count of workgroups, and a tile index an int32_t in the kernels
inline bool speckle_grid_fits(const SpeckleTiles& t) { return t.first.back() < ((int64_t)1 << 31); }

// one map as the kernels read it
struct SpeckleItem {
	float *depth, *normal, *conf; // normal, conf: null = not given
	int32_t* outLabels;           // null = not wanted
	int32_t *labels, *sizes;      // the item's part of the scratch
	int32_t w, h, tilesX, pad;
};

// what a tile adds to the call's counters; summed by the last launch
struct SpecklePartial {
	uint32_t valid, removed, segments, small, largest, pad;
};
// the counters of a call and its error word as they come back
struct SpeckleResult {
	uint64_t valid, removed, segments, small;
	uint32_t largest, error; // error: a union or find loop ran past its bound (never expected)
};

// the one device buffer of a call: the result, the items and the prefix table (these travel through the page-locked staging), one partial
// per tile, then 8 B per pixel of the batch: the labels of all items, then their sizes
struct SpeckleLayout {
	size_t result = 0, items = 0, first = 0, staged = 0, partials = 0, labels = 0, sizes = 0, bytes = 0;
};
inline SpeckleLayout speckle_layout(int n, size_t nTiles, size_t nPixels) {
	Carve cv;
	SpeckleLayout l;
	l.result = cv(sizeof(SpeckleResult));
	l.items = cv((size_t)n * sizeof(SpeckleItem));
	l.first = cv(((size_t)n + 1) * sizeof(int32_t));
	l.staged = cv.size;
	l.partials = cv(nTiles * sizeof(SpecklePartial));
	l.labels = cv(nPixels * (kSpeckleScratchPerPixel / 2));
	l.sizes = cv(nPixels * (kSpeckleScratchPerPixel / 2));
	l.bytes = cv.size;
	return l;
}

} // namespace hcmvs
#endif

/*
 * hc-mvs_amd/csrc/pm_types.h -- the constants and the structures of an estimate that the host fills and the gfx950 kernels read.
 * Plain C++ without a HIP header, so that est_plan.h fills them on a CPU (tests/test_est_plan.py); the kernels and the host API
 * take them through pm_common.h.
 */
#ifndef HCMVS_PM_TYPES_H
#define HCMVS_PM_TYPES_H

#include <stdint.h>

namespace hcmvs {

// The one HIP type among the members below: HIP's float4 where the compiler knows it (pm_common.h includes the runtime header first),
// an opaque type to every other compiler -- a pointer either way, so the layouts agree
#ifdef __HIPCC__
using DnTexel = ::float4;
#else
struct DnTexel;
#endif

constexpr int kHalfWindow = 7;      // nSizeHalfWindow, DepthMap.h:354 (fixed border, DepthMap.cpp:442-447)
// The reference fixes nSizeHalfWindow = 7 / nTexels = 64 at compile time (DepthMap.h:354-358).  Patches beyond that
// (BASELINE.json configs[4]: 11 x 11 taps, adapthalfwin 10) generalise the two constants: the border every pass keeps
// clear follows the half window, EstConst::border = max(7, adapthalfwin).
constexpr int kMaxHalfWindow = 10;
constexpr int kBigTaps = (kMaxHalfWindow + 1) * (kMaxHalfWindow + 1); // 121
constexpr int kBigSlots = 128;      // tap slots of the big-patch tables (taps dealt round-robin to the lanes of a view group)
constexpr int kMaxViews = 16;
constexpr int kMaxSlots = 32;       // neighbour slots of one pixel (cross pattern: 4 * ceil(halfwin/step))
constexpr int kProgressStride = 16; // ints between the progress words of consecutive rows (64 B)

// per source view constants, one lane group reads its own view's entry (DepthMap.h:412-444 ViewData)
struct DevView {
	uint32_t byteOff; // start of the view's footprint image (launch_quads) relative to EstConst::imgBase
	int32_t w, h;
	float A[9];  // Hl * Hr = Kj Rj Ri^T Ki^-1 (computed in double on the host, held as float)
	float Hm[3]; // Kj Rj (Ci - Cj)
};

// --n-viewspread (DepthMap.cpp:1504-1608): what a sweep worker needs of one source view j whose own maps are offered as hypotheses.
// depth == null: the view offers none.  The maps have the view's image size.
struct SpreadView {
	const float* depth;     // w * h
	const float* normal;    // w * h * 3, view j's camera frame
	const float* conf;      // w * h
	int32_t w, h;
	double cx, cy, ifx, ify; // view j's principal point and 1 / focal
	double Tz[3], tz;        // third row of R_ref R_j^T and of R_ref (C_j - C_ref): depth in the reference camera of a point of view j's
};

// uniform constants of one EstimateDepthMap call (DepthMap.cpp:386-439 DepthEstimator ctor)
struct EstConst {
	int32_t W, H, V;
	int32_t border;         // max(kHalfWindow, adapthalfwin): pixels closer than this to an edge are not estimated
	int32_t adapthalfwin, nRandomIters, itExternal, propHalfwin, propStep;
	const float* ref;
	const uint8_t* gra;
	const DevView* views;
	const char* imgBase;    // lowest source footprint-image address of this call (32-bit offsets from here)
	float Hr[9];            // Ki^-1 (double on the host, held as float)
	double cx, cy, ifx, ify; // reference principal point and 1/focal (Camera.h:299-312)
	float dMin, dMax, dMinSqr, dMaxSqr;
	float smoothBonusDepth, smoothBonusNormal, smoothSigmaDepth, smoothSigmaNormal;
	float angle1Range, angle2Range;
	float thConfSmall, thConfBig, thConfRand, thRobust, thKeep;
	float depthRatio, pfScale;
	uint32_t seed;
	// working state: (depth, nx, ny, nz) per pixel + score per pixel
	DnTexel* dn;
	float* conf;
	int32_t* progress; // [rows * kProgressStride] pixels finished per logical row of this image (sweeps)
	// restore-variant extra hypothesis (restore/libs/MVS/DepthMap.cpp:1527-1549): in sweep number hintIter every pixel also tries
	// the estimate of the up-sampled coarser level, with a 0.1 bonus; null / -1 when not in use
	const float* hintDepth;
	const float* hintNormal;
	int32_t hintIter;
	// --ignore-mask-label (DepthMap.cpp:319-381): per pixel 1 = estimated, 0 = ignored (left out of the visiting order of every pass:
	// the pixel keeps what ApplyIgnoreMask and the median left it); null when the reference view has no mask
	const uint8_t* keep;
	// view spread (SPREAD instances of the sweep): [V] entries in the estimate's view order; null when the call has it off, at outer
	// iteration 0 or when no source view of the item offers maps
	const SpreadView* spread;
};

// Depth prior of one item (PRIOR instances of the kernels; DepthMap.cpp:941-954).  EstConst keeps its layout: the entry lives behind the
// item's DevView table -- EstConst::views points at kViewSlotEntries entries, kMaxViews views and then this (prior_item()); only the
// PRIOR instances ever look there.
struct PriorItem {
	const float* prior;   // the reference view's prior depth map, W * H, read and never written; null: the item has no active prior
	float keep, para, sigma; // 1 - para_prior, para_prior, -1 / (2 sigma_prior^2)
	int32_t countIter;    // the sweep index in which the pixels with a usable prior are counted; -1: the init-score pass counts them
};
constexpr int kViewSlotEntries = kMaxViews + 2; // DevView entries per item of the table EstConst::views points into
static_assert(sizeof(PriorItem) <= 2 * sizeof(DevView) && (kMaxViews * sizeof(DevView)) % 8 == 0 && (kViewSlotEntries * sizeof(DevView)) % 8 == 0,
              "the PriorItem behind an item's views must be 8-byte aligned in every slot");
inline const PriorItem* prior_item(const DevView* views) { return (const PriorItem*)(const void*)(views + kMaxViews); }
inline PriorItem* prior_item(DevView* views) { return (PriorItem*)(void*)(views + kMaxViews); }

// Geometric consistency (GEO instances of the kernels): what a lane needs of one source view j whose own maps
// of the previous outer iteration score a hypothesis.  depth == null: the view offers none.  The maps have the view's image size and are
// the ones registered with hcmvs_set_spread_maps_device.  Everything is held as float: computed in double on the host, rounded once.
struct GeoView {
	const float* depth;   // w * h
	const float* normal;  // w * h * 3, view j's camera frame
	int32_t w, h;
	float cx, cy, ifx, ify; // view j's principal point and 1 / focal
	float B[9];           // K_i R_i R_j^T: a point of view j's camera into the reference image (homogeneous)
	float b[3];           // K_i R_i (C_j - C_i)
	float Rr[9];          // R_i R_j^T: a normal of view j's camera frame into the reference camera's
	int32_t pad;
};
// The term's constants of one item, behind the item's PriorItem in the slot of the DevView table (geo_item()); only the GEO instances
// ever look there.  views == null: the term is not active for the item.
struct GeoItem {
	const GeoView* views; // [V] entries in the estimate's view order
	float w1, w2;         // para_tapa, para_tapa2
	float keep1, keep2;   // 1 - para_tapa, 1 - para_tapa2, rounded once
	float tx1, tx2;       // txthreshold, txthreshold2
	float maxPx;          // the reprojection error at and beyond which a pair is "worst"
	int32_t countIter;    // the sweep index in which the pixels with a weight are counted; -1: the init-score pass counts them
};
static_assert(sizeof(PriorItem) % 8 == 0 && sizeof(PriorItem) + sizeof(GeoItem) <= 2 * sizeof(DevView) && sizeof(GeoView) % 8 == 0,
              "the GeoItem behind an item's PriorItem must fit the slot and be 8-byte aligned");
inline const GeoItem* geo_item(const DevView* views) { return (const GeoItem*)(const void*)((const char*)prior_item(views) + sizeof(PriorItem)); }
inline GeoItem* geo_item(DevView* views) { return (GeoItem*)(void*)((char*)prior_item(views) + sizeof(PriorItem)); }


} // namespace hcmvs
#endif

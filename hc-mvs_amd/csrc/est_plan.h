/* hc-mvs_amd/csrc/est_plan.h -- the host-side arithmetic of an estimate call: what a batch is refused for, the constants of an item the way
 * DepthEstimator's constructor derives them (DepthMap.cpp:386-439, DepthMap.h:412-444), the 4 GiB window of an item's source images and
 * the aliasing rule of view spread.  Pure functions of cameras, parameters, sizes and addresses in plain C++ (no HIP), so that
 * tests/test_est_plan.py checks them without a GPU, the constants bit for bit against the oracle's own derivation; hcmvs_api.cpp adds the
 * device pointers.  Everything is written into storage of the caller's: nothing here allocates. */
#ifndef HCMVS_EST_PLAN_H
#define HCMVS_EST_PLAN_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/hcmvs_hip.h"
#include "carve.h"
#include "pm_types.h"
#include "sweep_plan.h"
namespace hcmvs {

inline float fd2r(float d) { return d * (3.14159274101257324f / 180.f); }

inline void mat3_mul(const double* a, const double* b, double* c) {
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double s = 0;
			for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
			c[i * 3 + j] = s;
		}
}
inline void mat3_mul_bt(const double* a, const double* b, double* c) {
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j) {
			double s = 0;
			for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[j * 3 + k];
			c[i * 3 + j] = s;
		}
}
inline void mat3_inv(const double* m, double* r) {
	const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
	                 m[2] * (m[3] * m[7] - m[4] * m[6]);
	const double id = 1.0 / d;
	r[0] = (m[4] * m[8] - m[5] * m[7]) * id;
	r[1] = (m[2] * m[7] - m[1] * m[8]) * id;
	r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
	r[3] = (m[5] * m[6] - m[3] * m[8]) * id;
	r[4] = (m[0] * m[8] - m[2] * m[6]) * id;
	r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
	r[6] = (m[3] * m[7] - m[4] * m[6]) * id;
	r[7] = (m[1] * m[6] - m[0] * m[7]) * id;
	r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// a registered view as the plan sees it: x_cam = R (X - C), pixel = K x_cam / z
struct EstCamera {
	const double *K, *R, *C;
	int w, h;
};

// ---- what an estimate call is refused for ----
enum EstBad {
	kEstOk = 0,
	kEstBatchSize,  // not 1 .. HCMVS_MAX_BATCH items
	kEstHalfWindow, // adapthalfwin not in 1 .. kMaxHalfWindow
	kEstIterCounts, // a negative count, or more than 20 random iterations
	kEstSrcCount,   // item `at`: n_src not in 1 .. kMaxViews
	kEstSrcClass,   // item `at`: not the source-count class (1-8 or 9-16) of item 0
	kEstNull,       // item `at`: no source ids or no in/out maps
	kEstDepthRange, // item `at`: not 0 <= d_min < d_max
	kEstBorder,     // item `at`: its reference image has no pixel inside the border
	kEstPriorHint,  // item `at` has the `restore` hint in effect while an item of the batch has an active depth prior
	kEstPriorSpread, // item `at` has view spread doing work while an item of the batch has an active depth prior
	kEstSweepRange, // sweeps-only call: first_sweep < 0, n_sweeps < 1 or an index beyond HCMVS_MAX_SWEEP_INDEX
	kEstGeoHint,    // item `at` has the `restore` hint in effect while the geometric-consistency term is active for an item of the batch
	kEstGeoSpread,  // item `at` has view spread doing work while the term is active for an item of the batch
	kEstGeoPrior    // item `at` has an active depth prior while the term is active for an item of the batch
};
struct EstCheck {
	EstBad broken = kEstOk;
	int at = -1; // the item that broke the rule; -1: the call as a whole
};
// the call as a whole, before any item is looked at
inline EstCheck est_check_call(int nItems, const hcmvs_params& p) {
	if (nItems < 1 || nItems > HCMVS_MAX_BATCH) return {kEstBatchSize, -1};
	if (p.adapthalfwin < 1 || p.adapthalfwin > kMaxHalfWindow) return {kEstHalfWindow, -1};
	if (p.n_estimation_iters < 0 || p.n_random_iters < 0 || p.n_random_iters > 20) return {kEstIterCounts, -1};
	return {};
}
// item i of the batch, before its views are looked up.  d_min == 0 is what the `restore` variant ends up with (its range takes the
// enlarged previous-level map in, zeros included, restore/libs/MVS/SceneDensify.cpp:526-532)
inline EstCheck est_check_item(const hcmvs_batch_item* items, int i) {
	const hcmvs_batch_item& it = items[i];
	if (it.n_src < 1 || it.n_src > kMaxViews) return {kEstSrcCount, i};
	if (segments_for(it.n_src) != segments_for(items[0].n_src)) return {kEstSrcClass, i};
	if (!it.src_ids || !it.d_depth || !it.d_normal || !it.d_conf) return {kEstNull, i};
	if (!(it.d_min >= 0.f) || !(it.d_max > it.d_min)) return {kEstDepthRange, i};
	return {};
}
// nSizeHalfWindow generalised (pm_types.h): pixels closer than this to an edge are not estimated
inline int est_border(const hcmvs_params& p) { return p.adapthalfwin > kHalfWindow ? p.adapthalfwin : kHalfWindow; }
// item i's reference image of w x h against the border
inline EstCheck est_check_image(int i, int w, int h, const hcmvs_params& p) {
	const int b = est_border(p);
	if (w < 2 * b + 2 || h < 2 * b + 2) return {kEstBorder, i};
	return {};
}

// ---- the constants of one item ----
// the `restore` variant's extra hypothesis is tried in the last sweep of the last outer iteration (restore/libs/MVS/DepthMap.cpp:1527)
inline bool est_uses_hint(const hcmvs_params& p, bool offered) { return offered && p.it_external == p.n_external_iters - 1; }

// Every value member of k and of dv[kMaxViews] (the entries from nSrc on are zero); the pointer members are left null and
// dv[v].byteOff zero (est_image_window).  Hr = K_i^-1, A = (K_j R_j R_i^T) Hr and Hm = K_j R_j (C_i - C_j) are computed in double and
// rounded once.
inline void est_item_consts(const EstCamera& ref, const EstCamera* src, int nSrc, const hcmvs_params& p, float dMin, float dMax, uint32_t seedOffset,
                            bool hintOffered, EstConst& k, DevView* dv) {
	memset(&k, 0, sizeof k);
	k.W = ref.w; k.H = ref.h; k.V = nSrc;
	k.border = est_border(p);
	k.adapthalfwin = p.adapthalfwin; k.nRandomIters = p.n_random_iters; k.itExternal = p.it_external;
	k.propHalfwin = p.propagate_halfwin; k.propStep = p.propagate_step;
	double Hr[9];
	mat3_inv(ref.K, Hr);
	for (int i = 0; i < 9; ++i) k.Hr[i] = (float)Hr[i];
	k.ifx = 1.0 / ref.K[0]; k.ify = 1.0 / ref.K[4]; k.cx = ref.K[2]; k.cy = ref.K[5];
	memset(dv, 0, sizeof(DevView) * kMaxViews);
	for (int v = 0; v < nSrc; ++v) {
		const EstCamera& s = src[v];
		double KR[9], Hl[9], A[9];
		mat3_mul(s.K, s.R, KR);
		mat3_mul_bt(KR, ref.R, Hl);
		const double dC[3] = {ref.C[0] - s.C[0], ref.C[1] - s.C[1], ref.C[2] - s.C[2]};
		for (int i = 0; i < 3; ++i) dv[v].Hm[i] = (float)(KR[i * 3] * dC[0] + KR[i * 3 + 1] * dC[1] + KR[i * 3 + 2] * dC[2]);
		mat3_mul(Hl, Hr, A);
		for (int i = 0; i < 9; ++i) dv[v].A[i] = (float)A[i];
		dv[v].w = s.w; dv[v].h = s.h;
	}
	k.dMin = dMin; k.dMax = dMax; k.dMinSqr = sqrtf(dMin); k.dMaxSqr = sqrtf(dMax);
	k.smoothBonusDepth = 1.f - p.random_smooth_bonus;
	k.smoothBonusNormal = (1.f - p.random_smooth_bonus) * 0.96f;
	k.smoothSigmaDepth = -1.f / (2.f * (p.random_smooth_depth * p.random_smooth_depth));
	{ const float r = fd2r(p.random_smooth_normal_deg); k.smoothSigmaNormal = -1.f / (2.f * (r * r)); }
	k.angle1Range = fd2r(p.random_angle1_deg);
	k.angle2Range = fd2r(p.random_angle2_deg);
	k.thConfSmall = p.ncc_threshold_keep * 0.2f;
	k.thConfBig = p.ncc_threshold_keep * 0.4f;
	k.thConfRand = p.ncc_threshold_keep * 0.9f;
	k.thRobust = p.ncc_threshold_keep * 1.2f;
	k.thKeep = p.ncc_threshold_keep;
	k.depthRatio = p.random_depth_ratio;
	k.pfScale = 1.f - p.photometric_flow;
	k.seed = p.seed + seedOffset;
	k.hintIter = est_uses_hint(p, hintOffered) ? p.n_estimation_iters - 1 : -1;
}

// --n-viewspread (DepthMap.cpp:1504-1608): from outer iteration 1 on, a source view that offers maps of its own size spreads
inline bool est_view_spreads(bool viewspread, const hcmvs_params& p, bool offersMaps, bool rescaled) {
	return viewspread && p.it_external >= 1 && offersMaps && !rescaled;
}
// the value members of source view s's entry.  Depth in the reference camera of a point Xc of view j's camera:
// (R_ref R_j^T Xc + R_ref (C_j - C_ref)).z
inline void est_spread_consts(const EstCamera& ref, const EstCamera& s, SpreadView& sv) {
	sv.w = s.w; sv.h = s.h;
	sv.cx = s.K[2]; sv.cy = s.K[5]; sv.ifx = 1.0 / s.K[0]; sv.ify = 1.0 / s.K[4];
	double T[9];
	mat3_mul_bt(ref.R, s.R, T);
	const double dC[3] = {s.C[0] - ref.C[0], s.C[1] - ref.C[1], s.C[2] - ref.C[2]};
	sv.Tz[0] = T[6]; sv.Tz[1] = T[7]; sv.Tz[2] = T[8];
	sv.tz = ref.R[6] * dC[0] + ref.R[7] * dC[1] + ref.R[8] * dC[2];
}

// what plan_sweeps needs of an item whose constants and pointers are set
inline SweepItem est_sweep_item(const EstConst& k, int nSweeps, bool prior = false, bool geo = false) {
	return {k.H - 2 * k.border, k.W - 2 * k.border, k.V, k.hintDepth && k.hintIter == nSweeps - 1, k.keep != nullptr, k.spread != nullptr, prior, geo};
}

// ---- the image window ----
// The scorer reaches a source view's footprint image by a 32-bit offset from one scalar base, so the images of one item must lie
// within a 4 GiB window.  Where the caller's are further apart they are first copied into a compact slab, each at the offset Carve gives
// it in view order; a slab that itself reaches the limit is refused.
constexpr uint64_t kEstWindowLimit = 0xFFFF0000ull;
enum EstWindowKind { kEstWindowDirect, kEstWindowSlab, kEstWindowRefused };
struct EstWindow {
	EstWindowKind kind;
	uint64_t base;    // kEstWindowDirect: the lowest address
	size_t slabBytes; // kEstWindowSlab, kEstWindowRefused: what the slab needs
};
// addr[v], bytes[v]: where source view v's image lies and its size; off[v]: its offset from the base, or in the slab
inline EstWindow est_image_window(const uint64_t* addr, const size_t* bytes, int n, uint32_t* off) {
	uint64_t lo = ~(uint64_t)0, hi = 0;
	for (int v = 0; v < n; ++v) {
		if (addr[v] < lo) lo = addr[v];
		if (addr[v] + bytes[v] > hi) hi = addr[v] + bytes[v];
	}
	if (hi - lo < kEstWindowLimit) {
		for (int v = 0; v < n; ++v) off[v] = (uint32_t)(addr[v] - lo);
		return {kEstWindowDirect, lo, 0};
	}
	Carve slab;
	for (int v = 0; v < n; ++v) off[v] = (uint32_t)slab(bytes[v]);
	return {slab.size >= kEstWindowLimit ? kEstWindowRefused : kEstWindowSlab, 0, slab.size};
}

// ---- depth priors (DepthMap.cpp:941-954) ----
// what hcmvs_set_prior_params refuses: para_prior outside [0, 1] or not finite, sigma_prior not > 0 (or not finite), photo2geo < 0
enum PriorBad { kPriorOk = 0, kPriorPara, kPriorSigma, kPriorPhoto2geo };
inline PriorBad est_check_prior_params(const hcmvs_prior_params& pp) {
	if (!(pp.para_prior >= 0.f && pp.para_prior <= 1.f)) return kPriorPara; // (a NaN fails both comparisons)
	if (!(pp.sigma_prior > 0.f) || !(pp.sigma_prior < INFINITY)) return kPriorSigma;
	if (pp.photo2geo < 0) return kPriorPhoto2geo;
	return kPriorOk;
}
// the active-prior rule: a prior is registered for the reference view, the term has weight, and the outer iteration has reached photo2geo
inline bool est_prior_active(bool registered, const hcmvs_prior_params& pp, const hcmvs_params& p) {
	return registered && pp.para_prior > 0.f && p.it_external >= pp.photo2geo;
}
// the term's constants (PriorItem::prior itself is the caller's pointer): score * keep + (2 * (1 - exp(dd^2 * sigma))) * para.
// countIter: the sweep in which the pixels with a usable prior are counted; -1: the init-score pass counts them
inline void est_prior_consts(const hcmvs_prior_params& pp, int countIter, PriorItem& k) {
	k.keep = 1.f - pp.para_prior;
	k.para = pp.para_prior;
	k.sigma = -1.f / (2.f * (pp.sigma_prior * pp.sigma_prior));
	k.countIter = countIter;
}
// Per item of a batch: has an active prior, has the hint in effect (est_uses_hint), has view spread doing work (est_view_spreads of some
// source view).  A batch is one set of launches, so an active prior anywhere in it is refused together with a hint or with view spread
// at work anywhere in it; `at` is the first item with the hint (or, failing that, with view spread) that stands in the way.
inline EstCheck est_check_prior_batch(const bool* priorActive, const bool* hintInEffect, const bool* spreadWork, int nItems) {
	bool any = false;
	for (int i = 0; i < nItems; ++i) any = any || priorActive[i];
	if (!any) return {};
	for (int i = 0; i < nItems; ++i) if (hintInEffect[i]) return {kEstPriorHint, i};
	for (int i = 0; i < nItems; ++i) if (spreadWork[i]) return {kEstPriorSpread, i};
	return {};
}
// the sweeps-only call (hcmvs_estimate_sweeps_batch_device): a sweep's random stream is it_external * 64 + 1 + index, and stream
// (it_external + 1) * 64 is the next outer iteration's init-score pass, so an index has room up to HCMVS_MAX_SWEEP_INDEX = 62
inline EstCheck est_check_sweeps(int firstSweep, int nSweeps) {
	if (firstSweep < 0 || nSweeps < 1 || firstSweep > HCMVS_MAX_SWEEP_INDEX || nSweeps > HCMVS_MAX_SWEEP_INDEX + 1 - firstSweep) return {kEstSweepRange, -1};
	return {};
}

// ---- geometric consistency ----
// what hcmvs_set_geo_params refuses: a weight outside [0, 1] or not finite, a threshold that is not finite, max_px not finite and > 0,
// photo2geo < 0
enum GeoBad { kGeoOk = 0, kGeoWeight, kGeoThreshold, kGeoMaxPx, kGeoPhoto2geo };
inline GeoBad est_check_geo_params(const hcmvs_geo_params& gp) {
	if (!(gp.para_tapa >= 0.f && gp.para_tapa <= 1.f) || !(gp.para_tapa2 >= 0.f && gp.para_tapa2 <= 1.f)) return kGeoWeight; // (a NaN fails both comparisons)
	if (!(fabsf(gp.txthreshold) < INFINITY) || !(fabsf(gp.txthreshold2) < INFINITY)) return kGeoThreshold;
	if (!(gp.max_px > 0.f) || !(gp.max_px < INFINITY)) return kGeoMaxPx;
	if (gp.photo2geo < 0) return kGeoPhoto2geo;
	return kGeoOk;
}
// a source view offers maps to the term when it has some registered (hcmvs_set_spread_maps_device) and was not made by hcmvs_rescale_view
inline bool est_geo_offers(bool offersMaps, bool rescaled) { return offersMaps && !rescaled; }
// the activity rule: the switch is set, the outer iteration has reached photo2geo, and a source view of the item offers maps
inline bool est_geo_active(const hcmvs_geo_params& gp, const hcmvs_params& p, bool anyViewOffers) {
	return gp.on != 0 && p.it_external >= gp.photo2geo && anyViewOffers;
}
// The value members of source view s's entry (the map pointers are the caller's).  A point Xc of view j's camera lands in the reference
// image at B Xc + b (homogeneous) with B = K_i R_i R_j^T and b = K_i R_i (C_j - C_i); a normal of view j's camera frame is Rr = R_i R_j^T
// times it in the reference camera's.  Computed in double, rounded once.
inline void est_geo_view(const EstCamera& ref, const EstCamera& s, GeoView& gv) {
	gv.w = s.w; gv.h = s.h; gv.pad = 0;
	gv.cx = (float)s.K[2]; gv.cy = (float)s.K[5]; gv.ifx = (float)(1.0 / s.K[0]); gv.ify = (float)(1.0 / s.K[4]);
	double KR[9], B[9], Rr[9];
	mat3_mul(ref.K, ref.R, KR);
	mat3_mul_bt(KR, s.R, B);
	mat3_mul_bt(ref.R, s.R, Rr);
	const double dC[3] = {s.C[0] - ref.C[0], s.C[1] - ref.C[1], s.C[2] - ref.C[2]};
	for (int i = 0; i < 9; ++i) { gv.B[i] = (float)B[i]; gv.Rr[i] = (float)Rr[i]; }
	for (int i = 0; i < 3; ++i) gv.b[i] = (float)(KR[i * 3] * dC[0] + KR[i * 3 + 1] * dC[1] + KR[i * 3 + 2] * dC[2]);
}
// the term's constants of an item (GeoItem::views itself is the context's pointer).  countIter: as PriorItem::countIter
inline void est_geo_consts(const hcmvs_geo_params& gp, int countIter, GeoItem& k) {
	k.w1 = gp.para_tapa; k.w2 = gp.para_tapa2;
	k.keep1 = 1.f - gp.para_tapa; k.keep2 = 1.f - gp.para_tapa2;
	k.tx1 = gp.txthreshold; k.tx2 = gp.txthreshold2;
	k.maxPx = gp.max_px;
	k.countIter = countIter;
}
// Per item of a batch: has the term active, has the hint in effect, has view spread doing work, has an active depth prior.  A batch is
// one set of launches, so the term active anywhere in it is refused together with any of the three anywhere in it; `at` is the first
// item with the hint (or, failing that, with view spread, or, failing that, with a prior) that stands in the way.
inline EstCheck est_check_geo_batch(const bool* geoActive, const bool* hintInEffect, const bool* spreadWork, const bool* priorActive, int nItems) {
	bool any = false;
	for (int i = 0; i < nItems; ++i) any = any || geoActive[i];
	if (!any) return {};
	for (int i = 0; i < nItems; ++i) if (hintInEffect[i]) return {kEstGeoHint, i};
	for (int i = 0; i < nItems; ++i) if (spreadWork[i]) return {kEstGeoSpread, i};
	for (int i = 0; i < nItems; ++i) if (priorActive[i]) return {kEstGeoPrior, i};
	return {};
}

// ---- view spread: a launch must not read what it writes ----
// The in/out maps of no item may share a byte with the spread maps of a source view of any item (depth and conf: 4 bytes per pixel,
// normal: 12).  k, spread ([nItems][kMaxViews]) and items describe the batch as it is about to be launched; the first offender in
// (item, other item, source view of the other item) order, or item < 0.
struct EstOverlap {
	int item = -1, other = -1, view = -1;
};
inline bool est_ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
	const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
	return a0 < b0 + nb && b0 < a0 + na;
}
inline EstOverlap est_spread_overlap(const EstConst* k, const SpreadView* spread, const hcmvs_batch_item* items, int nItems) {
	for (int i = 0; i < nItems; ++i) {
		const size_t n = (size_t)k[i].W * k[i].H;
		const void* io[3] = {items[i].d_depth, items[i].d_normal, items[i].d_conf};
		const size_t ion[3] = {n * 4, n * 12, n * 4};
		for (int j = 0; j < nItems; ++j)
			for (int v = 0; v < items[j].n_src; ++v) {
				const SpreadView& sv = spread[(size_t)j * kMaxViews + v];
				if (!k[j].spread || !sv.depth) continue;
				const size_t m = (size_t)sv.w * sv.h;
				const void* sp[3] = {sv.depth, sv.normal, sv.conf};
				const size_t spn[3] = {m * 4, m * 12, m * 4};
				for (int a = 0; a < 3; ++a)
					for (int b = 0; b < 3; ++b)
						if (est_ranges_overlap(io[a], ion[a], sp[b], spn[b])) return {i, j, v};
			}
	}
	return {};
}
// the same rule for the maps the geometric-consistency term reads (depth and normal): geo is [nItems][kMaxViews], active[j] tells
// whether item j's term is active
inline EstOverlap est_geo_overlap(const EstConst* k, const GeoView* geo, const bool* active, const hcmvs_batch_item* items, int nItems) {
	for (int i = 0; i < nItems; ++i) {
		const size_t n = (size_t)k[i].W * k[i].H;
		const void* io[3] = {items[i].d_depth, items[i].d_normal, items[i].d_conf};
		const size_t ion[3] = {n * 4, n * 12, n * 4};
		for (int j = 0; j < nItems; ++j)
			for (int v = 0; v < items[j].n_src; ++v) {
				const GeoView& gv = geo[(size_t)j * kMaxViews + v];
				if (!active[j] || !gv.depth) continue;
				const size_t m = (size_t)gv.w * gv.h;
				const void* sp[2] = {gv.depth, gv.normal};
				const size_t spn[2] = {m * 4, m * 12};
				for (int a = 0; a < 3; ++a)
					for (int b = 0; b < 2; ++b)
						if (est_ranges_overlap(io[a], ion[a], sp[b], spn[b])) return {i, j, v};
			}
	}
	return {};
}

} // namespace hcmvs
#endif

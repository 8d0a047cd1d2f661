// C face of what the geometric-consistency term adds to hc-mvs_amd/csrc/est_plan.h and sweep_plan.h, for tests/test_geo_plan.py (ctypes).
// Links nothing of the library and nothing of HIP.
#include "../hc-mvs_amd/csrc/est_plan.h"

using namespace hcmvs;

extern "C" {

// ---- est_plan.h ----
// 0 ok, 1 weight, 2 threshold, 3 max_px, 4 photo2geo
int gp_check_params(float tapa, float tapa2, float tx, float tx2, int photo2geo, float maxPx) {
	const hcmvs_geo_params p = {1, tapa, tapa2, tx, tx2, photo2geo, maxPx};
	const GeoBad b = est_check_geo_params(p);
	return b == kGeoOk ? 0 : b == kGeoWeight ? 1 : b == kGeoThreshold ? 2 : b == kGeoMaxPx ? 3 : 4;
}
int gp_offers(int maps, int rescaled) { return est_geo_offers(maps != 0, rescaled != 0); }
int gp_active(int on, int photo2geo, int itExternal, int anyOffers) {
	hcmvs_geo_params gp = {on, 0.25f, 0.15f, 150.f, 160.f, photo2geo, 3.f};
	hcmvs_params p;
	memset(&p, 0, sizeof p);
	p.it_external = itExternal;
	return est_geo_active(gp, p, anyOffers != 0);
}
// cameras: K[9], R[9], C[3] of the reference and of the source view (doubles); out: w, h as floats, cx, cy, ifx, ify, B[9], b[3], Rr[9]
void gp_view(const double* ref, const double* src, int w, int h, float* out) {
	const EstCamera r = {ref, ref + 9, ref + 18, 0, 0}, s = {src, src + 9, src + 18, w, h};
	GeoView gv;
	memset(&gv, 0xff, sizeof gv);
	est_geo_view(r, s, gv);
	out[0] = (float)gv.w; out[1] = (float)gv.h; out[2] = gv.cx; out[3] = gv.cy; out[4] = gv.ifx; out[5] = gv.ify;
	memcpy(out + 6, gv.B, sizeof gv.B); memcpy(out + 15, gv.b, sizeof gv.b); memcpy(out + 18, gv.Rr, sizeof gv.Rr);
}
// out[7]: w1, w2, keep1, keep2, tx1, tx2, maxPx; returns countIter
int gp_consts(float tapa, float tapa2, float tx, float tx2, float maxPx, int countIter, float* out) {
	const hcmvs_geo_params gp = {1, tapa, tapa2, tx, tx2, 0, maxPx};
	GeoItem k;
	memset(&k, 0xff, sizeof k);
	est_geo_consts(gp, countIter, k);
	out[0] = k.w1; out[1] = k.w2; out[2] = k.keep1; out[3] = k.keep2; out[4] = k.tx1; out[5] = k.tx2; out[6] = k.maxPx;
	return k.countIter;
}
// flags: n x (term active, hint in effect, spread at work, prior active); returns 0 ok, 1 hint, 2 spread, 3 prior; *at: the item
int gp_check_batch(const int* flags, int n, int* at) {
	bool g[HCMVS_MAX_BATCH], h[HCMVS_MAX_BATCH], s[HCMVS_MAX_BATCH], p[HCMVS_MAX_BATCH];
	for (int i = 0; i < n; ++i) { g[i] = flags[4 * i] != 0; h[i] = flags[4 * i + 1] != 0; s[i] = flags[4 * i + 2] != 0; p[i] = flags[4 * i + 3] != 0; }
	const EstCheck c = est_check_geo_batch(g, h, s, p, n);
	*at = c.at;
	return c.broken == kEstOk ? 0 : c.broken == kEstGeoHint ? 1 : c.broken == kEstGeoSpread ? 2 : c.broken == kEstGeoPrior ? 3 : -1;
}
// sizes of EstConst, DevView, PriorItem, GeoItem, GeoView, entries per view slot; where the GeoItem of a slot lies and where the slot ends
void gp_layout(int* out) {
	out[0] = (int)sizeof(EstConst); out[1] = (int)sizeof(DevView); out[2] = (int)sizeof(PriorItem); out[3] = (int)sizeof(GeoItem);
	out[4] = (int)sizeof(GeoView); out[5] = kViewSlotEntries;
	DevView slot[kViewSlotEntries];
	out[6] = (int)((const char*)geo_item(slot) - (const char*)slot);
	out[7] = (int)sizeof slot;
}
int gp_sweep_item_geo(int geo) {
	EstConst k;
	memset(&k, 0, sizeof k);
	k.W = 96; k.H = 80; k.border = 7; k.V = 3; k.hintIter = -1;
	return est_sweep_item(k, 2, false, geo != 0).geo;
}
// the aliasing rule: one item of w x h whose in/out maps start at io[3]; one source view of sw x sh whose maps start at sp[2]; returns the offending item or -1
int gp_overlap(int w, int h, const uint64_t* io, int sw, int sh, const uint64_t* sp, int active) {
	EstConst k;
	memset(&k, 0, sizeof k);
	k.W = w; k.H = h;
	GeoView gv[kMaxViews];
	memset(gv, 0, sizeof gv);
	gv[0].w = sw; gv[0].h = sh; gv[0].depth = (const float*)(uintptr_t)sp[0]; gv[0].normal = (const float*)(uintptr_t)sp[1];
	hcmvs_batch_item it;
	memset(&it, 0, sizeof it);
	it.n_src = 1; it.d_depth = (float*)(uintptr_t)io[0]; it.d_normal = (float*)(uintptr_t)io[1]; it.d_conf = (float*)(uintptr_t)io[2];
	const bool act = active != 0;
	return est_geo_overlap(&k, gv, &act, &it, 1).item;
}

// ---- sweep_plan.h ----
int gp_exists(int nw, int big, int two, int pack, int hint, int mask, int spread, int prior, int geo) {
	return sweep_variant_exists({nw, big != 0, two != 0, pack != 0, hint != 0, mask != 0, spread != 0, prior != 0, geo != 0});
}
// out[10]: nw, big, two, pack, hint, mask, spread, prior, geo, exists
void gp_resolve(int requested, int V, int big, int hint, int mask, int spread, int prior, int geo, int* out) {
	const SweepVariant v = resolve_sweep_variant(requested, V, big != 0, hint != 0, mask != 0, spread != 0, prior != 0, geo != 0);
	const int f[10] = {v.nw, v.big, v.two, v.pack, v.hint, v.mask, v.spread, v.prior, v.geo, sweep_variant_exists(v)};
	for (int i = 0; i < 10; ++i) out[i] = f[i];
}
// items: n x (rows, cols, nSrc, mask, geo); out per launch: first, count, nw, geo, exists
int gp_plan(const int* items, int n, int nSweeps, int perLaunch, int* out, int cap) {
	SweepBatch b;
	for (int i = 0; i < n; ++i, items += 5) b.items.push_back({items[0], items[1], items[2], false, items[3] != 0, false, false, items[4] != 0});
	b.nSweeps = nSweeps; b.nCU = 256; b.sweepPerLaunch = perLaunch;
	const std::vector<SweepLaunch> plan = plan_sweeps(b);
	for (int i = 0; i < (int)plan.size() && i < cap; ++i, out += 5) {
		out[0] = plan[i].first; out[1] = plan[i].count; out[2] = plan[i].v.nw; out[3] = plan[i].v.geo; out[4] = sweep_variant_exists(plan[i].v);
	}
	return (int)plan.size();
}
}

// C face of what the depth prior adds to hc-mvs_amd/csrc/est_plan.h and sweep_plan.h, for tests/test_prior_plan.py (ctypes).  Links nothing
// of the library and nothing of HIP.
#include "../hc-mvs_amd/csrc/est_plan.h"

using namespace hcmvs;

extern "C" {

// ---- est_plan.h ----
// 0 ok, 1 para_prior, 2 sigma_prior, 3 photo2geo
int pp_check_params(float para, float sigma, int photo2geo) {
	const hcmvs_prior_params p = {para, sigma, photo2geo};
	const PriorBad b = est_check_prior_params(p);
	return b == kPriorOk ? 0 : b == kPriorPara ? 1 : b == kPriorSigma ? 2 : 3;
}
int pp_active(int registered, float para, float sigma, int photo2geo, int itExternal) {
	const hcmvs_prior_params pp = {para, sigma, photo2geo};
	hcmvs_params p;
	memset(&p, 0, sizeof p);
	p.it_external = itExternal;
	return est_prior_active(registered != 0, pp, p);
}
// out[3]: keep, para, sigma; returns countIter
int pp_consts(float para, float sigma, int countIter, float* out) {
	const hcmvs_prior_params pp = {para, sigma, 0};
	PriorItem k;
	memset(&k, 0xff, sizeof k);
	est_prior_consts(pp, countIter, k);
	out[0] = k.keep; out[1] = k.para; out[2] = k.sigma;
	return k.countIter;
}
// flags: n x (prior active, hint in effect, spread at work); returns 0 ok, 1 hint, 2 spread; *at: the item
int pp_check_batch(const int* flags, int n, int* at) {
	bool a[HCMVS_MAX_BATCH], h[HCMVS_MAX_BATCH], s[HCMVS_MAX_BATCH];
	for (int i = 0; i < n; ++i) { a[i] = flags[3 * i] != 0; h[i] = flags[3 * i + 1] != 0; s[i] = flags[3 * i + 2] != 0; }
	const EstCheck c = est_check_prior_batch(a, h, s, n);
	*at = c.at;
	return c.broken == kEstOk ? 0 : c.broken == kEstPriorHint ? 1 : c.broken == kEstPriorSpread ? 2 : -1;
}
int pp_check_sweeps(int first, int n) { return est_check_sweeps(first, n).broken == kEstOk ? 0 : est_check_sweeps(first, n).broken == kEstSweepRange ? 1 : -1; }
int pp_max_sweep_index() { return HCMVS_MAX_SWEEP_INDEX; }
// sizes of EstConst, DevView, PriorItem, entries per view slot; where the PriorItem of a slot lies (bytes behind the slot's first view)
void pp_layout(int* out) {
	out[0] = (int)sizeof(EstConst); out[1] = (int)sizeof(DevView); out[2] = (int)sizeof(PriorItem); out[3] = kViewSlotEntries;
	DevView slot[kViewSlotEntries];
	out[4] = (int)((const char*)prior_item(slot) - (const char*)slot);
}
int pp_sweep_item_prior(int prior) {
	EstConst k;
	memset(&k, 0, sizeof k);
	k.W = 96; k.H = 80; k.border = 7; k.V = 3; k.hintIter = -1;
	return est_sweep_item(k, 2, prior != 0).prior;
}

// ---- sweep_plan.h ----
int pp_exists(int nw, int big, int two, int pack, int hint, int mask, int spread, int prior) {
	return sweep_variant_exists({nw, big != 0, two != 0, pack != 0, hint != 0, mask != 0, spread != 0, prior != 0});
}
int pp_exists_default(int nw, int big, int two, int pack, int hint, int mask, int spread) { // the seven-member form existing callers use
	return sweep_variant_exists({nw, big != 0, two != 0, pack != 0, hint != 0, mask != 0, spread != 0});
}
// out[9]: nw, big, two, pack, hint, mask, spread, prior, exists
void pp_resolve(int requested, int V, int big, int hint, int mask, int spread, int prior, int* out) {
	const SweepVariant v = resolve_sweep_variant(requested, V, big != 0, hint != 0, mask != 0, spread != 0, prior != 0);
	const int f[9] = {v.nw, v.big, v.two, v.pack, v.hint, v.mask, v.spread, v.prior, sweep_variant_exists(v)};
	for (int i = 0; i < 9; ++i) out[i] = f[i];
}
// items: n x (rows, cols, nSrc, hintLast, mask, spread, prior); out per launch: first, count, nw, prior, exists
int pp_plan(const int* items, int n, int nSweeps, int firstSweep, int perLaunch, int* out, int cap) {
	SweepBatch b;
	for (int i = 0; i < n; ++i, items += 7) b.items.push_back({items[0], items[1], items[2], items[3] != 0, items[4] != 0, items[5] != 0, items[6] != 0});
	b.nSweeps = nSweeps; b.firstSweep = firstSweep; b.nCU = 256; b.sweepPerLaunch = perLaunch;
	const std::vector<SweepLaunch> plan = plan_sweeps(b);
	for (int i = 0; i < (int)plan.size() && i < cap; ++i, out += 5) {
		out[0] = plan[i].first; out[1] = plan[i].count; out[2] = plan[i].v.nw; out[3] = plan[i].v.prior; out[4] = sweep_variant_exists(plan[i].v);
	}
	return (int)plan.size();
}
}

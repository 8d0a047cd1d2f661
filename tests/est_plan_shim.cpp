// C face of hc-mvs_amd/csrc/est_plan.h (and of the knob parser of sweep_plan.h) for tests/test_est_plan.py (ctypes).  Links nothing of
// the library and nothing of HIP.  Addresses come in as plain integers: nothing here is dereferenced or allocated on a device.
#include "../hc-mvs_amd/csrc/est_plan.h"
#include <vector>

using namespace hcmvs;

struct EpCam {
	double K[9], R[9], C[3];
	int32_t w, h;
};
static EstCamera cam(const EpCam& c) { return {c.K, c.R, c.C, c.w, c.h}; }

// the value members of EstConst and of its DevView entries, by name
struct EpItem {
	int32_t W, H, V, border, adapthalfwin, nRandomIters, itExternal, propHalfwin, propStep, hintIter;
	uint32_t seed;
	int32_t pointersSet; // pointer members of EstConst that are not null, plus byteOff members that are not zero (expected: 0)
	float Hr[9];
	float dMin, dMax, dMinSqr, dMaxSqr, smoothBonusDepth, smoothBonusNormal, smoothSigmaDepth, smoothSigmaNormal, angle1Range, angle2Range;
	float thConfSmall, thConfBig, thConfRand, thRobust, thKeep, depthRatio, pfScale;
	double cx, cy, ifx, ify;
	float A[kMaxViews][9], Hm[kMaxViews][3];
	int32_t vw[kMaxViews], vh[kMaxViews];
};

extern "C" {

// sizes of the structures the kernels read, and the values of the reason codes in the order of the enum's declaration
void ep_layout(int* sizes, int* reasons) {
	sizes[0] = (int)sizeof(EstConst); sizes[1] = (int)sizeof(DevView); sizes[2] = (int)sizeof(SpreadView);
	const int r[9] = {kEstOk, kEstBatchSize, kEstHalfWindow, kEstIterCounts, kEstSrcCount, kEstSrcClass, kEstNull, kEstDepthRange, kEstBorder};
	for (int i = 0; i < 9; ++i) reasons[i] = r[i];
}

void ep_item(const EpCam* ref, const EpCam* src, int nSrc, const hcmvs_params* p, float dMin, float dMax, uint32_t seedOffset, int hintOffered, EpItem* o) {
	EstCamera s[kMaxViews];
	for (int v = 0; v < nSrc; ++v) s[v] = cam(src[v]);
	EstConst k;
	DevView dv[kMaxViews];
	memset(&k, 0xff, sizeof k); memset(dv, 0xff, sizeof dv); // the plan must leave nothing as it found it
	est_item_consts(cam(*ref), s, nSrc, *p, dMin, dMax, seedOffset, hintOffered != 0, k, dv);
	memset(o, 0, sizeof *o);
	o->W = k.W; o->H = k.H; o->V = k.V; o->border = k.border; o->adapthalfwin = k.adapthalfwin; o->nRandomIters = k.nRandomIters;
	o->itExternal = k.itExternal; o->propHalfwin = k.propHalfwin; o->propStep = k.propStep; o->hintIter = k.hintIter; o->seed = k.seed;
	o->pointersSet = (k.ref != nullptr) + (k.gra != nullptr) + (k.views != nullptr) + (k.imgBase != nullptr) + (k.dn != nullptr) + (k.conf != nullptr) +
	                 (k.progress != nullptr) + (k.hintDepth != nullptr) + (k.hintNormal != nullptr) + (k.keep != nullptr) + (k.spread != nullptr);
	memcpy(o->Hr, k.Hr, sizeof k.Hr);
	o->dMin = k.dMin; o->dMax = k.dMax; o->dMinSqr = k.dMinSqr; o->dMaxSqr = k.dMaxSqr;
	o->smoothBonusDepth = k.smoothBonusDepth; o->smoothBonusNormal = k.smoothBonusNormal;
	o->smoothSigmaDepth = k.smoothSigmaDepth; o->smoothSigmaNormal = k.smoothSigmaNormal;
	o->angle1Range = k.angle1Range; o->angle2Range = k.angle2Range;
	o->thConfSmall = k.thConfSmall; o->thConfBig = k.thConfBig; o->thConfRand = k.thConfRand; o->thRobust = k.thRobust; o->thKeep = k.thKeep;
	o->depthRatio = k.depthRatio; o->pfScale = k.pfScale;
	o->cx = k.cx; o->cy = k.cy; o->ifx = k.ifx; o->ify = k.ify;
	for (int v = 0; v < kMaxViews; ++v) {
		memcpy(o->A[v], dv[v].A, sizeof dv[v].A); memcpy(o->Hm[v], dv[v].Hm, sizeof dv[v].Hm);
		o->vw[v] = dv[v].w; o->vh[v] = dv[v].h;
		o->pointersSet += dv[v].byteOff != 0;
	}
}

int ep_uses_hint(const hcmvs_params* p, int offered) { return est_uses_hint(*p, offered != 0); }
int ep_view_spreads(int viewspread, const hcmvs_params* p, int offersMaps, int rescaled) {
	return est_view_spreads(viewspread != 0, *p, offersMaps != 0, rescaled != 0);
}
// out[8]: cx, cy, ifx, ify, Tz[3], tz; wh[2]
void ep_spread(const EpCam* ref, const EpCam* s, double* out, int* wh) {
	SpreadView sv;
	memset(&sv, 0, sizeof sv);
	est_spread_consts(cam(*ref), cam(*s), sv);
	out[0] = sv.cx; out[1] = sv.cy; out[2] = sv.ifx; out[3] = sv.ify; out[4] = sv.Tz[0]; out[5] = sv.Tz[1]; out[6] = sv.Tz[2]; out[7] = sv.tz;
	wh[0] = sv.w; wh[1] = sv.h;
}

// in: W, H, border, V, hint pointers set, hintIter, keep set, spread set; out: rows, cols, nSrc, hintLast, mask, spread
void ep_sweep_item(const int* in, int nSweeps, int* out) {
	static const float f = 0.f; static const uint8_t u = 0; static const SpreadView sv = {};
	EstConst k;
	memset(&k, 0, sizeof k);
	k.W = in[0]; k.H = in[1]; k.border = in[2]; k.V = in[3];
	if (in[4]) { k.hintDepth = &f; k.hintNormal = &f; }
	k.hintIter = in[5];
	if (in[6]) k.keep = &u;
	if (in[7]) k.spread = &sv;
	const SweepItem it = est_sweep_item(k, nSweeps);
	out[0] = it.rows; out[1] = it.cols; out[2] = it.nSrc; out[3] = it.hintLast; out[4] = it.mask; out[5] = it.spread;
}

// returns the kind (0 direct, 1 slab, 2 refused); off[n]; baseAndSlab[2]
int ep_window(const uint64_t* addr, const uint64_t* bytes, int n, uint32_t* off, uint64_t* baseAndSlab) {
	std::vector<size_t> b(bytes, bytes + n);
	const EstWindow w = est_image_window(addr, b.data(), n, off);
	baseAndSlab[0] = w.base; baseAndSlab[1] = w.slabBytes;
	return w.kind == kEstWindowDirect ? 0 : w.kind == kEstWindowSlab ? 1 : 2;
}
// what Carve gives for the same sizes in the same order: off[n], returns the total
uint64_t ep_carve(const uint64_t* bytes, int n, uint64_t* off) {
	Carve cv;
	for (int v = 0; v < n; ++v) off[v] = cv((size_t)bytes[v]);
	return cv.size;
}

// items: n x (W, H, depth, normal, conf, n_src, spread on); views: n x kMaxViews x (depth, normal, conf, w, h), depth 0 = offers none.
// out[3]: item, other, view
void ep_overlap(const uint64_t* items, const uint64_t* views, int n, int* out) {
	std::vector<EstConst> k(n);
	std::vector<SpreadView> sv((size_t)n * kMaxViews);
	std::vector<hcmvs_batch_item> it(n);
	memset(k.data(), 0, sizeof(EstConst) * n); memset(sv.data(), 0, sizeof(SpreadView) * sv.size()); memset(it.data(), 0, sizeof(hcmvs_batch_item) * n);
	for (int i = 0; i < n; ++i) {
		const uint64_t* a = items + 7 * i;
		k[i].W = (int32_t)a[0]; k[i].H = (int32_t)a[1];
		it[i].d_depth = (float*)(uintptr_t)a[2]; it[i].d_normal = (float*)(uintptr_t)a[3]; it[i].d_conf = (float*)(uintptr_t)a[4];
		it[i].n_src = (int32_t)a[5];
		k[i].spread = a[6] ? sv.data() + (size_t)i * kMaxViews : nullptr;
		for (int v = 0; v < kMaxViews; ++v) {
			const uint64_t* b = views + 5 * ((size_t)i * kMaxViews + v);
			SpreadView& s = sv[(size_t)i * kMaxViews + v];
			s.depth = (const float*)(uintptr_t)b[0]; s.normal = (const float*)(uintptr_t)b[1]; s.conf = (const float*)(uintptr_t)b[2];
			s.w = (int32_t)b[3]; s.h = (int32_t)b[4];
		}
	}
	const EstOverlap o = est_spread_overlap(k.data(), sv.data(), it.data(), n);
	out[0] = o.item; out[1] = o.other; out[2] = o.view;
}

int ep_check_call(int nItems, const hcmvs_params* p) { return est_check_call(nItems, *p).broken; }
// the items in order, as a batch is built: the first broken rule and, in *at, its item.  isNull[i]: the item comes without its maps
int ep_check_items(const int* nSrc, const float* dMin, const float* dMax, const int* isNull, int n, int* at) {
	static uint32_t ids[kMaxViews];
	static float map;
	std::vector<hcmvs_batch_item> it(n);
	memset(it.data(), 0, sizeof(hcmvs_batch_item) * n);
	for (int i = 0; i < n; ++i) {
		it[i].n_src = nSrc[i]; it[i].d_min = dMin[i]; it[i].d_max = dMax[i];
		it[i].src_ids = ids; it[i].d_depth = &map; it[i].d_normal = &map; it[i].d_conf = isNull[i] ? nullptr : &map;
	}
	*at = -1;
	for (int i = 0; i < n; ++i) {
		const EstCheck c = est_check_item(it.data(), i);
		if (c.broken != kEstOk) { *at = c.at; return c.broken; }
	}
	return kEstOk;
}
int ep_check_image(int i, int w, int h, const hcmvs_params* p, int* at) {
	const EstCheck c = est_check_image(i, w, h, *p);
	*at = c.at;
	return c.broken;
}

// out[5]: lag, affinity, launches, segment, waves per row
void ep_knobs(const char* lag, const char* affinity, const char* launches, const char* segment, const char* waves, int* out) {
	const SweepKnobs k = parse_sweep_knobs(lag, affinity, launches, segment, waves);
	out[0] = k.lag; out[1] = k.affinity; out[2] = k.perLaunch; out[3] = k.segment; out[4] = k.wavesPerRow;
}
}

// C face of hc-mvs_amd/csrc/fuse_plan.h for tests/test_fuse_plan.py (ctypes).  Links nothing of the library and nothing of HIP.
#include "../hc-mvs_amd/csrc/fuse_plan.h"

using namespace hcmvs;
typedef unsigned long long u64;

// the map table: per image id its pixels, whether it has maps, and its neighbour list nbIds[nbFirst[id] .. nbFirst[id + 1])
static std::vector<PlanMap> table(const u64* pixels, const int* hasMaps, const int* nbFirst, const uint32_t* nbIds, int nMaps) {
	std::vector<PlanMap> maps((size_t)nMaps);
	for (int i = 0; i < nMaps; ++i) {
		maps[(size_t)i].pixels = (size_t)pixels[i]; maps[(size_t)i].hasMaps = hasMaps[i] != 0;
		maps[(size_t)i].nNeighbors = nbFirst[i + 1] - nbFirst[i]; maps[(size_t)i].neighbors = nbIds + nbFirst[i];
	}
	return maps;
}
static FuseDims dims_of(u64 maxArea, u64 stride, int maxNb) {
	FuseDims d;
	d.maxArea = (size_t)maxArea; d.stride = (size_t)stride; d.maxNb = maxNb;
	return d;
}
static int put_core(const FuseCore& o, u64* out) {
	const size_t v[11] = {o.pending, o.settle, o.targets, o.head, o.next, o.ctl, o.counters, o.status, o.merged, o.flag, o.nv};
	for (int i = 0; i < 11; ++i) out[i] = v[i];
	return 11;
}

extern "C" {
int fup_max_views() { return kFuseMaxViews; }
// out: maxArea, stride, maxNb, broken (FuseLimit), at
void fup_dims(const u64* pixels, const int* hasMaps, const int* nbFirst, const uint32_t* nbIds, int nMaps, const uint32_t* order, int nOrder, u64* out) {
	const FuseDims d = fuse_dims(table(pixels, hasMaps, nbFirst, nbIds, nMaps), order, nOrder);
	out[0] = d.maxArea; out[1] = d.stride; out[2] = (u64)d.maxNb; out[3] = (u64)d.broken; out[4] = (u64)(long long)d.at;
}
// off: pending settle targets head next ctl counters status merged flag nv | totals flag32 pos scan xyz nrm bgr pviews pweights voff; returns the bytes
u64 fup_cloud_pass(u64 maxArea, u64 stride, int maxNb, u64 settleBytes, u64 ctlBytes, u64 scanBytes, int viewLists, u64* off) {
	const FuseCloudPass o = plan_fuse_cloud_pass(dims_of(maxArea, stride, maxNb), (size_t)settleBytes, (size_t)ctlBytes, (size_t)scanBytes, viewLists != 0);
	int k = put_core(o, off);
	const size_t v[10] = {o.totals, o.flag32, o.pos, o.scan, o.xyz, o.nrm, o.bgr, o.pviews, o.pweights, o.voff};
	for (int i = 0; i < 10; ++i) off[k++] = v[i];
	return o.bytes;
}
// off: the core as above | dF dF2 nF; returns the bytes
u64 fup_postfilter_pass(u64 maxArea, u64 stride, int maxNb, u64 settleBytes, u64 ctlBytes, u64 maxIdArea, u64* off) {
	const FusePostfilterPass o = plan_postfilter_pass(dims_of(maxArea, stride, maxNb), (size_t)settleBytes, (size_t)ctlBytes, (size_t)maxIdArea);
	int k = put_core(o, off);
	off[k++] = o.dF; off[k++] = o.dF2; off[k++] = o.nF;
	return o.bytes;
}
// off: xyz normal bgr nViews viewIds viewWeights; returns the bytes
u64 fup_cloud_out(u64 capacity, u64 viewCapacity, int wantXyz, int wantNormal, int wantBgr, int wantNViews, u64* off) {
	const FuseCloudOut o = plan_fuse_cloud_out((size_t)capacity, (size_t)viewCapacity, wantXyz != 0, wantNormal != 0, wantBgr != 0, wantNViews != 0);
	const size_t v[6] = {o.xyz, o.normal, o.bgr, o.nViews, o.viewIds, o.viewWeights};
	for (int i = 0; i < 6; ++i) off[i] = v[i];
	return o.bytes;
}
// img: per image id 13 words (own chgNow valNext tgt head next acc mm fm stamp touch stride inOrder); tail: anyChg table scratch ctl counters status dF
// dF2 nF.  Returns 1 and the bytes when the chain can run incrementally, else 0 (img and tail are then left alone).
int fup_chain(const u64* pixels, const int* hasMaps, const int* nbFirst, const uint32_t* nbIds, int nMaps, const uint32_t* ids, int nIds, const uint32_t* order,
              int nOrder, u64 maxIdArea, u64 pfImageBytes, u64 scratchBytes, u64 ctlBytes, u64* img, u64* tail, u64* bytes) {
	const PfChainPlan p = plan_pf_chain(table(pixels, hasMaps, nbFirst, nbIds, nMaps), ids, nIds, order, nOrder, (size_t)maxIdArea, (size_t)pfImageBytes,
	                                    (size_t)scratchBytes, (size_t)ctlBytes);
	*bytes = p.bytes;
	if (!p.ok) return 0;
	for (int i = 0; i < nMaps; ++i) {
		const PfImagePlan& L = p.images[(size_t)i];
		const size_t v[13] = {L.own, L.chgNow, L.valNext, L.tgt, L.head, L.next, L.acc, L.mm, L.fm, L.stamp, L.touch, L.stride, (size_t)L.inOrder};
		for (int k = 0; k < 13; ++k) img[13 * (size_t)i + k] = v[k];
	}
	const size_t t[9] = {p.anyChg, p.table, p.scratch, p.ctl, p.counters, p.status, p.dF, p.dF2, p.nF};
	for (int k = 0; k < 9; ++k) tail[k] = t[k];
	return 1;
}
}

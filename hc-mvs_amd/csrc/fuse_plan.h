/* hc-mvs_amd/csrc/fuse_plan.h -- the host-side arithmetic of the fusion and of the post-filter chain: the dimensions of a fusion call and
 * their limits, the layout of the per-pass tables, the layout of the chain's state.  Plain C++ (no HIP), so that tests/test_fuse_plan.py
 * checks it without a GPU; what only the device side knows (the kernels' scratch sizes, the sizes of their structures) is an argument. */
#ifndef HCMVS_FUSE_PLAN_H
#define HCMVS_FUSE_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "carve.h"
namespace hcmvs {

constexpr int kFuseMaxViews = 32; // views merged into one point / estimates one point can invalidate

// one entry of the map table (indexed by image id) as the plans see it
struct PlanMap {
	size_t pixels = 0;
	bool hasMaps = false;
	int nNeighbors = 0;
	const uint32_t* neighbors = nullptr; // the image's neighbour list (ids; an id outside the table or without maps is passed over)
};

// ---- the dimensions of a fusion call ----
enum FuseLimit {
	kFuseOk = 0,
	kFuseNoMaps,           // order[at] has no maps                                    (an invalid call)
	kFuseTooManyNeighbors, // order[at] has more neighbours than a point has views     (an invalid call)
	kFuseStrideLimit,      // a map too large for the 29 index bits of a target        (beyond the tables' capacity)
	kFuseTableLimit        // stride * maxNb beyond a 31-bit index into the tables     (beyond the tables' capacity)
};
struct FuseDims {
	size_t maxArea = 0; // pixels of the largest image of the order
	size_t stride = 0;  // pixels reserved per neighbour map in the per-target tables: the largest image with maps of the whole table
	int maxNb = 1;      // most neighbours of an image of the order, at least 1
	FuseLimit broken = kFuseOk;
	int at = -1;        // position of the order that broke the limit (kFuseNoMaps, kFuseTooManyNeighbors)
};
inline FuseDims fuse_dims(const std::vector<PlanMap>& maps, const uint32_t* order, int nOrder) {
	FuseDims d;
	for (int i = 0; i < nOrder; ++i) {
		d.at = i;
		if (order[i] >= maps.size() || !maps[order[i]].hasMaps) { d.broken = kFuseNoMaps; return d; }
		const PlanMap& m = maps[order[i]];
		if (m.nNeighbors > kFuseMaxViews - 1) { d.broken = kFuseTooManyNeighbors; return d; }
		d.maxArea = std::max(d.maxArea, m.pixels);
		d.maxNb = std::max(d.maxNb, m.nNeighbors);
	}
	d.at = -1;
	d.stride = d.maxArea;
	for (const PlanMap& m : maps) if (m.hasMaps) d.stride = std::max(d.stride, m.pixels);
	if (d.stride >= ((size_t)1 << 29)) d.broken = kFuseStrideLimit;
	else if (d.stride * (size_t)d.maxNb > 0x7FFFFFFFull) d.broken = kFuseTableLimit;
	return d;
}

// ---- the per-pass tables of a fusion from scratch (fuse_common.h), sized for the largest image / neighbour count of the call ----
// Every piece is rounded up to 256 bytes on its own: the total does not depend on the order of the pieces.
struct FuseCore { // what launch_fuse_begin and launch_fuse_pass work on
	size_t pending, settle, targets, head, next, ctl, counters, status, merged, flag, nv;
};
inline FuseCore carve_fuse_core(Carve& cv, const FuseDims& d, size_t settleBytes, size_t ctlBytes) {
	FuseCore o;
	const size_t links = d.maxArea * 4 * (size_t)d.maxNb;
	o.pending = cv(d.maxArea * 4); o.settle = cv(settleBytes); o.targets = cv(links); o.head = cv(d.stride * (size_t)d.maxNb * 4); o.next = cv(links);
	o.ctl = cv(ctlBytes); o.counters = cv(64); o.status = cv(64); o.merged = cv(d.maxArea * 4); o.flag = cv(d.maxArea); o.nv = cv(d.maxArea * 4);
	return o;
}
// hcmvs_fuse_cloud: the running totals, the compaction's tables and one image's points before they are compacted into the cloud
struct FuseCloudPass : FuseCore {
	size_t totals, flag32, pos, scan, xyz, nrm, bgr, pviews, pweights, voff, bytes;
};
inline FuseCloudPass plan_fuse_cloud_pass(const FuseDims& d, size_t settleBytes, size_t ctlBytes, size_t scanBytes, bool viewLists) {
	Carve cv;
	FuseCloudPass o;
	static_cast<FuseCore&>(o) = carve_fuse_core(cv, d, settleBytes, ctlBytes);
	const size_t lists = viewLists ? d.maxArea * 4 * (size_t)(d.maxNb + 1) : 0;
	o.totals = cv(64); o.flag32 = cv(d.maxArea * 4); o.pos = cv(d.maxArea * 4); o.scan = cv(scanBytes);
	o.xyz = cv(d.maxArea * 12); o.nrm = cv(d.maxArea * 12); o.bgr = cv(d.maxArea * 3);
	o.pviews = cv(lists); o.pweights = cv(lists); o.voff = cv(viewLists ? d.maxArea * 4 : 0);
	o.bytes = cv.size;
	return o;
}
// hcmvs_postfilter_sequence: the gap interpolation's scratch, for the largest image to filter (maxIdArea pixels)
struct FusePostfilterPass : FuseCore {
	size_t dF, dF2, nF, bytes;
};
inline FusePostfilterPass plan_postfilter_pass(const FuseDims& d, size_t settleBytes, size_t ctlBytes, size_t maxIdArea) {
	Carve cv;
	FusePostfilterPass o;
	static_cast<FuseCore&>(o) = carve_fuse_core(cv, d, settleBytes, ctlBytes);
	o.dF = cv(maxIdArea * 4); o.dF2 = cv(maxIdArea * 4); o.nF = cv(maxIdArea * 12);
	o.bytes = cv.size;
	return o;
}
// the device copy of the cloud hcmvs_fuse_cloud fills: only the outputs the caller asked for take room
struct FuseCloudOut {
	size_t xyz, normal, bgr, nViews, viewIds, viewWeights, bytes;
};
inline FuseCloudOut plan_fuse_cloud_out(size_t capacity, size_t viewCapacity, bool wantXyz, bool wantNormal, bool wantBgr, bool wantNViews) {
	Carve cv;
	FuseCloudOut o;
	o.xyz = cv(wantXyz ? capacity * 12 : 0); o.normal = cv(wantNormal ? capacity * 12 : 0); o.bgr = cv(wantBgr ? capacity * 3 : 0);
	o.nViews = cv(wantNViews || viewCapacity ? capacity * 4 : 0); o.viewIds = cv(viewCapacity * 4); o.viewWeights = cv(viewCapacity * 4);
	o.bytes = std::max(cv.size, (size_t)256);
	return o;
}

// ---- the state of the post-filter chain (pf_chain.h), kept from fusion to fusion ----
// Per pixel of an image with maps: own 2 + chgNow 1 + valNext 1 = 4 bytes.  Per pixel of an image of the fusion order, with N = max(its
// neighbours, 1): tgt 4 N + next 8 N + acc 1 + mm, fm, stamp, touch 16 = 17 + 12 N bytes more, and head 4 N bytes per pixel of its largest
// neighbour map.
struct PfImagePlan {
	size_t own = 0, chgNow = 0, valNext = 0;                                       // every image with maps
	size_t tgt = 0, head = 0, next = 0, acc = 0, mm = 0, fm = 0, stamp = 0, touch = 0; // the images of the order
	size_t stride = 0; // pixels reserved per neighbour in head: the image's largest neighbour map, at least 1
	bool inOrder = false;
};
struct PfChainPlan {
	bool ok = false; // false: the chain cannot run incrementally (the caller fuses from scratch)
	std::vector<PfImagePlan> images; // by image id
	size_t anyChg = 0, table = 0, scratch = 0, ctl = 0, counters = 0, status = 0, dF = 0, dF2 = 0, nF = 0;
	size_t bytes = 0;
};
// pfImageBytes: sizeof(PfImage); scratchBytes: pf_pass_scratch_bytes of the order's largest image; maxIdArea: the largest image to filter.
inline PfChainPlan plan_pf_chain(const std::vector<PlanMap>& maps, const uint32_t* ids, int nIds, const uint32_t* order, int nOrder, size_t maxIdArea,
                                 size_t pfImageBytes, size_t scratchBytes, size_t ctlBytes) {
	PfChainPlan p;
	if (nIds < 2 || nIds > 2000 || nOrder > 60000) return p;
	{ // an image is filled once per chain (a pair of estimates is linked into a bidder list at most twice)
		std::vector<uint32_t> u(ids, ids + nIds);
		std::sort(u.begin(), u.end());
		if (std::adjacent_find(u.begin(), u.end()) != u.end()) return p;
	}
	p.images.resize(maps.size());
	for (int i = 0; i < nOrder; ++i) { if (order[i] >= maps.size() || p.images[order[i]].inOrder) return p; p.images[order[i]].inOrder = true; }
	Carve cv;
	for (size_t id = 0; id < maps.size(); ++id) {
		const PlanMap& m = maps[id];
		if (!m.hasMaps) continue;
		const size_t n = m.pixels;
		if (n >= ((size_t)1 << 26) - 1) return p; // tgt holds a pixel index in 26 bits, all ones = "projects nowhere"
		PfImagePlan& L = p.images[id];
		L.own = cv(n * 2); L.chgNow = cv(n); L.valNext = cv(n);
		if (!L.inOrder) continue;
		L.stride = 1;
		for (int q = 0; q < m.nNeighbors; ++q) {
			const uint32_t nb = m.neighbors[q];
			if (nb < maps.size() && maps[nb].hasMaps) L.stride = std::max(L.stride, maps[nb].pixels);
		}
		const size_t nNb = (size_t)std::max(m.nNeighbors, 1);
		if (2 * nNb * n >= 0xFFFFFFFFull || nNb * L.stride >= 0xFFFFFFFFull) return p; // list entries are 32-bit, all ones = "none"
		L.tgt = cv(n * nNb * 4); L.head = cv(nNb * L.stride * 4); L.next = cv(2 * nNb * n * 4);
		L.acc = cv(n); L.mm = cv(n * 4); L.fm = cv(n * 4); L.stamp = cv(n * 4); L.touch = cv(n * 4);
	}
	p.anyChg = cv(maps.size() * 4); p.table = cv(maps.size() * pfImageBytes); p.scratch = cv(scratchBytes); p.ctl = cv(ctlBytes);
	p.counters = cv(64); p.status = cv(64); p.dF = cv(maxIdArea * 4); p.dF2 = cv(maxIdArea * 4); p.nF = cv(maxIdArea * 12);
	p.bytes = cv.size;
	p.ok = true;
	return p;
}

} // namespace hcmvs
#endif

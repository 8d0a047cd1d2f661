/*
 * hc-mvs_amd/csrc/view_kernels.hip -- view selection for every image of a scene on the device.
 *
 * Scene::SelectNeighborViews (frame_main/libs/MVS/Scene.cpp:545-661; Footprint :531-539, the covered area :606-645 with
 * ComputeCoveredArea<float,2,16,false>, libs/Common/Util.inl:711-730), Scene::FilterNeighborViews (:665-678) with the bounds of
 * DepthMapsData::SelectViews (SceneDensify.cpp:307-327) and the cut of DepthMapsData::InitViews (SceneDensify.cpp:362-367).  The
 * reference runs this once per image, each time over the whole sparse cloud.  Here the cloud is walked once: every vertex contributes one
 * record per ORDERED pair (A, B) of its calibrated views, and a pair's records, gathered by a stable sort, are added up by one wave, one
 * record after the other in ascending vertex index -- the reference's order, so no float atomics and a result that is bit-identical run
 * to run and independent of how the images are split into ranges.
 *
 * Launches.  Once: entry_kernel (one thread per view entry: the key of the per-image sort and float(depth)), a radix sort of the entries
 * by image, image_kernel (one wave per image: nPoints, the points list's length, avgDepth summed sequentially by shuffles), a second
 * time when the points lists are asked for, to write them.  Per range [a0, a1) of images A: count_kernel + exclusive scan (records per entry),
 * emit_kernel (one thread per view entry (vertex, A): its m - 1 records), a stable radix sort of (key = (A - a0) * nImages + B, record
 * index), segment_kernel (one wave per (A, B): two binary searches for its segment, then the records 64 at a time -- the gathers of a
 * round in flight together, the float32 sums one record after the other through shuffles -- and the 256-bit cell mask) and select_kernel (one
 * wave per image: counts the candidates, then picks the best M that pass the filter one by one -- M <= 64 rounds of a strided scan and a
 * wave reduction, which is the stable sort by decreasing score, ties by ascending id, cut after M -- and lane 0 makes the InitViews cut).
 */
#include "view_kernels.h"

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

namespace hcmvs {

namespace {

static const dim3 kBlock(256);

struct Cam { double K[9], R[9], C[3]; int w, h; };
struct __align__(16) Rec { float term, ratio, angle; int cell; };            // cell < 0: the vertex does not count for the covered area
struct Cand { float score, sumScale, sumAngle; uint32_t points, cells, nProj; };
struct DevParams {
	int nMinViews, nMinPointViews, nMaxViews, numberViews;
	float optimAngle, minAngle, maxAngle, minArea, minScale, maxScale, minScoreRatio, minScore; // angles in radians
};
struct DevOut {
	int32_t* status;
	uint32_t *nSeen, *nPts, *nCandidates, *nNeighbors, *nSrcs;
	float* avgDepth;
	uint32_t *nbId, *nbPoints;
	float *nbScale, *nbAngle, *nbArea, *nbScore, *srcScale;
};

__device__ __forceinline__ bool calibrated(const Cam* cams, uint32_t nImages, uint32_t id) { return id < nImages && cams[id].w > 0; }
// Camera::TransformPointW2C for a Point3f: R (X - C) in double
__device__ __forceinline__ void w2c(const Cam& c, const float* X, double* p) {
	const double d0 = (double)X[0] - c.C[0], d1 = (double)X[1] - c.C[1], d2 = (double)X[2] - c.C[2];
#pragma unroll
	for (int i = 0; i < 3; ++i) p[i] = (c.R[3 * i] * d0 + c.R[3 * i + 1] * d1) + c.R[3 * i + 2] * d2;
}
// Camera::ProjectPointP (Camera.h:284-288): K (R (X - C)) and the division in double, the result as float; inside: 0 <= u < w, 0 <= v < h
__device__ __forceinline__ bool project_inside(const Cam& c, const double* p, float& u, float& v) {
	const double q0 = (c.K[0] * p[0] + c.K[1] * p[1]) + c.K[2] * p[2], q1 = (c.K[3] * p[0] + c.K[4] * p[1]) + c.K[5] * p[2],
	             q2 = (c.K[6] * p[0] + c.K[7] * p[1]) + c.K[8] * p[2];
	u = (float)(q0 / q2); v = (float)(q1 / q2);
	return u >= 0.f && v >= 0.f && u < (float)c.w && v < (float)c.h;
}

// one thread per view entry: the key of the per-image sort (nImages for an entry that is skipped) and float(PointDepth) (Scene.cpp:575)
__global__ __launch_bounds__(256) void entry_kernel(uint32_t nEntries, const uint32_t* ids, const uint32_t* vertOf, const float* xyz, const Cam* cams,
                                                    uint32_t nImages, uint32_t* keyA, uint32_t* valA, float* depthF) {
	for (unsigned long long t = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; t < nEntries; t += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t e = (uint32_t)t;
		const uint32_t A = ids[e];
		const bool ok = calibrated(cams, nImages, A);
		float z = 0.f;
		if (ok) {
			double p[3];
			w2c(cams[A], xyz + 3 * (size_t)vertOf[e], p);
			z = (float)p[2];
		}
		keyA[e] = ok ? A : nImages; valA[e] = e; depthF[e] = z;
	}
}

// first position in the ascending keys[0, n) that is >= key
__device__ __forceinline__ uint32_t lower_bound(const uint32_t* keys, uint32_t n, uint32_t key) {
	uint32_t lo = 0, hi = n;
	while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < key) lo = mid + 1; else hi = mid; }
	return lo;
}

// one wave per image: its entries are the segment of the sorted keys, in ascending vertex index.  nSeen (nPoints, Scene.cpp:576), the length
// of the points list (:573-574) and avgDepth (:575, :603): the loads go 64 at a time, the sum one value after the other through shuffles.
// pointIds (or null): the points list itself, at pointsFirst[image]
__global__ __launch_bounds__(256) void image_kernel(uint32_t nImages, uint32_t nEntries, const uint32_t* keyA, const uint32_t* valA, const float* depthF,
                                                    const uint32_t* vertOf, const uint32_t* first, uint32_t nMinPointViews, uint32_t* nSeen, uint32_t* nPts,
                                                    float* avgDepth, const unsigned long long* pointsFirst, uint32_t* pointIds) {
	const uint32_t img = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (img >= nImages) return;
	const uint32_t lo = lower_bound(keyA, nEntries, img), hi = lower_bound(keyA, nEntries, img + 1);
	float sum = 0.f;
	uint32_t pts = 0;
	for (unsigned long long base = lo; base < hi; base += 64) { // 64 bits: base + 64 may pass 2^32
		const unsigned long long i = base + lane;
		float z = 0.f;
		bool isPoint = false;
		uint32_t v = 0;
		if (i < hi) {
			const uint32_t e = valA[i];
			v = vertOf[e];
			z = depthF[e];
			isPoint = first[v + 1] - first[v] >= nMinPointViews;
		}
		const unsigned long long m = __ballot(isPoint);
		if (pointIds) {
			if (isPoint) pointIds[pointsFirst[img] + pts + __popcll(m & ((1ull << lane) - 1))] = v;
		} else {
			const uint32_t cnt = (uint32_t)min(64ull, hi - base);
			for (uint32_t k = 0; k < cnt; ++k) sum += __shfl(z, (int)k, 64);
		}
		pts += (uint32_t)__popcll(m);
	}
	if (lane == 0 && !pointIds) {
		nSeen[img] = hi - lo; nPts[img] = pts;
		avgDepth[img] = hi > lo ? sum / (float)(hi - lo) : 0.f;
	}
}

// one thread per view entry: the records it will emit in the range [a0, a1)
__global__ __launch_bounds__(256) void count_kernel(uint32_t nEntries, const uint32_t* ids, const uint32_t* vertOf, const uint32_t* nValid, const Cam* cams,
                                                    uint32_t nImages, uint32_t a0, uint32_t a1, uint32_t* counts) {
	for (unsigned long long t = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; t < nEntries; t += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t e = (uint32_t)t;
		const uint32_t A = ids[e];
		counts[e] = A >= a0 && A < a1 && calibrated(cams, nImages, A) ? nValid[vertOf[e]] - 1 : 0;
	}
}

// one thread per view entry (vertex, A) with A in [a0, a1): one record per other calibrated view B of the vertex (Scene.cpp:578-600 and the
// vertex's share of :620-635).  nRecords bounds every store
__global__ __launch_bounds__(256) void emit_kernel(uint32_t nEntries, const uint32_t* ids, const uint32_t* vertOf, const uint32_t* first, const float* xyz,
                                                   const Cam* cams, uint32_t nImages, uint32_t a0, uint32_t a1, const uint32_t* offsets, uint32_t nRecords,
                                                   uint32_t nMinPointViews, float optimAngle, uint32_t* keys, uint32_t* vals, Rec* recs) {
	for (unsigned long long t = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; t < nEntries; t += (unsigned long long)gridDim.x * blockDim.x) {
		const uint32_t e = (uint32_t)t;
		const uint32_t A = ids[e];
		if (A < a0 || A >= a1 || !calibrated(cams, nImages, A)) continue;
		const uint32_t v = vertOf[e], lo = first[v], hi = first[v + 1];
		const float X[3] = {xyz[3 * (size_t)v], xyz[3 * (size_t)v + 1], xyz[3 * (size_t)v + 2]};
		const Cam& ca = cams[A];
		double pa[3];
		w2c(ca, X, pa);
		const float V1[3] = {(float)(ca.C[0] - (double)X[0]), (float)(ca.C[1] - (double)X[1]), (float)(ca.C[2] - (double)X[2])};
		const float n1 = (V1[0] * V1[0] + V1[1] * V1[1]) + V1[2] * V1[2];
		const float fp1 = (float)(ca.K[0] / pa[2]); // Footprint (Scene.cpp:531-539): focal length / depth
		float ua = 0.f, va = 0.f;
		const bool counted = hi - lo >= nMinPointViews && pa[2] > 0 && project_inside(ca, pa, ua, va);
		int cell = -1;
		if (counted) cell = min(15, (int)(ua / (float)ca.w * 16.f)) * 16 + min(15, (int)(va / (float)ca.h * 16.f));
		uint32_t o = offsets[e];
		for (uint32_t j = lo; j < hi; ++j) {
			const uint32_t B = ids[j];
			if (j == e || !calibrated(cams, nImages, B) || o >= nRecords) continue;
			const Cam& cb = cams[B];
			const float V2[3] = {(float)(cb.C[0] - (double)X[0]), (float)(cb.C[1] - (double)X[1]), (float)(cb.C[2] - (double)X[2])};
			const float n2 = (V2[0] * V2[0] + V2[1] * V2[1]) + V2[2] * V2[2];
			float c = ((V1[0] * V2[0] + V1[1] * V2[1]) + V1[2] * V2[2]) / sqrtf(n1 * n2); // ComputeAngle (Util.inl:417-420)
			c = fminf(1.f, fmaxf(-1.f, c));
			const float ang = acosf(c);
			const float wAngle = fminf(powf(ang / optimAngle, 1.5f), 1.f);
			double pb[3];
			w2c(cb, X, pb);
			const float r = fp1 / (float)(cb.K[0] / pb[2]);
			float wScale;
			if (r > 1.6f) { const float q = 1.6f / r; wScale = q * q; }
			else if (r >= 1.f) wScale = 1.f;
			else wScale = r * r;
			float ub, vb;
			Rec rec;
			rec.term = wAngle * wScale; rec.ratio = r; rec.angle = ang;
			rec.cell = cell >= 0 && pb[2] > 0 && project_inside(cb, pb, ub, vb) ? cell : -1;
			keys[o] = (A - a0) * nImages + B; vals[o] = o; recs[o] = rec;
			++o;
		}
	}
}

// one wave per (A, B) of the range: the pair's records are the segment of its key, in ascending vertex index.  The wave gathers 64 records
// at a time -- one round of loads instead of 64 dependent ones -- and adds them one after the other through shuffles: the sums are those of
// one lane walking the segment, in the same order
__global__ __launch_bounds__(256) void segment_kernel(uint32_t nCells, uint32_t nRecords, const uint32_t* keys, const uint32_t* vals, const Rec* recs, Cand* cand) {
	const uint32_t lane = threadIdx.x & 63;
	const unsigned long long wavesPerBlock = blockDim.x >> 6;
	for (unsigned long long t = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); t < nCells; t += (unsigned long long)gridDim.x * wavesPerBlock) {
		const uint32_t c = (uint32_t)t; // c + 1 <= nCells < 2^32
		const uint32_t lo = lower_bound(keys, nRecords, c), hi = lower_bound(keys, nRecords, c + 1);
		float score = 0.f, sumScale = 0.f, sumAngle = 0.f;
		uint32_t nProj = 0;
		unsigned long long m0 = 0, m1 = 0, m2 = 0, m3 = 0;
		for (uint32_t base = lo; base < hi; base += 64) {
			Rec r = {0.f, 0.f, 0.f, -1};
			if (base + lane < hi) r = recs[vals[base + lane]];
			if (r.cell >= 0) {
				const unsigned long long bit = 1ull << (r.cell & 63);
				const int w = r.cell >> 6;
				m0 |= w == 0 ? bit : 0; m1 |= w == 1 ? bit : 0; m2 |= w == 2 ? bit : 0; m3 |= w == 3 ? bit : 0;
				++nProj;
			}
			const uint32_t cnt = min(64u, hi - base);
			for (uint32_t k = 0; k < cnt; ++k) {
				score += __shfl(r.term, (int)k, 64); sumScale += __shfl(r.ratio, (int)k, 64); sumAngle += __shfl(r.angle, (int)k, 64);
			}
		}
		for (int o = 32; o > 0; o >>= 1) {
			nProj += __shfl_xor(nProj, o, 64);
			m0 |= __shfl_xor(m0, o, 64); m1 |= __shfl_xor(m1, o, 64); m2 |= __shfl_xor(m2, o, 64); m3 |= __shfl_xor(m3, o, 64);
		}
		if (lane == 0) {
			const Cand out = {score, sumScale, sumAngle, hi - lo, (uint32_t)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3)), nProj};
			cand[c] = out;
		}
	}
}

struct Pick { float score; uint32_t id; }; // id == ~0u: none
// the order of the stable sort by decreasing score: ties keep ascending id; a NaN score sorts as -infinity
__device__ __forceinline__ float sort_score(float s) { return s != s ? -INFINITY : s; }
__device__ __forceinline__ bool before(const Pick& a, const Pick& b) {
	if (b.id == ~0u) return a.id != ~0u;
	if (a.id == ~0u) return false;
	return a.score > b.score || (a.score == b.score && a.id < b.id);
}

// one wave per image A of the range
__global__ __launch_bounds__(256) void select_kernel(uint32_t a0, uint32_t a1, uint32_t nImages, const Cam* cams, uint32_t nCalibrated, const Cand* cand,
                                                     DevParams p, DevOut out) {
	const uint32_t A = a0 + blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (A >= a1) return;
	const uint32_t M = (uint32_t)p.nMaxViews;
	if (!(cams[A].w > 0)) {
		if (lane == 0) { out.status[A] = 3; out.nCandidates[A] = 0; out.nNeighbors[A] = 0; out.nSrcs[A] = 0; }
		return;
	}
	const Cand* row = cand + (size_t)(A - a0) * nImages;
	uint32_t nCand = 0;
	for (uint32_t B = lane; B < nImages; B += 64) nCand += row[B].points >= 3 && row[B].nProj > 0; // Scene.cpp:613, :633
	for (int o = 32; o > 0; o >>= 1) nCand += __shfl_xor(nCand, o, 64);
	// Scene.cpp:656: the points list and the number of neighbours before the filter
	const uint32_t need = (uint32_t)max(0, min(p.nMinViews, (int)nCalibrated - 1));
	if (out.nPts[A] <= 3 || nCand < need) {
		if (lane == 0) { out.status[A] = 1; out.nCandidates[A] = nCand; out.nNeighbors[A] = 0; out.nSrcs[A] = 0; }
		return;
	}
	Pick prev = {0.f, ~0u};
	uint32_t k = 0;
	for (; k < M; ++k) {
		Pick best = {0.f, ~0u};
		for (uint32_t B = lane; B < nImages; B += 64) {
			const Cand c = row[B];
			if (c.points < 3 || c.nProj == 0) continue;
			const float n = (float)c.points, scale = c.sumScale / n, angle = c.sumAngle / n, area = (float)c.cells / 256.f;
			if (area < p.minArea || !(scale >= p.minScale && scale < p.maxScale) || !(angle >= p.minAngle && angle < p.maxAngle)) continue; // :670-672
			const Pick me = {sort_score(c.score * area), B};
			if (prev.id != ~0u && !before(prev, me)) continue; // taken in an earlier round
			if (before(me, best)) best = me;
		}
		for (int o = 32; o > 0; o >>= 1) {
			Pick other;
			other.score = __shfl_xor(best.score, o, 64); other.id = __shfl_xor(best.id, o, 64);
			if (before(other, best)) best = other;
		}
		if (best.id == ~0u) break;
		prev = best;
		if (lane == 0) {
			const Cand c = row[best.id];
			const float n = (float)c.points, area = (float)c.cells / 256.f;
			const size_t o = (size_t)A * M + k;
			out.nbId[o] = best.id; out.nbPoints[o] = c.points; out.nbScale[o] = c.sumScale / n; out.nbAngle[o] = c.sumAngle / n;
			out.nbArea[o] = area; out.nbScore[o] = c.score * area;
		}
	}
	if (lane != 0) return;
	// SceneDensify.cpp:362-367: neighbours in score order while #images <= number-views and score >= the bound
	uint32_t nSrc = 0;
	if (k) {
		const float fMin = fmaxf(out.nbScore[(size_t)A * M] * (p.minScoreRatio * 0.1f), p.minScore);
		for (uint32_t i = 0; i < k; ++i) {
			const size_t o = (size_t)A * M + i;
			if ((p.numberViews && (int)nSrc + 1 > p.numberViews) || out.nbScore[o] < fMin) break;
			out.srcScale[o] = fabsf(out.nbScale[o] - 1.f) >= 0.15f ? out.nbScale[o] : 1.f; // >= 15 %: the view is resampled (DepthMap.h:233-238)
			++nSrc;
		}
	}
	out.status[A] = nSrc ? 0 : 2; out.nCandidates[A] = nCand; out.nNeighbors[A] = k; out.nSrcs[A] = nSrc;
}

inline unsigned grid_for(unsigned long long n) { return (unsigned)std::min<unsigned long long>(std::max<unsigned long long>((n + 255) / 256, 1), 65536); }
inline int bits_for(unsigned long long maxKey) { int b = 1; while (b < 32 && (maxKey >> b)) ++b; return b; }

int select_views_impl(const ViewSelectInput& in, const ViewSelectParams& p, const ViewSelectOutput& out, ViewSelectCounters& st, Reclaimer* rec, hipStream_t s,
                      std::string& err) {
	st = ViewSelectCounters();
	char msg[200];
	auto refuse = [&](const char* m) { err = m; return 1; };
	const uint32_t nI = in.nImages;
	const unsigned long long nP = in.nPoints;
	if (nI == 0 || nI >= 65536) { snprintf(msg, sizeof msg, "select_views: %u images (1 to 65535 expected)", nI); return refuse(msg); }
	if (p.nMaxViews < 1 || p.nMaxViews > 64) { snprintf(msg, sizeof msg, "select_views: n_max_views is %d (1 to 64 expected)", p.nMaxViews); return refuse(msg); }
	if (p.nMinViews < 0 || p.nMinPointViews < 0 || p.numberViews < 0) return refuse("select_views: a negative count among the parameters");
	if (nP >= 0xFFFFFFFFull) return refuse("select_views: 2^32 - 1 points or more");
	const uint32_t M = (uint32_t)p.nMaxViews;
	// ---- validation and the host side of the plan: nothing has reached the device yet ----
	std::vector<Cam> cams(nI);
	uint32_t nCal = 0;
	for (uint32_t i = 0; i < nI; ++i) {
		Cam& c = cams[i];
		c = Cam();
		if (in.wh[2 * i] <= 0 || in.wh[2 * i + 1] <= 0) continue; // uncalibrated
		c.w = in.wh[2 * i]; c.h = in.wh[2 * i + 1];
		for (int q = 0; q < 9; ++q) { c.K[q] = in.K[9 * (size_t)i + q]; c.R[q] = in.R[9 * (size_t)i + q]; }
		for (int q = 0; q < 3; ++q) c.C[q] = in.C[3 * (size_t)i + q];
		bool finite = true;
		for (int q = 0; q < 9; ++q) finite = finite && std::isfinite(c.K[q]) && std::isfinite(c.R[q]);
		for (int q = 0; q < 3; ++q) finite = finite && std::isfinite(c.C[q]);
		if (!finite) { snprintf(msg, sizeof msg, "select_views: the camera of image %u has an entry that is not finite", i); return refuse(msg); }
		++nCal;
	}
	unsigned long long nE = 0;
	for (unsigned long long v = 0; v < nP; ++v) {
		nE += in.nViews[v];
		if (nE >= (1ull << 32)) return refuse("select_views: 2^32 view entries or more");
	}
	std::vector<uint32_t> first(nP + 1), vertOf(nE), nValid(nP);
	std::vector<unsigned long long> pairsOf(nI, 0); // records per image A
	unsigned long long skipped = 0;
	{
		uint32_t e = 0;
		for (unsigned long long v = 0; v < nP; ++v) {
			if (!std::isfinite(in.xyz[3 * v]) || !std::isfinite(in.xyz[3 * v + 1]) || !std::isfinite(in.xyz[3 * v + 2])) {
				snprintf(msg, sizeof msg, "select_views: point %llu has a coordinate that is not finite", v);
				return refuse(msg);
			}
			first[v] = e;
			uint32_t ok = 0;
			for (uint32_t k = 0; k < in.nViews[v]; ++k, ++e) {
				const uint32_t id = in.viewIds[e];
				if (k && id <= in.viewIds[e - 1]) {
					snprintf(msg, sizeof msg, "select_views: the view ids of point %llu are not strictly ascending", v);
					return refuse(msg);
				}
				vertOf[e] = (uint32_t)v;
				if (id < nI && cams[id].w > 0) ++ok; else ++skipped;
			}
			nValid[v] = ok;
			if (ok > 1)
				for (uint32_t j = first[v]; j < e; ++j) {
					const uint32_t id = in.viewIds[j];
					if (id < nI && cams[id].w > 0) pairsOf[id] += ok - 1;
				}
		}
		first[nP] = e;
	}
	st.skipped = skipped;
	unsigned long long totalPairs = 0;
	for (uint32_t i = 0; i < nI; ++i) totalPairs += pairsOf[i];
	st.pairs = totalPairs;
	const uint32_t E = (uint32_t)nE;
	const bool wantPoints = out.pointsFirst && out.pointIds;

	// ---- the fixed part of the work space ----
	const unsigned long long kMaxRecords = 0x7FFFFFFFull; // per range: record offsets and indices are 32 bits, with room to spare
	auto sort_temp = [](unsigned long long items, int bits) { // what the library's sort asks for at exactly this size
		size_t bytes = 0;
		hipcub::DoubleBuffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
		(void)hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k, v, (size_t)std::max<unsigned long long>(items, 1), 0, bits);
		return bytes;
	};
	size_t tempBytes = sort_temp(E, bits_for(nI));
	{
		size_t scanB = 0;
		(void)hipcub::DeviceScan::ExclusiveSum(nullptr, scanB, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)std::max<uint32_t>(E, 1));
		tempBytes = std::max(tempBytes, scanB);
	}
	const size_t tempGuess = std::max(tempBytes, sort_temp(std::min(totalPairs, kMaxRecords), 32)); // for the budget; the ranges' own sizes follow
	const size_t e4 = (size_t)std::max<uint32_t>(E, 1) * 4, nm = (size_t)nI * M * 4;
	Carve fx;
	const size_t oCam = fx((size_t)nI * sizeof(Cam)), oXyz = fx(std::max<size_t>(nP, 1) * 12), oFirst = fx((nP + 1) * 4), oIds = fx(e4), oVert = fx(e4),
	             oNValid = fx(std::max<size_t>(nP, 1) * 4), oKeyA0 = fx(e4), oKeyA1 = fx(e4), oValA0 = fx(e4), oValA1 = fx(e4), oDepth = fx(e4),
	             oCnt = fx(e4), oOff = fx(e4), oPF = fx(((size_t)nI + 1) * 8), oPid = fx(wantPoints ? e4 : 0),
	             oStatus = fx((size_t)nI * 4), oSeen = fx((size_t)nI * 4), oPts = fx((size_t)nI * 4), oNC = fx((size_t)nI * 4), oNN = fx((size_t)nI * 4),
	             oNS = fx((size_t)nI * 4), oAvg = fx((size_t)nI * 4), oNbId = fx(nm), oNbPts = fx(nm), oNbScale = fx(nm), oNbAngle = fx(nm), oNbArea = fx(nm),
	             oNbScore = fx(nm), oSrcScale = fx(nm);
	size_t freeB = 0, totalB = 0;
	bool knowFree = hipMemGetInfo(&freeB, &totalB) == hipSuccess;
	if (!knowFree) (void)hipGetLastError();
	if (knowFree && fx.size > freeB && rec && rec->reclaim()) { knowFree = hipMemGetInfo(&freeB, &totalB) == hipSuccess; if (!knowFree) (void)hipGetLastError(); }
	if (knowFree && fx.size > freeB) {
		snprintf(msg, sizeof msg, "select_views: the cloud needs %.1f MiB of device memory, more than is free", fx.size / 1048576.0);
		return refuse(msg);
	}
	// ---- the ranges of images: a range's records (record 16 B, key and index twice for the sort's double buffer) and its table of pairs
	// stay within half of the free device memory; HCMVS_SELECT_CHUNK=<images> forces the size of a range ----
	auto range_bytes = [&](unsigned long long records, unsigned long long images) { return records * 32 + images * (unsigned long long)nI * sizeof(Cand) + tempGuess + 7 * 256; };
	const unsigned long long budget = knowFree ? (freeB / 2 > fx.size ? freeB / 2 - fx.size : 0) : ~0ull;
	unsigned long long forced = 0;
	if (const char* env = getenv("HCMVS_SELECT_CHUNK")) { const long long f = atoll(env); if (f > 0) forced = (unsigned long long)f; }
	std::vector<uint32_t> bounds(1, 0);
	unsigned long long maxRecords = 0, maxImages = 0;
	for (uint32_t a = 0; a < nI;) {
		unsigned long long recs = 0, imgs = 0;
		while (a + imgs < nI) {
			const unsigned long long r2 = recs + pairsOf[a + imgs];
			if (imgs && (forced ? imgs >= forced : (range_bytes(r2, imgs + 1) > budget || r2 > kMaxRecords))) break;
			recs = r2; ++imgs;
		}
		if (recs > kMaxRecords) {
			snprintf(msg, sizeof msg, "select_views: image %u alone shares 2^31 or more (point, view) records", a);
			return refuse(msg);
		}
		maxRecords = std::max(maxRecords, recs); maxImages = std::max(maxImages, imgs);
		if (recs) tempBytes = std::max(tempBytes, sort_temp(recs, bits_for(imgs * nI)));
		a += (uint32_t)imgs;
		bounds.push_back(a);
	}
	Carve rg;
	const size_t r4 = (size_t)std::max<unsigned long long>(maxRecords, 1) * 4;
	const size_t oKey0 = rg(r4), oKey1 = rg(r4), oVal0 = rg(r4), oVal1 = rg(r4), oRec = rg(r4 * 4), oCand = rg((size_t)maxImages * nI * sizeof(Cand)), oTemp = rg(tempBytes);
	if (knowFree && fx.size + rg.size > freeB) {
		snprintf(msg, sizeof msg, "select_views: one range of images needs %.1f MiB of device memory, more than is free", (fx.size + rg.size) / 1048576.0);
		return refuse(msg);
	}
	st.chunks = bounds.size() - 1;

	// ---- device ----
	DevBuf fixed(rec), range(rec); // freed on return
	if (fixed.reserve(fx.size, s) != hipSuccess || range.reserve(rg.size, s) != hipSuccess) { err = "select_views: out of device memory"; return 2; }
	st.deviceBytes = fx.size + rg.size;
	char *b = fixed.get(), *rb = range.get();
	hipEvent_t ev[2] = {nullptr, nullptr};
	auto fail = [&](const char* what) {
		err = what;
		(void)hipStreamSynchronize(s); // fixed and range are freed on return
		(void)hipGetLastError();
		for (auto& e : ev) if (e) (void)hipEventDestroy(e);
		return 2;
	};
	if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess) return fail("select_views: event creation failed");
	Cam* dCam = (Cam*)(b + oCam);
	float *dXyz = (float*)(b + oXyz), *dDepth = (float*)(b + oDepth);
	uint32_t *dFirst = (uint32_t*)(b + oFirst), *dIds = (uint32_t*)(b + oIds), *dVert = (uint32_t*)(b + oVert), *dNValid = (uint32_t*)(b + oNValid),
	         *dCnt = (uint32_t*)(b + oCnt), *dOff = (uint32_t*)(b + oOff), *dPid = (uint32_t*)(b + oPid);
	unsigned long long* dPF = (unsigned long long*)(b + oPF);
	DevOut d;
	d.status = (int32_t*)(b + oStatus); d.nSeen = (uint32_t*)(b + oSeen); d.nPts = (uint32_t*)(b + oPts); d.nCandidates = (uint32_t*)(b + oNC);
	d.nNeighbors = (uint32_t*)(b + oNN); d.nSrcs = (uint32_t*)(b + oNS); d.avgDepth = (float*)(b + oAvg); d.nbId = (uint32_t*)(b + oNbId);
	d.nbPoints = (uint32_t*)(b + oNbPts); d.nbScale = (float*)(b + oNbScale); d.nbAngle = (float*)(b + oNbAngle); d.nbArea = (float*)(b + oNbArea);
	d.nbScore = (float*)(b + oNbScore); d.srcScale = (float*)(b + oSrcScale);
	if (hipMemcpyAsync(dCam, cams.data(), (size_t)nI * sizeof(Cam), hipMemcpyHostToDevice, s) != hipSuccess ||
	    hipMemcpyAsync(dFirst, first.data(), (nP + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
	    (nP && (hipMemcpyAsync(dXyz, in.xyz, nP * 12, hipMemcpyHostToDevice, s) != hipSuccess ||
	            hipMemcpyAsync(dNValid, nValid.data(), nP * 4, hipMemcpyHostToDevice, s) != hipSuccess)) ||
	    (E && (hipMemcpyAsync(dIds, in.viewIds, (size_t)E * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
	           hipMemcpyAsync(dVert, vertOf.data(), (size_t)E * 4, hipMemcpyHostToDevice, s) != hipSuccess)) ||
	    hipMemsetAsync(b + oNbId, 0, oSrcScale + ((nm + 255) & ~(size_t)255) - oNbId, s) != hipSuccess) // the seven image x M arrays are adjacent
		return fail("select_views: upload failed");
	(void)hipEventRecord(ev[0], s);
	const uint32_t minPV = (uint32_t)std::min<long long>(p.nMinPointViews, nCal); // Scene.cpp:562-563
	const unsigned waveGrid = (nI + 3) / 4;                                      // four waves, four images per block
	// the entries by image, each image's in ascending vertex index
	hipcub::DoubleBuffer<uint32_t> keyA((uint32_t*)(b + oKeyA0), (uint32_t*)(b + oKeyA1)), valA((uint32_t*)(b + oValA0), (uint32_t*)(b + oValA1));
	if (E) {
		hipLaunchKernelGGL(entry_kernel, dim3(grid_for(E)), kBlock, 0, s, E, dIds, dVert, dXyz, dCam, nI, keyA.Current(), valA.Current(), dDepth);
		if (hipGetLastError() != hipSuccess) return fail("select_views: launch failed");
		size_t tb = tempBytes;
		if (hipcub::DeviceRadixSort::SortPairs(rb + oTemp, tb, keyA, valA, (size_t)E, 0, bits_for(nI), s) != hipSuccess) return fail("select_views: sort failed");
	}
	hipLaunchKernelGGL(image_kernel, dim3(waveGrid), kBlock, 0, s, nI, E, keyA.Current(), valA.Current(), dDepth, dVert, dFirst, minPV, d.nSeen, d.nPts, d.avgDepth,
	                   (const unsigned long long*)nullptr, (uint32_t*)nullptr);
	if (hipGetLastError() != hipSuccess) return fail("select_views: launch failed");
	std::vector<uint32_t> hPts(nI);
	if (wantPoints) { // the lists' offsets: a scan of nImages counts on the host
		if (hipMemcpyAsync(hPts.data(), d.nPts, (size_t)nI * 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
			return fail("select_views: device failure");
		out.pointsFirst[0] = 0;
		for (uint32_t i = 0; i < nI; ++i) out.pointsFirst[i + 1] = out.pointsFirst[i] + hPts[i];
		if (hipMemcpyAsync(dPF, out.pointsFirst, ((size_t)nI + 1) * 8, hipMemcpyHostToDevice, s) != hipSuccess) return fail("select_views: upload failed");
		if (out.pointsFirst[nI]) {
			hipLaunchKernelGGL(image_kernel, dim3(waveGrid), kBlock, 0, s, nI, E, keyA.Current(), valA.Current(), dDepth, dVert, dFirst, minPV, d.nSeen, d.nPts,
			                   d.avgDepth, dPF, dPid);
			if (hipGetLastError() != hipSuccess) return fail("select_views: launch failed");
		}
	}
	DevParams dp;
	dp.nMinViews = p.nMinViews; dp.nMinPointViews = p.nMinPointViews; dp.nMaxViews = p.nMaxViews; dp.numberViews = p.numberViews;
	dp.optimAngle = p.optimAngleDeg * 3.14159265f / 180.f; dp.minAngle = p.minAngleDeg * 3.14159265f / 180.f; dp.maxAngle = p.maxAngleDeg * 3.14159265f / 180.f;
	dp.minArea = p.minArea; dp.minScale = p.minScale; dp.maxScale = p.maxScale; dp.minScoreRatio = p.minScoreRatio; dp.minScore = p.minScore;
	Cand* dCand = (Cand*)(rb + oCand);
	Rec* dRec = (Rec*)(rb + oRec);
	for (size_t c = 0; c + 1 < bounds.size(); ++c) {
		const uint32_t a0 = bounds[c], a1 = bounds[c + 1];
		unsigned long long recs = 0;
		for (uint32_t a = a0; a < a1; ++a) recs += pairsOf[a];
		const uint32_t nRec = (uint32_t)recs, nCells = (a1 - a0) * nI; // < 2^32: both factors are below 2^16
		hipcub::DoubleBuffer<uint32_t> keys((uint32_t*)(rb + oKey0), (uint32_t*)(rb + oKey1)), vals((uint32_t*)(rb + oVal0), (uint32_t*)(rb + oVal1));
		if (nRec) {
			hipLaunchKernelGGL(count_kernel, dim3(grid_for(E)), kBlock, 0, s, E, dIds, dVert, dNValid, dCam, nI, a0, a1, dCnt);
			if (hipGetLastError() != hipSuccess) return fail("select_views: launch failed");
			size_t tb = tempBytes;
			if (hipcub::DeviceScan::ExclusiveSum(rb + oTemp, tb, dCnt, dOff, (size_t)E, s) != hipSuccess) return fail("select_views: scan failed");
			hipLaunchKernelGGL(emit_kernel, dim3(grid_for(E)), kBlock, 0, s, E, dIds, dVert, dFirst, dXyz, dCam, nI, a0, a1, dOff, nRec, minPV, dp.optimAngle,
			                   keys.Current(), vals.Current(), dRec);
			if (hipGetLastError() != hipSuccess) return fail("select_views: launch failed");
			tb = tempBytes;
			if (hipcub::DeviceRadixSort::SortPairs(rb + oTemp, tb, keys, vals, (size_t)nRec, 0, bits_for((unsigned long long)nCells), s) != hipSuccess)
				return fail("select_views: sort failed");
		}
		hipLaunchKernelGGL(segment_kernel, dim3(grid_for(256ull * ((nCells + 3) / 4))), kBlock, 0, s, nCells, nRec, keys.Current(), vals.Current(), dRec, dCand);
		if (hipGetLastError() != hipSuccess) return fail("select_views: launch failed");
		hipLaunchKernelGGL(select_kernel, dim3((a1 - a0 + 3) / 4), kBlock, 0, s, a0, a1, nI, dCam, nCal, dCand, dp, d);
		if (hipGetLastError() != hipSuccess) return fail("select_views: launch failed");
	}
	(void)hipEventRecord(ev[1], s);
	const size_t i4 = (size_t)nI * 4;
	if (hipMemcpyAsync(out.status, d.status, i4, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(out.nSeen, d.nSeen, i4, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipMemcpyAsync(out.avgDepth, d.avgDepth, i4, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipMemcpyAsync(out.nCandidates, d.nCandidates, i4, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipMemcpyAsync(out.nNeighbors, d.nNeighbors, i4, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(out.nSrcs, d.nSrcs, i4, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipMemcpyAsync(out.nbId, d.nbId, nm, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(out.nbPoints, d.nbPoints, nm, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipMemcpyAsync(out.nbScale, d.nbScale, nm, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(out.nbAngle, d.nbAngle, nm, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipMemcpyAsync(out.nbArea, d.nbArea, nm, hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(out.nbScore, d.nbScore, nm, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    hipMemcpyAsync(out.srcScale, d.srcScale, nm, hipMemcpyDeviceToHost, s) != hipSuccess ||
	    (wantPoints && out.pointsFirst[nI] && hipMemcpyAsync(out.pointIds, dPid, (size_t)out.pointsFirst[nI] * 4, hipMemcpyDeviceToHost, s) != hipSuccess) ||
	    hipStreamSynchronize(s) != hipSuccess)
		return fail("select_views: device failure");
	(void)hipEventElapsedTime(&st.ms, ev[0], ev[1]);
	for (auto& e : ev) (void)hipEventDestroy(e);
	return 0;
}
} // namespace

// the host side allocates (the plan, the messages): an allocation that fails must not leave through the C entry as an exception
int select_views_device(const ViewSelectInput& in, const ViewSelectParams& p, const ViewSelectOutput& out, ViewSelectCounters& st, Reclaimer* rec, hipStream_t s,
                        std::string& err) {
	try {
		return select_views_impl(in, p, out, st, rec, s, err);
	} catch (const std::exception&) {
		(void)hipStreamSynchronize(s);
		try { err = "select_views: out of host memory"; } catch (...) {}
		return 2;
	}
}

} // namespace hcmvs

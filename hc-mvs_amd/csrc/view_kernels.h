/* hc-mvs_amd/csrc/view_kernels.h -- scene-wide view selection on the device (view_kernels.hip) */
#ifndef HCMVS_VIEW_KERNELS_H
#define HCMVS_VIEW_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "dev_buf.h"
namespace hcmvs {
struct ViewSelectParams {
	int nMinViews = 2, nMinPointViews = 2, nMaxViews = 12, numberViews = 5;
	float optimAngleDeg = 10.f, minAngleDeg = 3.f, maxAngleDeg = 65.f;
	float minArea = 0.01f, minScale = 0.2f, maxScale = 3.2f, minScoreRatio = 0.3f, minScore = 0.f;
};
struct ViewSelectInput {
	uint32_t nImages = 0;
	const int32_t* wh = nullptr;                                  // nImages * 2 (width, height; width 0 = uncalibrated)
	const double *K = nullptr, *R = nullptr, *C = nullptr;        // nImages * 9, 9, 3
	unsigned long long nPoints = 0;
	const float* xyz = nullptr;                                   // nPoints * 3
	const uint32_t *nViews = nullptr, *viewIds = nullptr;         // the view lists as CSR, ids strictly ascending per point
};
// host arrays; M = nMaxViews
struct ViewSelectOutput {
	int32_t* status = nullptr;                                              // nImages
	uint32_t *nSeen = nullptr, *nCandidates = nullptr, *nNeighbors = nullptr, *nSrcs = nullptr; // nImages
	float* avgDepth = nullptr;                                              // nImages
	uint32_t *nbId = nullptr, *nbPoints = nullptr;                          // nImages * M
	float *nbScale = nullptr, *nbAngle = nullptr, *nbArea = nullptr, *nbScore = nullptr, *srcScale = nullptr; // nImages * M
	unsigned long long* pointsFirst = nullptr;                              // nImages + 1, or null
	uint32_t* pointIds = nullptr;                                           // sum of nViews entries suffice, or null
};
struct ViewSelectCounters {
	unsigned long long pairs = 0, skipped = 0, chunks = 0, deviceBytes = 0;
	float ms = 0.f;
};
// Scene::SelectNeighborViews (Scene.cpp:545-661) + FilterNeighborViews (:665-678) + the InitViews cut (SceneDensify.cpp:362-367) for every
// image of the scene, with the arithmetic of DESIGN.md section 5 (D12).  0 = ok, 1 = refused (err names the first offender; nothing has
// reached the device, or the work space exceeds the free device memory), 2 = device failure (err says which)
int select_views_device(const ViewSelectInput& in, const ViewSelectParams& p, const ViewSelectOutput& out, ViewSelectCounters& st, Reclaimer* rec,
                        hipStream_t s, std::string& err);
}
#endif

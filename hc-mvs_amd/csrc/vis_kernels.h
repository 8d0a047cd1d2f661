/* hc-mvs_amd/csrc/vis_kernels.h -- the visibility filter of a finished cloud on the device (vis_kernels.hip) */
#ifndef HCMVS_VIS_KERNELS_H
#define HCMVS_VIS_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "dev_buf.h"
namespace hcmvs {
struct VisCounters {
	unsigned long long pairs = 0, skipped = 0, fallback = 0, candidates = 0, hits = 0, deviceBytes = 0;
	float ms = 0.f;
};
// Scene::PointCloudFilter's visibility sums (SceneDensify.cpp:4188-4320): for every (point, view) pair the points inside the view's cone
// around the ray through the point vote.  Points as CSR (n_views, view_ids); cameras per image: wh (width, height; width 0 = uncalibrated),
// K / R (9 doubles), C (3 doubles).  visibility: n host int32 out.  The device work space in scratch (the caller's, grown as needed).
// 0 = ok, 1 = bad argument, 2 = device failure (err says which)
int point_cloud_visibility_device(unsigned long long n, const float* xyz, const uint32_t* nViews, const uint32_t* viewIds, uint32_t nImages,
                                  const int32_t* wh, const double* K, const double* R, const double* C, int32_t* visibility, VisCounters& st,
                                  DevBuf& scratch, hipStream_t s, std::string& err);
}
#endif

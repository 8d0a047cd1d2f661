/* hc-mvs_amd/csrc/init_kernels.h -- the initial depth / normal maps rasterised on the device (init_kernels.hip) from the tables and the
 * tile lists of init_plan.h */
#ifndef HCMVS_INIT_KERNELS_H
#define HCMVS_INIT_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "init_plan.h"
namespace hcmvs {
// a splat point as the device reads it: its clamped 5 x 5 block (half open) and its depth
struct InitSplatBox { int32_t x0, y0, x1, y1; float d; };

struct InitRaster {
	int W = 0, H = 0, tilesX = 0, tilesY = 0;
	float fx = 0, fy = 0, cx = 0, cy = 0;     // triangles only
	const uint32_t *first = nullptr, *items = nullptr; // the tile lists (device)
	float *depth = nullptr, *normal = nullptr;         // W*H, W*H*3 (device): every pixel is written
	unsigned long long* counters = nullptr;            // [0] += covered pixels, [1] += cover hits (device, zero before the launch)
};
// one workgroup per tile; a pixel takes the last entry of its tile's list that covers it
void launch_init_triangles(const InitRaster& r, const InitFace* faces, hipStream_t s);
void launch_init_splats(const InitRaster& r, const InitSplatBox* points, hipStream_t s);
}
#endif

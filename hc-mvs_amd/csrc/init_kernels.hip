/*
 * hc-mvs_amd/csrc/init_kernels.hip -- the initial depth / normal maps on the device (gfx950): the pixel loops of
 * TriangulatePoints2DepthMap (DepthMap.cpp:1886-1931, rasteriser Types.inl:2474-2606) and of the 5 x 5 splat (SceneDensify.cpp:789-806)
 * over the tables the host sets up (init_plan.h, tri_init.cpp).
 *
 * The host loops let a later face / point overwrite an earlier one.  Here a pixel belongs to one lane: the workgroup of a tile
 * (kInitTileW x kInitTileH pixels, one wave per stretch of rows) walks the tile's list -- ascending, built on the host -- and every lane
 * keeps the last hit of its pixels in registers, then stores depth and normal once.  No atomics on the maps, no memset, no order
 * between workgroups.  The edge functions are 64-bit integers (16 * W is 2^16 at 4K), the depth is the host's float expression term by
 * term (the file is built with -ffp-contract=off; float division is correctly rounded).  No fp64 and no camera maths.
 */
#include "init_kernels.h"

namespace hcmvs {
namespace {

constexpr int kRowsPerLane = 4;                       // a wave owns kRowsPerLane consecutive rows of the tile, a lane one column of them
constexpr int kWaves = kInitTileH / kRowsPerLane;     // waves per workgroup
static_assert(kInitTileW == 64, "one lane per column of the tile");
static_assert(kWaves * kRowsPerLane == kInitTileH, "the waves' rows make up the tile");

__device__ inline unsigned wave_sum(unsigned v) {
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	return v; // lane 0 holds the sum
}

template <bool kTriangles, class Entry>
__global__ __launch_bounds__(kInitTileW* kWaves) void init_raster_kernel(const InitRaster r, const Entry* __restrict__ table) {
	const int tile = (int)blockIdx.x;
	const int x = (tile % r.tilesX) * kInitTileW + (int)threadIdx.x;
	const int yb = (tile / r.tilesX) * kInitTileH + (int)threadIdx.y * kRowsPerLane;
	float z[kRowsPerLane], n0[kRowsPerLane], n1[kRowsPerLane], n2[kRowsPerLane];
#pragma unroll
	for (int k = 0; k < kRowsPerLane; ++k) z[k] = n0[k] = n1[k] = n2[k] = 0.f;
	unsigned hits = 0;
	const uint32_t b = r.first[tile], e = r.first[tile + 1];
	if constexpr (kTriangles) {
		const float X0x = ((float)x - r.cx) / r.fx; // TransformPointI2C(Point2f)
		const int64_t xs = (int64_t)x << 4;
		for (uint32_t i = b; i < e; ++i) {
			const InitFace& f = table[r.items[i]];
			if (x < f.x0 || x >= f.x1) continue;
			const int64_t DX12 = f.X[0] - f.X[1], DX23 = f.X[1] - f.X[2], DX31 = f.X[2] - f.X[0];
			const int64_t DY12 = f.Y[0] - f.Y[1], DY23 = f.Y[1] - f.Y[2], DY31 = f.Y[2] - f.Y[0];
			const int64_t E1 = f.C[0] - DY12 * xs, E2 = f.C[1] - DY23 * xs, E3 = f.C[2] - DY31 * xs;
#pragma unroll
			for (int k = 0; k < kRowsPerLane; ++k) {
				const int y = yb + k;
				if (y < f.y0 || y >= f.y1) continue;
				const int64_t ys = (int64_t)y << 4;
				if (!(E1 + DX12 * ys > 0 && E2 + DX23 * ys > 0 && E3 + DX31 * ys > 0)) continue;
				const float X0y = ((float)y - r.cy) / r.fy;
				const float zz = 1.f / (f.np[0] * X0x + f.np[1] * X0y + f.np[2] * 1.f);
				if (!(zz > 0.f)) continue; // "due to numerical instability"
				z[k] = zz; n0[k] = f.nn[0]; n1[k] = f.nn[1]; n2[k] = f.nn[2];
				++hits;
			}
		}
	} else {
		for (uint32_t i = b; i < e; ++i) {
			const InitSplatBox& p = table[r.items[i]];
			if (x < p.x0 || x >= p.x1) continue;
#pragma unroll
			for (int k = 0; k < kRowsPerLane; ++k) {
				const int y = yb + k;
				if (y < p.y0 || y >= p.y1) continue;
				z[k] = p.d;
				++hits;
			}
		}
	}
	unsigned covered = 0;
	if (x < r.W) {
#pragma unroll
		for (int k = 0; k < kRowsPerLane; ++k) {
			const int y = yb + k;
			if (y >= r.H) continue;
			const size_t at = (size_t)y * r.W + x;
			r.depth[at] = z[k];
			float* o = r.normal + 3 * at;
			o[0] = n0[k]; o[1] = n1[k]; o[2] = n2[k];
			covered += z[k] > 0.f ? 1u : 0u;
		}
	}
	// one add per wave and counter; the boxes are clamped to the image, so a lane outside it has no hit
	covered = wave_sum(covered);
	hits = wave_sum(hits);
	if (threadIdx.x == 0) {
		if (covered) atomicAdd(r.counters, (unsigned long long)covered);
		if (hits) atomicAdd(r.counters + 1, (unsigned long long)hits);
	}
}

} // namespace

void launch_init_triangles(const InitRaster& r, const InitFace* faces, hipStream_t s) {
	hipLaunchKernelGGL((init_raster_kernel<true, InitFace>), dim3((unsigned)(r.tilesX * r.tilesY)), dim3(kInitTileW, kWaves), 0, s, r, faces);
}
void launch_init_splats(const InitRaster& r, const InitSplatBox* points, hipStream_t s) {
	hipLaunchKernelGGL((init_raster_kernel<false, InitSplatBox>), dim3((unsigned)(r.tilesX * r.tilesY)), dim3(kInitTileW, kWaves), 0, s, r, points);
}

} // namespace hcmvs

/* hc-mvs_amd/csrc/init_plan.h -- what the two initialisations (triangulation, splat) hand to a rasteriser, and the tiling of the image the
 * device rasteriser walks: plain C++ (no HIP).  The host forms (tri_init.cpp, hcmvs_splat_points) and the device forms (init_kernels.hip)
 * consume the same tables, so a table is the complete statement of a raster: a pixel takes the value of the LAST entry of the table that
 * covers it, 0 where none does. */
#ifndef HCMVS_INIT_PLAN_H
#define HCMVS_INIT_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <vector>
#include "carve.h"
namespace hcmvs {

// One face of the triangulation as TImage::RasterizeTriangle sees it (Types.inl:2474-2606).  A pixel (x, y) of the box is covered when
//   C[0] + DX12 * 16y - DY12 * 16x > 0,  C[1] + DX23 * 16y - DY23 * 16x > 0,  C[2] + DX31 * 16y - DY31 * 16x > 0     (64-bit integers)
// with DX12 = X[0] - X[1], DX23 = X[1] - X[2], DX31 = X[2] - X[0] and DY.. alike, and when its depth
//   z = 1.f / (np[0] * ((float)x - cx) / fx + np[1] * ((float)y - cy) / fy + np[2] * 1.f)   (left to right, nothing fused)
// is > 0; it then gets z and the normal nn.
struct InitFace {
	int64_t X[3], Y[3];     // 28.4 fixed point, in the order the rasteriser takes the vertices (the counter-clockwise face reversed)
	int64_t C[3];           // edge constants, the top-left bias applied
	int32_t x0, y0, x1, y1; // the pixels the host loop visits: whole 8 x 8 blocks over the vertices' box, clamped to the image; half open
	float nn[3], np[3];     // unit normal (camera space); normal / (normal . first corner)
	int32_t index, pad_;    // the face's place in the host loop's order (faces that loop skips are not in the table)
};

struct InitTriTable {
	std::vector<InitFace> faces;
	int nUsed = 0;                     // points that entered the triangulation
	float lo = 0.f, hi = 0.f;          // depth range of the projected points (not yet widened)
	float fx = 0, fy = 0, cx = 0, cy = 0; // the camera as the rasteriser reads it
};

// One point of the splat (SceneDensify.cpp:789-806): its pixel and its depth; it covers the 5 x 5 block around (x, y) clamped to the image
struct InitSplat { int32_t x, y; float d; };

struct InitBox { int32_t x0, y0, x1, y1; }; // half open; empty when x0 >= x1 or y0 >= y1

inline InitBox face_box(const InitFace& f) { return {f.x0, f.y0, f.x1, f.y1}; }
inline InitBox splat_box(const InitSplat& p, int W, int H) {
	const int64_t sx = (int64_t)p.x - 2 > 0 ? (int64_t)p.x - 2 : 0, sy = (int64_t)p.y - 2 > 0 ? (int64_t)p.y - 2 : 0;
	const int64_t ex = (int64_t)p.x + 2 < W - 1 ? (int64_t)p.x + 2 : W - 1, ey = (int64_t)p.y + 2 < H - 1 ? (int64_t)p.y + 2 : H - 1;
	if (sx > ex || sy > ey) return {0, 0, 0, 0};
	return {(int32_t)sx, (int32_t)sy, (int32_t)ex + 1, (int32_t)ey + 1};
}

// the per-point set-up of the splat: double-precision projection to an integer centre and a float depth.  dMin / dMax not yet widened
inline void splat_plan(const double* K, const double* R, const double* C, const float* pts, int n, std::vector<InitSplat>& out, float* dMin, float* dMax) {
	out.resize((size_t)n);
	float dmin = 3.402823466e+38f, dmax = 0.f;
	for (int i = 0; i < n; ++i) {
		const double X[3] = {pts[3 * i] - C[0], pts[3 * i + 1] - C[1], pts[3 * i + 2] - C[2]};
		double cam[3];
		for (int r = 0; r < 3; ++r) cam[r] = R[r * 3] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2];
		const int x = (int)std::floor(K[2] + K[0] * (cam[0] / cam[2]) + .5);
		const int y = (int)std::floor(K[5] + K[4] * (cam[1] / cam[2]) + .5);
		const float d = (float)cam[2];
		out[(size_t)i] = {x, y, d};
		if (dmin > d) dmin = d;
		if (dmax < d) dmax = d;
	}
	*dMin = dmin; *dMax = dmax;
}

// The device rasteriser's tiling: one workgroup per tile of kInitTileW x kInitTileH pixels (one row stretch per wave), and per tile the
// entries of the table whose box meets it, in ascending order (CSR: the list of tile t is items[first[t] .. first[t + 1])).
constexpr int kInitTileW = 64, kInitTileH = 16;

struct InitTiling {
	int tilesX = 0, tilesY = 0;
	std::vector<uint32_t> first, items;
};

// box(i): the InitBox of entry i (already clamped to the image).  Returns false when the lists would pass 2^31 entries.
template <class BoxOf>
inline bool bin_tiles(int W, int H, size_t n, BoxOf box, InitTiling& t) {
	t.tilesX = (W + kInitTileW - 1) / kInitTileW; t.tilesY = (H + kInitTileH - 1) / kInitTileH;
	const size_t nTiles = (size_t)t.tilesX * t.tilesY;
	std::vector<uint64_t> count(nTiles + 1, 0);
	auto span = [&](const InitBox& b, int& tx0, int& ty0, int& tx1, int& ty1) {
		if (b.x0 >= b.x1 || b.y0 >= b.y1) return false;
		tx0 = b.x0 / kInitTileW; tx1 = (b.x1 - 1) / kInitTileW; ty0 = b.y0 / kInitTileH; ty1 = (b.y1 - 1) / kInitTileH;
		return true;
	};
	int tx0, ty0, tx1, ty1;
	for (size_t i = 0; i < n; ++i)
		if (span(box(i), tx0, ty0, tx1, ty1))
			for (int ty = ty0; ty <= ty1; ++ty)
				for (int tx = tx0; tx <= tx1; ++tx) ++count[(size_t)ty * t.tilesX + tx + 1];
	for (size_t k = 0; k < nTiles; ++k) count[k + 1] += count[k];
	if (count[nTiles] >> 31) return false;
	t.first.assign(count.begin(), count.end());
	t.items.resize((size_t)count[nTiles]);
	std::vector<uint32_t> at(t.first.begin(), t.first.end() - 1);
	for (size_t i = 0; i < n; ++i)
		if (span(box(i), tx0, ty0, tx1, ty1))
			for (int ty = ty0; ty <= ty1; ++ty)
				for (int tx = tx0; tx <= tx1; ++tx) t.items[at[(size_t)ty * t.tilesX + tx]++] = (uint32_t)i;
	return true;
}

// The one device buffer of a call: two 64-bit counters (covered pixels, cover hits; they arrive zeroed with the tables), the table, the lists
struct InitLayout {
	size_t counters = 0, table = 0, first = 0, items = 0, bytes = 0;
};
inline InitLayout init_layout(size_t tableBytes, size_t nTiles, size_t nEntries) {
	Carve cv;
	InitLayout l;
	l.counters = cv(2 * sizeof(uint64_t));
	l.table = cv(tableBytes);
	l.first = cv((nTiles + 1) * sizeof(uint32_t));
	l.items = cv(nEntries * sizeof(uint32_t));
	l.bytes = cv.size;
	return l;
}

} // namespace hcmvs
#endif

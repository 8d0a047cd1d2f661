// C face of hc-mvs_amd/csrc/init_plan.h and of the triangulation's set-up (tri_init.cpp, compiled into this shim) for
// tests/init_plan_lib.py (ctypes).  Links nothing of the library and nothing of HIP.
#include "../hc-mvs_amd/csrc/tri_init.h"

#include <string.h>

using namespace hcmvs;

extern "C" {
int ip_face_bytes() { return (int)sizeof(InitFace); }
void ip_tile_shape(int* w, int* h) { *w = kInitTileW; *h = kInitTileH; }

// the face table of triangulate_plan: returns the number of faces (-1: no point in front of the camera), writes at most cap of them;
// info: nUsed; range: lo, hi; cam: fx, fy, cx, cy
int ip_tri_plan(int W, int H, const double* K, const double* R, const double* C, const float* xyz, int n, float avgDepth, int addCorners, InitFace* out, int cap,
                int* nUsed, float* range, float* cam) {
	InitTriTable t;
	if (!triangulate_plan(W, H, K, R, C, xyz, n, avgDepth, addCorners != 0, t)) return -1;
	*nUsed = t.nUsed; range[0] = t.lo; range[1] = t.hi;
	cam[0] = t.fx; cam[1] = t.fy; cam[2] = t.cx; cam[3] = t.cy;
	const int nf = (int)t.faces.size();
	if (nf) memcpy(out, t.faces.data(), sizeof(InitFace) * (size_t)(nf < cap ? nf : cap));
	return nf;
}

// the splat's table: xy[2 n], d[n], and the clamped blocks box[4 n] (half open) for a W x H image; range: min, max depth (not widened)
void ip_splat_plan(int W, int H, const double* K, const double* R, const double* C, const float* xyz, int n, int32_t* xy, float* d, int32_t* box, float* range) {
	std::vector<InitSplat> t;
	splat_plan(K, R, C, xyz, n, t, &range[0], &range[1]);
	for (int i = 0; i < n; ++i) {
		xy[2 * i] = t[(size_t)i].x; xy[2 * i + 1] = t[(size_t)i].y; d[i] = t[(size_t)i].d;
		const InitBox b = splat_box(t[(size_t)i], W, H);
		box[4 * i] = b.x0; box[4 * i + 1] = b.y0; box[4 * i + 2] = b.x1; box[4 * i + 3] = b.y1;
	}
}

// bin_tiles over n boxes (x0, y0, x1, y1): returns the number of list entries (-1: refused); fills first (tilesX * tilesY + 1) and items
// when capItems suffices
long long ip_bin(int W, int H, const int32_t* box, int n, int* tilesX, int* tilesY, uint32_t* first, uint32_t* items, long long capItems) {
	InitTiling t;
	if (!bin_tiles(W, H, (size_t)n, [&](size_t i) { return InitBox{box[4 * i], box[4 * i + 1], box[4 * i + 2], box[4 * i + 3]}; }, t)) return -1;
	*tilesX = t.tilesX; *tilesY = t.tilesY;
	memcpy(first, t.first.data(), t.first.size() * sizeof(uint32_t));
	if ((long long)t.items.size() <= capItems && !t.items.empty()) memcpy(items, t.items.data(), t.items.size() * sizeof(uint32_t));
	return (long long)t.items.size();
}

// InitLayout: offsets of counters, table, first, items, and the total
void ip_layout(unsigned long long tableBytes, unsigned long long nTiles, unsigned long long nEntries, unsigned long long* out) {
	const InitLayout l = init_layout((size_t)tableBytes, (size_t)nTiles, (size_t)nEntries);
	out[0] = l.counters; out[1] = l.table; out[2] = l.first; out[3] = l.items; out[4] = l.bytes;
}
}

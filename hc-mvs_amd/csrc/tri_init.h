/* hc-mvs_amd/csrc/tri_init.h -- see tri_init.cpp */
#ifndef HCMVS_TRI_INIT_H
#define HCMVS_TRI_INIT_H
#include "init_plan.h"
namespace hcmvs {
// Everything the initialisation does before its pixel loop: projection, exact-duplicate removal, Bowyer-Watson, the corner depths, one
// plane and one set of edge constants per face (init_plan.h).  avgDepth <= 0: use the mean depth of the points.  Returns false when no
// point projects in front of the camera.
bool triangulate_plan(int W, int H, const double* K, const double* R, const double* C, const float* xyz, int n, float avgDepth,
                      bool addCorners, InitTriTable& out);
// the host rasteriser over that table: depth[W*H], normal[W*H*3] (camera space), 0 where no face covers
void raster_triangles(const InitTriTable& t, int W, int H, float* depth, float* normal);
// both; dMin/dMax: depth range of the projected points (not yet widened).  Writes nothing when it returns false.
bool triangulate_init(int W, int H, const double* K, const double* R, const double* C, const float* xyz, int n, float avgDepth,
                      bool addCorners, float* depth, float* normal, float* dMin, float* dMax);
}
#endif

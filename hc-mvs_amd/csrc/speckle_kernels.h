/* hc-mvs_amd/csrc/speckle_kernels.h -- launches of speckle_kernels.hip */
#ifndef HCMVS_SPECKLE_KERNELS_H
#define HCMVS_SPECKLE_KERNELS_H
#include <hip/hip_runtime.h>
#include "speckle_plan.h"
namespace hcmvs {

// Five launches on s, whatever the maps hold: label the tiles, merge their borders, add the sizes up at the roots, apply, sum the
// counters.  items / first: device copies of the tile table (nItems, nItems + 1 entries); partials: one per tile; result: zeroed by the
// caller, its counters are written by the last launch and its error word is raised by a loop that ran past its bound.
void launch_speckle(const SpeckleItem* items, const int32_t* first, int nItems, int nTiles, float thr, uint32_t speckleSize, SpecklePartial* partials,
                    SpeckleResult* result, hipStream_t s);

} // namespace hcmvs
#endif

/* hc-mvs_amd/csrc/handoff_host.h -- the hand-off between two pyramid levels on host buffers (handoff_host.cpp) */
#ifndef HCMVS_HANDOFF_HOST_H
#define HCMVS_HANDOFF_HOST_H
#include "handoff_device.h"
namespace hcmvs {
// one image: every pixel of dstDepth (dw * dh) and dstNormal (dw * dh * 3) is written; r takes the counters.  Init mode: *dMin / *dMax are
// written unless the map holds no valid depth (returns false).  Hint mode: they are read and widened.
bool handoff_host(int mode, const HandoffGeom& g, const float* srcDepth, const float* srcNormal, float* dstDepth, float* dstNormal, float* dMin, float* dMax,
                  HandoffResult& r);
}
#endif

/* hc-mvs_amd/csrc/handoff_kernels.h -- the hand-off between pyramid levels on the device (handoff_kernels.hip) over the plan of
 * handoff_plan.h */
#ifndef HCMVS_HANDOFF_KERNELS_H
#define HCMVS_HANDOFF_KERNELS_H
#include <hip/hip_runtime.h>
#include "handoff_plan.h"
namespace hcmvs {
// Every destination pixel of every item is written.  nBlocks = first[nItems]; partials: nBlocks entries (device), one per workgroup of
// the pass; a second, small launch (one workgroup per item) reduces them into results[0 .. nItems) and, in hint mode, folds the range
// again behind a NaN (handoff_device.h)
void launch_handoff(int mode, const HandoffItem* items, const int32_t* first, int nItems, int nBlocks, HandoffResult* partials, HandoffResult* results,
                    hipStream_t s);
}
#endif

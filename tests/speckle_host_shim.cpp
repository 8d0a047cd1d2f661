// C face of hc-mvs_amd/csrc/speckle_host.h (the CPU form of the speckle filter, a sequential flood fill) for tests/test_speckle_ref.py
// (ctypes, through tests/speckle_lib.py).  Built with g++ alone: nothing of the library, nothing of HIP.
#include "../hc-mvs_amd/csrc/speckle_host.h"

using namespace hcmvs;

extern "C" {
// the CPU form on host arrays (normal, conf, labels: null = not given).  counters: valid, removed, segments, small, largest
void ss_host(int w, int h, float* depth, float* normal, float* conf, int32_t* labels, float thr, uint32_t speckleSize, uint64_t* counters) {
	SpeckleResult r = SpeckleResult();
	speckle_host(w, h, depth, normal, conf, labels, thr, speckleSize, r);
	counters[0] = r.valid; counters[1] = r.removed; counters[2] = r.segments; counters[3] = r.small; counters[4] = r.largest;
}

} // extern "C"

/* hc-mvs_amd/csrc/prior_kernels.h -- depth priors from planes fitted to a labelled region, on the device (prior_kernels.hip) */
#ifndef HCMVS_PRIOR_KERNELS_H
#define HCMVS_PRIOR_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "dev_buf.h"
#include "prior_gen_plan.h"
namespace hcmvs {

// what hcmvs_get_plane_prior_trace reads of the last call: the scratch keeps the stage map and the fitting set
struct PriorGenTrace {
	bool valid = false;
	int w = 0, h = 0;
	uint64_t n0 = 0;             // fitting-set samples whose pixel and assignment the scratch holds (0: the call ended before S4)
	PriorGenLayout lay;
	std::vector<int32_t> rounds; // 6 per round: winner or -1, cnt_0 .. cnt_3, valid candidates
	std::vector<int32_t> clusters; // 4 per round (S4c): occupied cells, components, size of the largest, accepted; zeros without a winner
	std::vector<int32_t> refits;   // 6 per round (S4r): steps solved, steps kept, cnt_0 .. cnt_3 of the final plane; zeros without a winner
	std::vector<float> refitPlanes; // 4 per round: the final n, d; zeros without a winner
	hcmvs_plane_prior_refit_stats refitStats = {0, 0}; // what hcmvs_get_plane_prior_refit_stats reads
};

// DESIGN.md section 5, D13.  region: the view's region mask as the ignore-mask kernel writes it (u8 per pixel, 0 = INSIDE the region), or
// null (no region).  The arguments have passed prior_gen_check.  All device pointers; planes (64 entries, or null) and st are the host's.
// Waits for the stream several times (stage sizes, one winner per round -- with clustering one more per round that has a winner, with
// refit_iters > 0 up to refit_iters + 1 more --, the plane reductions).  0 = ok, 2 = device failure (err says which)
int generate_plane_prior_device(int w, int h, const double K[9], const uint8_t* region, const float* depth, const float* normal, const float* conf,
                                const hcmvs_plane_prior_params& p, float* prior, float* priorNormal, hcmvs_prior_plane* planes, hcmvs_plane_prior_stats& st,
                                DevBuf& scratch, PriorGenTrace& trace, hipStream_t s, std::string& err);
}
#endif

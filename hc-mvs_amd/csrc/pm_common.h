/*
 * hc-mvs_amd/csrc/pm_common.h -- what the host API and the gfx950 kernels share: the structures of an estimate (pm_types.h), those of a
 * sweep launch and the launch wrappers.
 */
#ifndef HCMVS_PM_COMMON_H
#define HCMVS_PM_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility> // std::integer_sequence: the kernel tables of pm_kernels.hip
#include "pm_types.h" // after the runtime header: EstConst::dn is a float4*
#include "sweep_plan.h"

namespace hcmvs {

struct SweepSync {
	int32_t* ticket;   // [kMaxBatch] next row of every image of the batch, counted through the sweeps of the launch (row + sweep * rows)
	int32_t* rowsDone; // [kMaxBatch] rows every image has finished, counted through the sweeps of the launch
	int32_t* error;    // set non-zero when a worker times out
	unsigned long long* evals;  // [0] ScorePixel calls of the sequential algorithm, [1] evaluations issued (incl. speculative), [2] patch taps of [0],
	                            // [4 .. 8) view spread: slots scored, slots accepted, slots dropped (depth <= 0), candidates outside the view's map,
	                            // [8 .. 10) depth prior: evaluations that blended the term, pixels with a usable prior,
	                            // [10 .. 12) geometric consistency: evaluations that blended the term, pixels with a weight
};

// what all sweep launches of one call share
struct SweepArgs {
	const EstConst* dItems;
	int nItems, maxRows;
	SweepSync sync;
	int lag, affinity;
};

// launch wrappers (pm_kernels.hip)
void launch_gray_to_u8(const float* gray, uint8_t* out, int n, hipStream_t s);
void launch_bgr_to_u8(const uint8_t* bgr, uint8_t* out, int n, hipStream_t s);
void launch_gradient_map(const uint8_t* g8, uint8_t* gra, int W, int H, hipStream_t s);
void launch_median3(const float* in, float* out, int W, int H, hipStream_t s);
void launch_apply_mask(const uint8_t* keep, float* depth, float* normal, int n, hipStream_t s); // DepthData::ApplyIgnoreMask
void launch_quads(const float* gray, float4* out, int W, int H, hipStream_t s); // 2 x 2 footprint layout of a source view
// prior: the item has an active depth prior (the PriorItem behind c.views is set): the PRIOR instance of the score kernel
// geo: the item has the geometric-consistency term active (the GeoItem behind it is set): the GEO instance (never together with prior)
void launch_score_pass(const EstConst& c, const float* depthIn, const float* normalIn, unsigned long long* evals,
                       hipStream_t s, bool prior = false, bool geo = false);
// the sweeps-only entry: the working state from maps that hold depth, normal and conf = the score; nothing is scored
void launch_import_state(const EstConst& c, const float* depthIn, const float* normalIn, const float* confIn, hipStream_t s);
bool launch_sweep(const SweepArgs& a, const SweepLaunch& l, hipStream_t s); // false: the library holds no instance l.v (nothing is launched)
void launch_end_pass(const EstConst& c, int finalPass, float* depth, float* normal, float* conf, hipStream_t s);

} // namespace hcmvs
#endif

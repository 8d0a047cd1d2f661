/*
 * include/hcmvs_hip.h -- C-ABI of the MI355X-native PatchMatch densifier (libhcmvs_hip.so).
 *
 * The reference (Liaoyongjian1/HC-MVS, an OpenMVS v1.1.1 fork) has no FFI for this path: it is private
 * C++ inside libMVS.  Each entry point below replaces one of its seams; paths are
 * under /root/reference/frame_main/libs/MVS/:
 *
 *   hcmvs_upload_view / hcmvs_set_view_device
 *        <- DepthMapsData::InitViews (SceneDensify.cpp:336-397): per view gray f32 image + camera
 *   hcmvs_estimate / hcmvs_estimate_device
 *        <- bool DepthMapsData::EstimateDepthMap(int it_external, IIndex idxImage)
 *           (SceneDensify.h:63, SceneDensify.cpp:758-1072) with DepthEstimator (DepthMap.cpp:386-1738)
 *   hcmvs_filter   <- bool DepthMapsData::FilterDepthMap(DepthData&, const IIndexArr&, bool bAdjust)
 *                     (SceneDensify.h:69, SceneDensify.cpp:3006-3259)
 *   hcmvs_filter_sequence <- void Scene::DenseReconstructionFilter(void*) (SceneDensify.cpp:4100-4185), the filter stage over all images
 *   hcmvs_fuse     <- void DepthMapsData::FuseDepthMaps(PointCloud&, bool, bool)
 *                     (SceneDensify.h:70, SceneDensify.cpp:3265-3495)
 *   hcmvs_params   <- the OPTDENSE::* globals (DepthMap.cpp:67-143) this path reads
 *
 * Conventions: plain pointers and sizes; caller owns every buffer; int status (0 = ok) instead of bool;
 * no exceptions cross the boundary; hcmvs_last_error() gives the message of the last failure on a
 * context.  One estimate may be in flight per context (the reference serialises EstimateDepthMap under
 * a semaphore of count 1, SceneDensify.cpp:3895); contexts on different devices run concurrently.
 * There is NO CPU fallback: every compute entry fails with HCMVS_ERR_NO_DEVICE when no gfx950 device is
 * usable.
 *
 * Layouts: images/maps row-major; gray f32 in [0,1]; depth f32 (0 = invalid); normal 3 x f32 interleaved,
 * camera space, unit, facing the camera; conf f32 (score in [0,2] between outer iterations, confidence in
 * [0,1] after the last one); K, R 3x3 row-major f64, C 3 x f64, x_cam = R (X - C), pixel = K x_cam / z
 * with pixel centres at integer coordinates (Camera.h:150-151).
 */
#ifndef HCMVS_HIP_H
#define HCMVS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HCMVS_MAX_VIEWS 16 /* source views per estimate (reference cap nMaxViews = 12, DepthMap.cpp:73) */

enum {
	HCMVS_OK = 0,
	HCMVS_ERR_NO_DEVICE = 1,   /* no usable gfx950 device / HIP runtime failure at create */
	HCMVS_ERR_INVALID = 2,     /* bad argument (null pointer, unknown view id, size mismatch, V out of range) */
	HCMVS_ERR_HIP = 3,         /* a HIP call failed */
	HCMVS_ERR_TIMEOUT = 4,     /* a sweep worker gave up waiting on its predecessor row (never expected) */
	HCMVS_ERR_CAPACITY = 5,    /* output buffer too small (fuse) */
	HCMVS_ERR_INTERNAL = 6     /* a bounded loop of a kernel ran past its bound (the speckle filter's union-find; never expected) */
};

typedef struct hcmvs_ctx hcmvs_ctx;

/* replaces the OPTDENSE globals read on this path; hcmvs_default_params() fills the reference defaults */
typedef struct {
	int32_t adapthalfwin;           /* --n-adapthalfwin 1..10, patch half window (DepthMap.cpp:455-461; beyond 7 = more than the reference's 64 taps) */
	int32_t n_estimation_iters;     /* --n-EstimationIters, inner sweeps (SceneDensify.cpp:949) */
	int32_t it_external;            /* outer iteration index of this call (SceneDensify.cpp:758) */
	int32_t n_external_iters;       /* --n-EstimationIters-external; the end pass runs on the last one */
	int32_t propagate_halfwin;      /* --n-propagatehalfwin (DepthMap.cpp:1071), <= 7 */
	int32_t propagate_step;         /* --n-propagatestep (DepthMap.cpp:1072), >= 1 */
	int32_t n_random_iters;         /* nRandomIters (DepthMap.cpp:120) */
	float ncc_threshold_keep;       /* fNCCThresholdKeep (DepthMap.cpp:117) */
	float random_depth_ratio;       /* fRandomDepthRatio */
	float random_angle1_deg;        /* fRandomAngle1Range */
	float random_angle2_deg;        /* fRandomAngle2Range */
	float random_smooth_depth;      /* fRandomSmoothDepth */
	float random_smooth_normal_deg; /* fRandomSmoothNormal */
	float random_smooth_bonus;      /* fRandomSmoothBonus */
	float photometric_flow;         /* --n-photometric_flow: every score is scaled by (1-pf) (DepthMap.cpp:892) */
	uint32_t seed;                  /* counter-based RNG seed; same seed => same maps on any schedule */
	int32_t median_blur;            /* 1: 3x3 median on the depth map first (SceneDensify.cpp:859) */
} hcmvs_params;

typedef struct {
	uint64_t evals;       /* ScorePixel evaluations of the sequential algorithm (each covers all source views) */
	uint64_t evals_issued;/* evaluations the device executed, including discarded speculative ones */
	uint64_t tap_evals;   /* sum over `evals` of the patch taps each one samples per source view (36/49/64) */
	float ms_score;       /* device time of the init-score pass (HIP events on the context's stream) */
	float ms_sweeps;      /* device time of all propagate/refine sweeps */
	float ms_sweep_avg;   /* ms_sweeps / n_sweeps: average duration of one sweep */
	float ms_end;         /* device time of median/end/export kernels */
	float ms_total;
	int32_t n_sweeps;
	int32_t n_sweep_launches; /* kernel launches the n_sweeps sweeps ran in: a batch whose rows fill the chip four times over (12 or more images of 1080p) runs all its sweeps in one launch */
} hcmvs_stats;

void hcmvs_default_params(hcmvs_params* p);

/* device = HIP device ordinal.  Fails with HCMVS_ERR_NO_DEVICE when it is not a usable GPU. */
int hcmvs_create(int device, hcmvs_ctx** out);
void hcmvs_destroy(hcmvs_ctx* ctx);
const char* hcmvs_last_error(const hcmvs_ctx* ctx);
/* stream: a hipStream_t owned by the caller (NULL = the context's own stream).  All work is enqueued
 * on it; the *_device entry points return without synchronising. */
int hcmvs_set_stream(hcmvs_ctx* ctx, void* stream);
int hcmvs_synchronize(hcmvs_ctx* ctx);

/* register view `id` (any number < 65536): host buffers are copied to the device.  bgr (B,G,R u8) is
 * optional: it feeds the gradient map exactly as the reference does (SceneDensify.cpp:586) and the fused
 * colours; without it the gradient map is taken from round(gray*255).  gray may be NULL when bgr is given: such a view can be
 * filtered and fused (camera, colours, gradient map) but not estimated or matched against -- what a rank of a multi-GPU job
 * holds of the images the other ranks estimate. */
int hcmvs_upload_view(hcmvs_ctx* ctx, uint32_t id, int32_t width, int32_t height, const float* gray,
                      const uint8_t* bgr_or_null, const double K[9], const double R[9], const double C[3]);
/* same, but gray/bgr already live in device memory and stay owned by the caller */
int hcmvs_set_view_device(hcmvs_ctx* ctx, uint32_t id, int32_t width, int32_t height, const float* d_gray,
                          const uint8_t* d_bgr_or_null, const double K[9], const double R[9], const double C[3]);
/* DepthData::ViewData::ScaleImage (DepthMap.h:233-238) + Image::GetCamera for the new size (SceneDensify.cpp:372-374,
 * Image.cpp:194-209): register view dst_id as view src_id resampled by `scale` on the device -- cv::resize(image, Size(),
 * scale, scale, scale > 1 ? INTER_CUBIC : INTER_AREA) on the f32 gray image, new size cvRound(w * scale) x cvRound(h * scale),
 * K rescaled by max(w', h') / max(w, h) like the reference's normalised K.  The reference resamples a source view when its
 * average footprint scale differs from the reference image's by 15 % or more; |scale - 1| < 0.15 is refused as it is there.
 * The new view has no colour image (source views are only matched against). */
int hcmvs_rescale_view(hcmvs_ctx* ctx, uint32_t src_id, uint32_t dst_id, float scale);
/* size and camera of a registered view (any pointer may be NULL) */
int hcmvs_get_view_info(hcmvs_ctx* ctx, uint32_t id, int32_t* width, int32_t* height, double K[9]);
/* copy the f32 gray image of a registered view to a host buffer of w*h floats */
int hcmvs_get_view_gray(hcmvs_ctx* ctx, uint32_t id, float* out);
int hcmvs_release_view(hcmvs_ctx* ctx, uint32_t id);
/* copy the u8 gradient map of a view (SceneDensify.cpp:581-595 InitGraMap) to a host buffer of w*h bytes */
int hcmvs_get_gradient_map(hcmvs_ctx* ctx, uint32_t id, uint8_t* out);

/* --ignore-mask-label (DepthEstimator::ImportIgnoreMask, DepthMap.cpp:319-348): a keep-mask for view `id` as a REFERENCE view.
 * labels: a 16-bit label image of lw x lh (any size; resampled to the view's size with cv::resize INTER_NEAREST on the device);
 * a pixel is ignored when its label equals one of ignore[0..n_ignore) (values outside 0..65535 never match).  Every estimate of
 * the view then applies the mask to its initial maps (depth, normal = 0) before the median and leaves the ignored pixels out of
 * every pass: they end the estimate with the median's depth, normal 0 and conf 0, and cost no evaluation.  Source views and views
 * made by hcmvs_rescale_view ignore masks; registering the view again or hcmvs_release_view drops it.  labels == NULL removes
 * the mask.  Blocking. */
int hcmvs_set_ignore_mask(hcmvs_ctx* ctx, uint32_t id, const uint16_t* labels, int32_t lw, int32_t lh, const int32_t* ignore,
                          int32_t n_ignore);
/* the same with the label image in DEVICE memory (ignore stays a host array) */
int hcmvs_set_ignore_mask_device(hcmvs_ctx* ctx, uint32_t id, const uint16_t* d_labels, int32_t lw, int32_t lh, const int32_t* ignore,
                                 int32_t n_ignore);
/* copy the keep-mask of view `id` (1 = estimated, 0 = ignored; all 1 without a mask) to a host buffer of w*h bytes */
int hcmvs_get_ignore_mask(hcmvs_ctx* ctx, uint32_t id, uint8_t* keep);

/* One EstimateDepthMap call for reference view ref_id against src_ids[0..n_src): [median] -> init score
 * -> n_estimation_iters sweeps -> end pass if it_external == n_external_iters-1.
 * depth (w*h), normal (w*h*3), conf (w*h) are in/out HOST buffers: on entry the initial maps (zeros +
 * splatted sparse depths at it_external 0, SceneDensify.cpp:783-808; the previous maps later).  Blocking. */
int hcmvs_estimate(hcmvs_ctx* ctx, uint32_t ref_id, const uint32_t* src_ids, int32_t n_src,
                   const hcmvs_params* params, float d_min, float d_max, float* depth, float* normal, float* conf);
/* the same on DEVICE buffers, asynchronous on the context's stream */
int hcmvs_estimate_device(hcmvs_ctx* ctx, uint32_t ref_id, const uint32_t* src_ids, int32_t n_src,
                          const hcmvs_params* params, float d_min, float d_max, float* d_depth, float* d_normal,
                          float* d_conf);
/* A batch of independent EstimateDepthMap calls (different reference images, the same options, source-view counts
 * of one class: up to 8, or 9-16) in ONE set of launches: the sweep kernel interleaves the rows of all items, so the images fill each
 * other's wavefront ramps (the reference overlaps images with two worker threads, SceneDensify.cpp:3699).
 * Every item produces exactly the maps hcmvs_estimate_device would produce for it with seed + seed_offset.
 * 1 <= n_items <= HCMVS_MAX_BATCH. */
#define HCMVS_MAX_BATCH 64
typedef struct {
	uint32_t ref_id;
	const uint32_t* src_ids;
	int32_t n_src;
	uint32_t seed_offset;  /* added to params->seed for this item */
	float d_min, d_max;
	float *d_depth, *d_normal, *d_conf; /* DEVICE in/out maps of this item */
	/* optional (NULL = none): DEVICE maps (w*h depth, w*h*3 normal) of the up-sampled coarser level.  With them, the last
	 * sweep of the last outer iteration also tries that estimate at every pixel, accepting it when it is at most 0.1 worse
	 * than the current score -- the extra hypothesis of the fork's `restore` variant (restore/libs/MVS/DepthMap.cpp:1527-1549) */
	const float *d_hint_depth, *d_hint_normal;
} hcmvs_batch_item;
int hcmvs_estimate_batch_device(hcmvs_ctx* ctx, const hcmvs_batch_item* items, int32_t n_items, const hcmvs_params* params);
/* synchronises, then reports counters/timings of the last estimate (summed over the items of a batch) */
int hcmvs_get_stats(hcmvs_ctx* ctx, hcmvs_stats* out);

/* ---- view spread (DensifyPointCloud --n-viewspread; DepthEstimator::ProcessPixel, DepthMap.cpp:1504-1608) --------------------
 * From outer iteration 1 on (params->it_external >= 1), after its refinement trials, every pixel that did not leave through the
 * full-random branch also tries the estimates its SOURCE views' own maps hold around the place it projects to: per source view, in
 * the estimate's view order, the four neighbours of the projected pixel in that view's map (depth brought into the reference camera,
 * normal as stored, CorrectNormal, accepted when the score improves); they also become the pixel's smoothness set.  What the
 * reference leaves undefined is fixed in DESIGN.md section 5, D10. */
/* switch view spread on (non-zero) or off for the estimates that follow.  Default 0 (the reference's default is 1): every caller that
 * does not ask for it computes what it computed before the feature existed. */
int hcmvs_set_viewspread(hcmvs_ctx* ctx, int32_t on);
/* the maps view `id` offers when it is a source view of an estimate with view spread on: DEVICE memory of the view's image size
 * (depth w*h, normal w*h*3 in the view's camera frame, conf w*h: the score, as an estimate leaves it between outer iterations),
 * caller-owned, not copied, read by the estimates that follow.  All three NULL removes them; registering the view again or
 * hcmvs_release_view drops them.  A view without maps, and a view made by hcmvs_rescale_view (refused here: there are no maps of
 * its size), never spreads.  An estimate must not write the maps it reads: hcmvs_estimate_batch_device fails with
 * HCMVS_ERR_INVALID when the in/out maps of an item overlap the spread maps of a source view of any item of the same call.
 * The registry has a second consumer: the geometric-consistency term (hcmvs_set_geo_params, below) reads the depth and the normal map
 * a source view offers here, under the same rules. */
int hcmvs_set_spread_maps_device(hcmvs_ctx* ctx, uint32_t id, const float* d_depth, const float* d_normal, const float* d_conf);
/* counters of the view spread of the last estimate (summed over the items of a batch and its sweeps); synchronises */
typedef struct {
	uint64_t slots_scored;       /* hypotheses taken from source views' maps and scored (they are part of hcmvs_stats::evals) */
	uint64_t slots_accepted;     /* ... that replaced the pixel's estimate */
	uint64_t slots_dropped;      /* not scored: their depth in the reference camera was not positive */
	uint64_t candidates_outside; /* candidate pixels beyond the source view's map (a source view smaller than the reference image) */
} hcmvs_spread_stats;
int hcmvs_get_spread_stats(hcmvs_ctx* ctx, hcmvs_spread_stats* out);

/* ---- depth priors (DensifyPointCloud --n-para_prior / --sigma-prior / --n-photo2geo; ScorePixelImage, DepthMap.cpp:941-954) -----
 * A reference view may carry a prior depth map.  While it is active, every ScorePixel evaluation of an estimate of that view blends,
 * per source view and before the two best views are taken,
 *     dd = |prior - depth| / prior,  wP = exp(-dd^2 / (2 sigma_prior^2)),  score = score * (1 - para_prior) + 2 * (1 - wP) * para_prior
 * at the pixels whose prior is finite and > 0; a view that failed (thRobust) is not blended.  The prior of view `id` is ACTIVE in an
 * estimate of `id` when one is registered, para_prior > 0 and params->it_external >= photo2geo; without an active prior every call
 * computes exactly what it computes without this section.  The library consumes the map; hcmvs_generate_plane_prior_device (below)
 * makes one from planes fitted to a labelled region, any other kind (a coarser level, a rendering) is the caller's.  DESIGN.md
 * section 5, D11 pins the association and the validity rule. */
typedef struct {
	float para_prior;   /* --n-para_prior: weight of the term, 0 .. 1 */
	float sigma_prior;  /* --sigma-prior: width of the relative depth difference, > 0 */
	int32_t photo2geo;  /* --n-photo2geo: first outer iteration that blends the term, >= 0 */
} hcmvs_prior_params;
/* the reference's defaults: 0.5, 0.2, 2 (DensifyPointCloud.cpp:162, :175, :183) */
void hcmvs_default_prior_params(hcmvs_prior_params* p);
/* for the estimates that follow.  Refused, with nothing changed: para_prior outside [0, 1] or not finite, sigma_prior not > 0 (or not
 * finite), photo2geo < 0. */
int hcmvs_set_prior_params(hcmvs_ctx* ctx, const hcmvs_prior_params* p);
/* the prior of view `id` as a REFERENCE view: w*h floats in DEVICE memory at the view's size, caller-owned, not copied, read (never
 * written) by the estimates that follow.  NULL removes it; registering the view again or hcmvs_release_view drops it.  A view made by
 * hcmvs_rescale_view is refused: only a reference view's prior is ever read. */
int hcmvs_set_depth_prior_device(hcmvs_ctx* ctx, uint32_t id, const float* d_prior);
/* the same from a HOST buffer, into a copy the context owns.  Blocking. */
int hcmvs_set_depth_prior(hcmvs_ctx* ctx, uint32_t id, const float* prior);
/* An item with an active prior is refused (HCMVS_ERR_INVALID, nothing enqueued) together with the `restore` hint in effect or with
 * view spread doing work for it: the authors run priors with --n-viewspread 0, and the hint belongs to the other binary. */

/* The reference's extra sweeps (SceneDensify.cpp:983-1031): sweeps first_sweep .. first_sweep + n_sweeps - 1 on maps that are the
 * state an estimate leaves between outer iterations (depth, normal, conf = the score) -- no mask application, no median, no init-score
 * pass; the sweep index decides direction and random stream as in an estimate; then the end pass as in hcmvs_estimate_batch_device.
 * params->n_estimation_iters is not used; the hint of an item is never offered.  Refused: first_sweep < 0, n_sweeps < 1, and
 * first_sweep + n_sweeps > HCMVS_MAX_SWEEP_INDEX + 1 (a sweep's random stream is it_external * 64 + 1 + index). */
#define HCMVS_MAX_SWEEP_INDEX 62
int hcmvs_estimate_sweeps_batch_device(hcmvs_ctx* ctx, const hcmvs_batch_item* items, int32_t n_items, const hcmvs_params* params,
                                       int32_t first_sweep, int32_t n_sweeps);
/* counters of the prior term of the last estimate (summed over the items of a batch); synchronises */
typedef struct {
	uint64_t evals_prior;  /* evaluations that blended the term (they are part of hcmvs_stats::evals) */
	uint64_t pixels_prior; /* estimated pixels of the items with an active prior whose prior is usable (finite and > 0) */
} hcmvs_prior_stats;
int hcmvs_get_prior_stats(hcmvs_ctx* ctx, hcmvs_prior_stats* out);

/* ---- geometric consistency (DensifyPointCloud --geo-consistency) -------------------------------------------
 * A hypothesis is also scored by whether the source views' own depth maps agree with it.  While the term is active for an estimate,
 * every ScorePixel evaluation blends, per source view j and before the two best views are taken,
 *     score = score * (1 - w) + w * geo
 * where w goes by the reference pixel's texture g (the gradient map): para_tapa where g < txthreshold, else para_tapa2 where
 * g < txthreshold2, else 0 (such a pixel is evaluated as without this section); and geo of the pair (hypothesis, view j): the centre
 * pixel goes through the hypothesis' homography into view j, view j's depth at the nearest pixel there takes that position back into
 * the reference image, e is the distance in pixels to where it started, c the cosine between the hypothesis' normal and view j's
 * normal there;  geo = e / max_px + (1 - c) where e < max_px, 2 elsewhere, and 1 (neutral) where view j offers no maps, the position
 * lies outside its map, its depth there is not finite and > 0 or the point falls behind the reference camera.  A view that failed
 * (thRobust) is not blended.  The maps of view j are those registered with hcmvs_set_spread_maps_device (depth and normal are read;
 * the aliasing refusal of that entry applies unchanged): the caller keeps the previous outer iteration's maps there.
 * The term is ACTIVE for an item when `on` is set, params->it_external >= photo2geo and a source view of the item offers maps;
 * without it every call computes exactly what it computes without this section.  The stored confidence of a blended pixel is the
 * blended score.  Refused (HCMVS_ERR_INVALID, nothing enqueued): a batch in which the term is active for an item while an item has the
 * `restore` hint in effect, view spread doing work, or an active depth prior. */
typedef struct {
	int32_t on;          /* --geo-consistency: 0 = off (the default) */
	float para_tapa;     /* --n-para_tapa: weight where the pixel has low texture, 0 .. 1 */
	float para_tapa2;    /* --n-para_tapa2: weight where the pixel has medium texture, 0 .. 1 */
	float txthreshold;   /* --n-txthreshold */
	float txthreshold2;  /* --n-txthreshold2 */
	int32_t photo2geo;   /* --n-photo2geo: first outer iteration that blends the term, >= 0 */
	float max_px;        /* --geo-max-px: reprojection error in pixels at and beyond which a pair is "worst", > 0 */
} hcmvs_geo_params;
/* off, 0.25, 0.15, 150, 160, 2 (the reference's defaults, DensifyPointCloud.cpp:176-183), 3.0 */
void hcmvs_default_geo_params(hcmvs_geo_params* p);
/* for the estimates that follow.  Refused, with nothing changed: a weight outside [0, 1] or not finite, a threshold that is not finite,
 * max_px not finite and > 0, photo2geo < 0. */
int hcmvs_set_geo_params(hcmvs_ctx* ctx, const hcmvs_geo_params* p);
/* counters of the term of the last estimate (summed over the items of a batch); synchronises */
typedef struct {
	uint64_t evals_geo;  /* evaluations that blended the term (they are part of hcmvs_stats::evals) */
	uint64_t pixels_geo; /* estimated pixels with a weight > 0 of the items for which the term was active */
} hcmvs_geo_stats;
int hcmvs_get_geo_stats(hcmvs_ctx* ctx, hcmvs_geo_stats* out);

/* ---- plane priors (DepthMapsData::GenerateDepthPrior, SceneDensify.cpp:1550-1950, restated without CGAL) ------------------------------
 * Planes are fitted inside a labelled region of a half-finished depth map and rendered into a prior depth map, which pulls the
 * textureless pixels of the region onto them (the section above consumes it).  The rule -- samples, planarity, spacing and outliers,
 * plane detection in rounds of 256 counter-based candidates, optionally the largest connected component of the winner's inliers
 * (cluster_mul), plane frames and image quads, rendering -- is DESIGN.md section 5, D13;
 * all of it runs on the device in the camera frame of the view.  The result depends on (maps, region, params) only: parity with
 * CGAL's randomised Efficient RANSAC is unpinned. */
#define HCMVS_MAX_PRIOR_PLANES 64
typedef struct {
	int32_t region_label;   /* 255: the label a caller hands to hcmvs_set_prior_region (the generate call reads the registered region) */
	float conf_max;         /* 0.18 (SceneDensify.cpp:1625): a sample's score lies below it */
	float planarity_min;    /* 0.3: (l1 - l0) / l2 of a sample's neighbourhood is at least this */
	int32_t n_neighbors;    /* 10, 3 .. 31: neighbourhood of the planarity and of the spacing */
	float probability;      /* 0.01, --ransac-probability: chance of overlooking a plane, inside (0, 1) */
	float min_points_div;   /* 80, --ransac-min-points: a plane has at least n0 / min_points_div samples (and 3) */
	float epsilon_mul;      /* 2, --ransac-epsilon: eps = average spacing * epsilon_mul */
	float normal_threshold; /* 0.25: |plane normal . sample normal| is at least this */
	int32_t max_rounds;     /* 256, 1 .. 4096: rounds of 256 candidates at the most */
	uint64_t seed;          /* of the counter-based candidate stream */
	float cluster_mul;      /* 0 (off), --ransac-cluster: a plane keeps the largest connected component of its inliers on a grid of cells of
	                           average spacing * cluster_mul in the plane; finite and >= 0 */
	int32_t refit_iters;    /* 0 (off), --plane-refit, 0 .. 16: total-least-squares steps on the winner of a round over its inliers in the
	                           eps / 4 band, before the clustering and before anything is assigned.  It lies in
	                           what was the struct's tail padding: the size of the struct is what it was */
} hcmvs_plane_prior_params;
void hcmvs_default_plane_prior_params(hcmvs_plane_prior_params* p);
/* The region of view `id` in which planes are fitted: the pixels whose label equals region_label, from a 16-bit label image of any
 * size on the HOST, resampled with cv::resize INTER_NEAREST as the ignore mask is.  labels == NULL removes the region; registering the
 * view again or hcmvs_release_view drops it.  A view made by hcmvs_rescale_view is refused.  Blocking. */
int hcmvs_set_prior_region(hcmvs_ctx* ctx, uint32_t id, const uint16_t* labels, int32_t lw, int32_t lh, int32_t region_label);
/* region: w*h bytes, 1 = inside (all 0 without a region) */
int hcmvs_get_prior_region(hcmvs_ctx* ctx, uint32_t id, uint8_t* region);
typedef struct {
	float normal[3];       /* unit normal, camera frame: the final normal of its round -- the candidate's, with refit_iters > 0 the last kept step's */
	uint32_t n_inliers;    /* the samples assigned to the plane: cnt_0, with clustering the size of the component that was kept */
	double centre[3];      /* centroid of the inliers, camera frame */
	double quad[8];        /* image quad x0 y0 .. x3 y3: lower-left, lower-right, upper-right, upper-left of the plane frame */
	int32_t box_fallback;  /* 1: a corner fell behind the camera, quad = the box of the inliers' pixels widened by half a pixel */
	int32_t reserved;
} hcmvs_prior_plane;
typedef struct {
	uint64_t region_pixels, samples, planar_samples, fitting_samples; /* the stages S1 .. S3 */
	double avg_spacing_all, avg_spacing; /* the average before the outliers went, and of the fitting set */
	float eps;
	int32_t min_points;
	int32_t rounds, planes;
	uint64_t candidates_valid; /* over all rounds */
	uint64_t prior_pixels;     /* pixels of the prior map that are > 0 */
	float ms_device;           /* first launch to the last, host round trips included */
	float ms_gather, ms_search, ms_rounds, ms_render; /* host clock between the points where the call waits for the stream: S1; S2 + S3
	                                                     (three neighbour searches); S4; S5 + S6 */
	uint64_t device_bytes;     /* scratch of the call */
	float cluster_eps;         /* the cell edge of the clustering, float32(avg_spacing * cluster_mul); 0 with clustering off */
	int32_t cluster_rejects;   /* rounds whose winner was rejected: its largest component was smaller than min_points */
	uint64_t cluster_left;     /* inliers that clustering left unassigned, summed over the accepted rounds */
} hcmvs_plane_prior_stats;
/* The counters of the refit (refit_iters, S4r).  They are a struct of their own, read with hcmvs_get_plane_prior_refit_stats:
 * hcmvs_plane_prior_stats keeps the size and the last field its callers were built against. */
typedef struct {
	int32_t refit_rounds;      /* rounds with at least one kept refit step (0 with refit_iters = 0) */
	int32_t refit_steps;       /* kept refit steps, summed over the rounds */
} hcmvs_plane_prior_refit_stats;
/* The prior of view `id` from its maps in DEVICE memory in the state an estimate leaves between outer iterations (d_conf = the score,
 * lower is better), which are read and never written: every pixel of d_prior (w*h floats) is written, 0 outside the region and where
 * no plane applies; d_prior_normal (w*h*3 floats, or NULL) gets the plane normal turned towards the camera, 0 where the prior is 0.
 * planes (HCMVS_MAX_PRIOR_PLANES entries, or NULL) and stats (or NULL) are HOST buffers; entries past stats->planes are zeroed.  Runs
 * on the context's stream and is blocking (the plane table comes back).  The output feeds hcmvs_set_depth_prior_device unchanged.
 * A pixel whose point ray * depth is not finite in float32 is not a sample.
 * Success with an all-zero prior and no plane: no region registered, no region pixel, fewer than n_neighbors + 1 samples at any stage.
 * HCMVS_ERR_INVALID before anything reaches the device: a null pointer, an unknown view, a K whose last row is not 0 0 1 or that
 * cannot be inverted, probability outside (0, 1), min_points_div / epsilon_mul not > 0 and finite, n_neighbors outside 3 .. 31,
 * max_rounds outside 1 .. 4096, cluster_mul negative, NaN or infinite, refit_iters outside 0 .. 16, an output overlapping an input map
 * or the other output. */
int hcmvs_generate_plane_prior_device(hcmvs_ctx* ctx, uint32_t id, const float* d_depth, const float* d_normal, const float* d_conf,
                                      const hcmvs_plane_prior_params* params, float* d_prior, float* d_prior_normal,
                                      hcmvs_prior_plane* planes, hcmvs_plane_prior_stats* stats);
/* TEST SURFACE.  The decisions of the last hcmvs_generate_plane_prior_device of the context, into HOST buffers (each may be NULL); they are
 * read out of that call's scratch, which the context keeps until the next call, its end, or a shortage of device memory (the trace is then
 * gone: HCMVS_ERR_INVALID for stage / assignment):
 * stage (w*h bytes of the view of that call: 0 outside the region, 1 region, 2 sample, 3 planar, 4 in the fitting set), assignment (w*h
 * int32: the plane of a fitting-set sample, -1 otherwise), rounds (6 int32 per round run: winning candidate or -1, its cnt_0 .. cnt_3,
 * the valid candidates of the round; at most rounds_capacity rounds are written), *n_rounds = the rounds run. */
int hcmvs_get_plane_prior_trace(hcmvs_ctx* ctx, uint8_t* stage, int32_t* assignment, int32_t* rounds, int32_t rounds_capacity,
                                int32_t* n_rounds);
/* TEST SURFACE.  What the clustering (cluster_mul, S4c) decided in every round of the same call, into a HOST buffer (may be NULL): 4 int32
 * per round run -- occupied cells, components, size of the largest component, accepted 0 / 1; at most `capacity` rounds are written,
 * *n_rounds = the rounds run.  A round without a winner is all zeros; with clustering off a round with a winner is 0, 0, cnt_0, 1 (and
 * 0, 1, cnt_0, 1 when the cell edge is not a finite number > 0: all inliers are one component). */
int hcmvs_get_plane_prior_cluster_trace(hcmvs_ctx* ctx, int32_t* clusters, int32_t capacity, int32_t* n_rounds);
/* TEST SURFACE.  What the refit (refit_iters, S4r) decided in every round of the same call, into HOST buffers (each may be NULL): steps, 6
 * int32 per round run -- steps solved, steps kept, cnt_0 .. cnt_3 of the round's final plane --, and planes, 4 floats per round run -- the
 * final n, d; at most `capacity` rounds are written, *n_rounds = the rounds run.  A round without a winner is all zeros; with
 * refit_iters = 0 a round with a winner is 0, 0, the candidate's counts and the candidate's plane. */
int hcmvs_get_plane_prior_refit_trace(hcmvs_ctx* ctx, int32_t* steps, float* planes, int32_t capacity, int32_t* n_rounds);
/* the refit's counters of the last hcmvs_generate_plane_prior_device of the context (zeros before the first call and after a failed one) */
int hcmvs_get_plane_prior_refit_stats(hcmvs_ctx* ctx, hcmvs_plane_prior_refit_stats* out);

/* SceneDensify.cpp:783-808: splat n_points sparse world points (xyz f32) seen by view `id` as 5x5 blocks
 * into host maps depth (w*h) / normal (w*h*3); returns the depth range (min*0.9, max*1.1). Host-side helper. */
int hcmvs_splat_init(hcmvs_ctx* ctx, uint32_t id, const float* points_xyz, int32_t n_points, float* depth,
                     float* normal, float* d_min, float* d_max);
/* the same without a context (size and camera given): pure host code, callable from any thread */
int hcmvs_splat_points(int32_t width, int32_t height, const double K[9], const double R[9], const double C[3],
                       const float* points_xyz, int32_t n_points, float* depth, float* normal, float* d_min, float* d_max);

/* DepthMap.cpp:1796-1936 TriangulatePoints2DepthMap (the default initialisation, nMinViewsTrustPoint >= 2) as
 * DepthMapsData::InitDepthMap uses it (SceneDensify.cpp:522-526): Delaunay-triangulate the projections of the sparse
 * points seen by view `id`, add the four image corners as support points when add_corners != 0 (OPTDENSE::bAddCorners;
 * their depth = distance-weighted mean of the three closest faces), rasterise one plane per face into host maps
 * depth (w*h) / normal (w*h*3, camera space); returns the depth range (min*0.9, max*1.1).  avg_depth <= 0: mean depth
 * of the points (Scene.cpp:565-603).  Host-side helper; hcmvs_triangulate_points is the same without a context. */
int hcmvs_triangulate_init(hcmvs_ctx* ctx, uint32_t id, const float* points_xyz, int32_t n_points, float avg_depth,
                           int32_t add_corners, float* depth, float* normal, float* d_min, float* d_max);
int hcmvs_triangulate_points(int32_t width, int32_t height, const double K[9], const double R[9], const double C[3],
                             const float* points_xyz, int32_t n_points, float avg_depth, int32_t add_corners, float* depth,
                             float* normal, float* d_min, float* d_max);

/* counters of the last hcmvs_triangulate_init_device / hcmvs_splat_init_device call */
typedef struct {
	uint64_t n_used;          /* points that entered the triangulation / were splatted */
	uint64_t n_faces;         /* faces rasterised (splat: 0) */
	uint64_t n_tile_entries;  /* sum of the tile lists' lengths */
	uint64_t covered_pixels;  /* pixels with depth > 0 */
	uint64_t cover_hits;      /* (pixel, face|point) hits; hits - pixels = overwrites the order rule decided */
	float ms_host;            /* set-up on the host (Delaunay, planes, binning) */
	float ms_device;          /* HIP events around the kernel */
	uint64_t device_bytes;    /* the tables and tile lists on the device */
} hcmvs_init_stats;
/* The two initialisations above with the pixel loop on the device: points_xyz is a HOST array, d_depth (w*h) and d_normal (w*h*3) are
 * DEVICE pointers; every pixel of both is written (0 where nothing covers; the splat's normals are 0 everywhere), bit-identical to the
 * host forms called with zero-filled normals.  The per-point / per-face set-up (projection, Delaunay, planes: double precision) runs on
 * the host, only its tables travel -- through page-locked staging of the context.  *d_min / *d_max are final on return; the raster is
 * enqueued on the context's stream, ordered before a following hcmvs_estimate*_device, and NOT synchronised.  Refused before anything
 * reaches the device: null pointers, n_points < 1, an unknown view, a non-finite coordinate, no point in front of the view
 * (triangulation). */
int hcmvs_triangulate_init_device(hcmvs_ctx* ctx, uint32_t id, const float* points_xyz, int32_t n_points, float avg_depth,
                                  int32_t add_corners, float* d_depth, float* d_normal, float* d_min, float* d_max);
int hcmvs_splat_init_device(hcmvs_ctx* ctx, uint32_t id, const float* points_xyz, int32_t n_points, float* d_depth,
                            float* d_normal, float* d_min, float* d_max);
/* waits for the context's stream, then reads the counters of the last of the two calls */
int hcmvs_get_init_stats(hcmvs_ctx* ctx, hcmvs_init_stats* out);

/* cv::resize(src, dst, Size(dst_w, dst_h), 0, 0, INTER_AREA) for an ENLARGING resize of an f32 image with `channels` interleaved
 * channels -- how the fork's `restore` variant brings the previous pyramid level's depth and normal maps to the current size before
 * offering them as the extra hypothesis (restore/libs/MVS/SceneDensify.cpp:523-524; d_hint_depth / d_hint_normal above).  OpenCV's
 * INTER_AREA enlarges with the bilinear kernel and "area mode" coefficients (a destination pixel inside one source pixel copies it,
 * one that straddles two mixes them by the overlap).  Host buffers, host code, no context (once per image and level).  dst_w >= src_w
 * and dst_h >= src_h, else HCMVS_ERR_INVALID. */
int hcmvs_resize_area_up(const float* src, int32_t src_w, int32_t src_h, int32_t channels, float* dst, int32_t dst_w, int32_t dst_h);

/* ---- the hand-off between two levels of the coarse-to-fine schedule (run.sh: levels 3, 2, 2, 1, 1) ---------------------------------
 * The previous level's maps of an image become what the next level starts from, in one of two ways:
 *   HCMVS_HANDOFF_INIT  (--n-initTriangulate 0, SceneDensify.cpp:527-553): they are the initial maps.  Equal sizes: copied; else
 *       cv::resize INTER_CUBIC (Keys kernel A = -0.75, pixel centres aligned, replicated border; any ratio, per axis).  Then a depth
 *       that is not > 0 (NaN included; the cubic kernel undershoots next to holes) becomes 0, and where a depth is left and the normal
 *       has a length it is brought to length 1.  d_min = 0.9f * the smallest, d_max = 1.1f * the largest of ALL cleaned depths, the
 *       zeros included.
 *   HCMVS_HANDOFF_HINT  (the `restore` variant, restore/libs/MVS/SceneDensify.cpp:508-532): they are the extra hypothesis of the last
 *       sweep (d_hint_depth / d_hint_normal above).  cv::resize INTER_AREA enlarging, exactly as hcmvs_resize_area_up; the range given
 *       in d_min / d_max is widened by every enlarged depth hd BEFORE the clean-up, in raster order (lo = lo > hd ? hd : lo,
 *       hi = hi > hd ? hi : hd -- so a NaN replaces hi and is replaced by whatever follows it); a pixel whose depth is not > 0 or
 *       whose normal has no length gets hint depth 0 (its normal stays as enlarged), the others the normal at length 1.  On return
 *       d_min = max(lo, 0) and d_max = hi, a zero of either sign as +0.
 * Both forms below compute the same bits (a NaN is a NaN: its sign and payload are not part of that). */
enum { HCMVS_HANDOFF_INIT = 0, HCMVS_HANDOFF_HINT = 1 };
enum {
	HCMVS_HANDOFF_OK = 0,
	HCMVS_HANDOFF_EMPTY = 1 /* init mode: the handed-over map holds no valid depth (hi is not > 0).  The destination maps are written all the
	                           same (depth 0 everywhere), d_min / d_max are left untouched; the call and its other items do not fail */
};
typedef struct {
	const float *src_depth, *src_normal; /* src_w * src_h, src_w * src_h * 3 */
	int32_t src_w, src_h;
	float *dst_depth, *dst_normal;       /* dst_w * dst_h, dst_w * dst_h * 3: every pixel of both is written */
	int32_t dst_w, dst_h;
	float d_min, d_max;                  /* hint mode: in / out; init mode: out */
	int32_t status;                      /* out: HCMVS_HANDOFF_* (set for every item of a call that was not refused) */
	uint64_t n_valid;                    /* out: destination pixels left with a depth > 0 */
	uint64_t n_clamped;                  /* out: ... whose resampled depth was <= 0 or NaN although a source sample that entered it was > 0 */
	uint64_t n_rescaled;                 /* out: ... whose normal was divided by its length */
} hcmvs_handoff_item;
/* counters of the last hcmvs_handoff_maps_device call, summed over its items */
typedef struct {
	uint64_t n_pixels;   /* destination pixels written */
	uint64_t n_valid;
	uint64_t n_clamped;
	uint64_t n_rescaled;
	int32_t n_items;
	int32_t n_empty;     /* items with status HCMVS_HANDOFF_EMPTY */
	float ms_device;     /* HIP events around the kernels */
} hcmvs_handoff_stats;
/* HOST buffers, host code, no context (callable from any thread): the rule in a plain loop.  1 <= n_items <= HCMVS_MAX_BATCH.
 * HCMVS_ERR_INVALID, before anything is read or written: a null pointer, a size below 1, a map of 2^29 pixels or more, hint mode with a
 * destination smaller than the source in either direction or a range given as NaN, a destination that overlaps a source or another
 * destination of the call (its own item's included: in place is not supported), an unknown mode. */
int hcmvs_handoff_maps(hcmvs_handoff_item* items, int32_t n_items, int32_t mode);
/* The same with every map in DEVICE memory (the items array itself is a host array): ONE pass for the whole batch of items of any
 * mix of sizes (a launch over all pixels and a small one that folds the ranges), enqueued on the context's stream and therefore ordered before a following hcmvs_estimate*_device.  The ranges must be
 * final on return, so the call synchronises with the stream -- once, however many items.  The same refusals, before anything reaches
 * the device.  HCMVS_OK when every item ran; an item without a valid depth is reported in its status only. */
int hcmvs_handoff_maps_device(hcmvs_ctx* ctx, hcmvs_handoff_item* items, int32_t n_items, int32_t mode);
int hcmvs_get_handoff_stats(hcmvs_ctx* ctx, hcmvs_handoff_stats* out);

/* ---- the speckle filter: small depth segments of a finished map are removed ---------------------------------
 * Upstream's speckle removal (nSpeckleSize, default 100; SceneDensify.cpp:1956-2042, compiled out in the fork) with a symmetric edge:
 *   a pixel is valid when depth > 0 (a NaN is not; an infinite depth is, and is similar to nothing);
 *   two valid 4-neighbours p, q are joined when fabsf(dp - dq) / dp < thr AND fabsf(dp - dq) / dq < thr, in float32, IEEE division;
 *   a segment is a connected component of valid pixels under those edges, its canonical label the smallest raster index y * w + x in it;
 *   a segment of fewer than speckle_size pixels is removed: depth = 0, normal = (0, 0, 0), conf = 0.  Everything else is left bit for
 *   bit as it was.  speckle_size 0 or 1 removes nothing.  thr: upstream's is 0.01f * 0.7f.
 * The filter is idempotent and deterministic (sizes are integers).  Both forms below compute the same bits. */
typedef struct {
	int32_t width, height;
	float* d_depth;     /* width * height, in / out */
	float* d_normal;    /* width * height * 3, in / out, or NULL */
	float* d_conf;      /* width * height, in / out, or NULL */
	int32_t* d_labels;  /* width * height, or NULL: out, the canonical label of every pixel, -1 where the depth is not valid, as BEFORE the removal */
} hcmvs_speckle_item;
/* counters of a call, summed over its maps */
typedef struct {
	uint64_t n_valid;      /* valid pixels before the removal */
	uint64_t n_removed;    /* pixels removed */
	uint64_t n_segments;
	uint64_t n_small;      /* segments removed */
	uint32_t largest;      /* pixels of the largest segment */
	float ms_device;       /* device form: HIP events around the kernels; host form: 0 */
	uint64_t device_bytes; /* device form: the scratch of the call (8 B per pixel of the batch and a little); host form: 0 */
} hcmvs_speckle_stats;
/* Every map in DEVICE memory (the items array itself is a host array), 1 <= n_items <= HCMVS_MAX_BATCH maps of any mix of sizes: ONE
 * set of five launches for the whole batch, however many maps and whatever they hold, enqueued on the context's stream; the call then
 * synchronises with the stream once, to read the counters and the error word.  HCMVS_ERR_INVALID, before anything reaches the device:
 * null items, n_items out of range, a size below 1 or width * height >= 2^31, a null depth, a depth_diff_threshold that is not a finite
 * number > 0, two buffers of the call that overlap.  HCMVS_ERR_INTERNAL when a union-find loop ran past its bound (never expected;
 * no loop of the kernels is unbounded). */
int hcmvs_remove_speckles_batch_device(hcmvs_ctx* ctx, const hcmvs_speckle_item* items, int32_t n_items, float depth_diff_threshold, uint32_t speckle_size,
                                       hcmvs_speckle_stats* stats_or_null);
/* HOST buffers, host code, no context (callable from any thread): the rule as a sequential flood fill.  The same refusals. */
int hcmvs_remove_speckles(int32_t w, int32_t h, float* depth, float* normal_or_null, float* conf_or_null, int32_t* labels_or_null, float depth_diff_threshold,
                          uint32_t speckle_size, hcmvs_speckle_stats* stats_or_null);

/* ---- filter and fuse: work on the estimated maps registered per view ------------------------------------ */

/* register the maps of view `id` (host buffers are copied).  normal may be NULL.  d_min/d_max: the depth range
 * FilterDepthMap clips the adjusted depth to (SceneDensify.cpp:3156). */
int hcmvs_set_depthmap(hcmvs_ctx* ctx, uint32_t id, const float* depth, const float* normal_or_null,
                       const float* conf, float d_min, float d_max);
/* same for maps that already live in device memory; d_depth is MUTATED by hcmvs_fuse like the reference does
 * (SceneDensify.cpp:3447-3449).  Depths must be >= 0 (0 = no estimate): while a fusion or a post-filter runs, the sign of a depth
 * marks the estimates that already belong to a point; it is restored before the call returns. */
int hcmvs_set_depthmap_device(hcmvs_ctx* ctx, uint32_t id, float* d_depth, const float* d_normal_or_null,
                              const float* d_conf, float d_min, float d_max);
/* read the (possibly mutated) maps back; any pointer may be NULL */
int hcmvs_get_depthmap(hcmvs_ctx* ctx, uint32_t id, float* depth, float* normal, float* conf);
/* DepthData::neighbors of view `id`: image ids in decreasing importance (Scene.cpp:545-678), at most 31 for fuse.
 * An entry need not be a registered view, nor one with maps: hcmvs_fuse, hcmvs_fuse_cloud, hcmvs_postfilter, hcmvs_postfilter_sequence and
 * hcmvs_filter_sequence pass such an entry over, as the reference does with an image without a depth map (SceneDensify.cpp:3383-3385) --
 * the result is that of the list without it (the entry still counts towards the 31).  The entry takes part as soon as a view with that id
 * is registered and given maps.  Every entry must be below 65536, the bound on view ids (hcmvs_upload_view): a larger one is refused with
 * HCMVS_ERR_INVALID and the list of the view stays as it was. */
int hcmvs_set_neighbors(hcmvs_ctx* ctx, uint32_t id, const uint32_t* ids, int32_t n);

/* bool DepthMapsData::FilterDepthMap(DepthData&, const IIndexArr&, bool bAdjust) (SceneDensify.cpp:3006-3259).
 * out_depth / out_conf: w*h host buffers (the reference writes them to filtered.dmap/.cmap).
 * Fails with HCMVS_ERR_INVALID when there are fewer neighbours than n_min_views (the reference returns false). */
int hcmvs_filter(hcmvs_ctx* ctx, uint32_t ref_id, const uint32_t* neighbor_ids, int32_t n_neighbors, int32_t adjust,
                 int32_t n_min_views, int32_t n_min_views_adjust, float depth_diff_threshold, float* out_depth,
                 float* out_conf, uint64_t* n_processed, uint64_t* n_discarded);

/* counters of one hcmvs_filter_sequence call */
typedef struct {
	uint64_t n_processed;      /* valid depths of the filtered images (the sum of what SceneDensify.cpp:3255 logs per image) */
	uint64_t n_discarded;      /* ... that the filter removed */
	uint32_t n_filtered;       /* images filtered */
	uint32_t n_skipped;        /* images of ids left untouched: no maps, or fewer usable neighbours than the filter needs */
	uint32_t batch;            /* reference images the largest batch held */
	float ms_device;           /* device time of the stage, first fill to commit (HIP events on the context's stream) */
	uint64_t device_bytes;     /* z-buffer keys of the largest batch + staging + tables */
	uint64_t* image_processed; /* in: NULL, or n_ids entries; out: per entry of ids its processed depths (0 for a skipped image) */
	uint64_t* image_discarded; /* the same for the discarded depths */
} hcmvs_filter_stats;
/* The depth-map filter STAGE: Scene::DenseReconstructionFilter (SceneDensify.cpp:4100-4185, queued at :3721-3756) on the registered
 * maps (hcmvs_set_depthmap_device, or hcmvs_set_depthmap: the context's copies), updated in place like hcmvs_postfilter does;
 * hcmvs_get_depthmap reads them back.
 *   - Every image of ids that has maps is filtered (FilterDepthMap, the arithmetic of hcmvs_filter) against the first max_neighbors
 *     entries of its hcmvs_set_neighbors list that have maps themselves; entries without maps are passed over, not counted
 *     (:4116-4131; the reference's numMaxNeighbors is 8).  1 <= max_neighbors <= 64.
 *   - Every image is filtered from the maps as they stood when the call began -- "load the filtered maps after all depth-maps were
 *     filtered" (:4134-4135: with one thread every EVT_FILTERDEPTHMAP precedes every EVT_ADJUSTDEPTHMAP).  The new depth and
 *     confidence wait in a staging area (8 B per pixel of the listed images) and replace the registered maps after the last vote.
 *   - An image with fewer usable neighbours than n_min_views or n_min_views_adjust (or with none) keeps its maps (:3016-3019:
 *     FilterDepthMap returns false, no adjust event); so does an image of ids without maps (:4110-4113).  Both are counted in
 *     stats->n_skipped; neither is an error.
 *   - Only depth and confidence change; the normal map is not touched, as in the reference.
 * The images are processed in batches (one z-buffer fill, one splat launch over all (image, neighbour) pairs, one vote launch per
 * batch, one commit launch at the end) on the context's stream, with no host synchronisation between the batches: like the other filter / fuse entries the call waits for
 * the stream and uploads its map table when it begins, and it waits once more at the end, to read the counters.  The
 * batch is as large as the z-buffer keys (images x neighbours x pixels x 8 B) fit into half of the free device memory;
 * HCMVS_FILTER_BATCH=<n>|all in the environment forces it.  The result does not depend on it.  stats may be NULL. */
int hcmvs_filter_sequence(hcmvs_ctx* ctx, const uint32_t* ids, int32_t n_ids, int32_t max_neighbors, int32_t adjust, int32_t n_min_views,
                          int32_t n_min_views_adjust, float depth_diff_threshold, hcmvs_filter_stats* stats);

/* Order in which the pixels of ONE image are visited by hcmvs_fuse (the image order is always the caller's).
 * 0 (default): raster order, the reference's (SceneDensify.cpp:3355-3358); the cloud equals the sequential one bit for bit.
 * 1: a fixed pseudo-random order (a bijective hash of the raster index): the same greedy rule visits the pixels in
 *    another order, and the cloud differs from the reference's within the tolerance the north star states (point count
 *    within 1 %); the output is still written in raster order and deterministic.  (The option dates from the rounds in
 *    which the order decided how long the fusion took; it no longer does.) */
int hcmvs_set_fuse_order(hcmvs_ctx* ctx, int32_t mode);

/* void DepthMapsData::FuseDepthMaps(PointCloud&, bool, bool) (SceneDensify.cpp:3265-3495).  order: image ids,
 * best connected first (SceneDensify.cpp:3302).  Output host buffers hold `capacity` points: xyz 3 f32, normal
 * 3 f32 or NULL, bgr 3 u8 (B,G,R) or NULL, n_views u32 or NULL.  *n_points / *n_depths are the numbers the
 * reference logs (SceneDensify.cpp:3461).  Points come out in the reference's order. */
int hcmvs_fuse(hcmvs_ctx* ctx, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse,
               float depth_diff_threshold, float normal_diff_deg, float depthweight, float normalweight,
               uint64_t capacity, float* xyz, float* normal_or_null, uint8_t* bgr_or_null, uint32_t* n_views_or_null,
               uint64_t* n_points, uint64_t* n_depths);

/* The fork's depth-map post-filters, which the reference applies to every image after outer iterations 1 and 2
 * (SceneDensify.cpp:3939-3958), on the registered DEVICE maps of view `id` (hcmvs_set_depthmap_device; depth, normal and conf
 * are updated in place):
 *   RemoveSmallSegments as the fork rewrote it (SceneDensify.cpp:2048-2275): a complete FuseDepthMaps pass over the maps of
 *   `order` -- it zeroes the estimates that fused points occlude, in every image, exactly like hcmvs_fuse -- which leaves
 *   depthMap_fuse / normalMap_fuse = the image's maps restricted to the pixels that ended up in a fused point;
 *   GapInterpolation (SceneDensify.cpp:2280-3001): gaps of at most gap_size (nIpolGapSize = 7) pixels along rows, then
 *   columns, whose ends agree within 2.5 x depth_diff_threshold -- or longer ones whose ends agree or whose gradient-map values
 *   differ by at most 10 % -- are filled by linear interpolation of depth and normal direction; finally the maps take the
 *   fused-and-filled values where those are valid.
 * RemoveSmallSegments compares with the plain thresholds (SceneDensify.cpp:2083, 2177): --depthweight / --normalweight only scale the
 * thresholds of FuseDepthMaps (SceneDensify.cpp:3310, 3400), so this entry takes no weights; and it visits the pixels of an image in
 * raster order (SceneDensify.cpp:2130-2131) whatever hcmvs_set_fuse_order says about FuseDepthMaps.
 * The reference's third, per-pixel pass (SceneDensify.cpp:2790-2983) reads uninitialised variables and is not reproduced.
 * n_filled: pixels the two interpolation passes wrote. */
int hcmvs_postfilter(hcmvs_ctx* ctx, uint32_t id, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse, float depth_diff_threshold,
                     float normal_diff_deg, int32_t gap_size, uint64_t* n_filled);
/* The same for the images ids[0 .. n_ids) one after the other: identical in effect to n_ids calls of hcmvs_postfilter in that order
 * (every image's fusion sees the maps the images before it left), with the per-call set-up paid once and every fusion after the first
 * computed INCREMENTALLY -- only what depends on the estimates that changed since the previous fusion (the pixels the previous image's
 * gap interpolation filled, the estimates that fusion zeroed) is evaluated again; same decisions, fusion after fusion (the state kept
 * between the fusions is about 360 B per pixel of the scene; when it does not fit the device, or an image occurs twice in ids, every
 * fusion runs from scratch).  n_filled: total over the images.
 * NOTE on the order: the reference filters image k right after image k's own estimate (single-thread event order,
 * SceneDensify.cpp:3889-3965), i.e. hcmvs_estimate(k), hcmvs_postfilter(k), hcmvs_estimate(k + 1), ...  Calling this entry AFTER all
 * estimates of an outer iteration is the batch schedule of this repo's driver -- a documented departure. */
int hcmvs_postfilter_sequence(hcmvs_ctx* ctx, const uint32_t* ids, int32_t n_ids, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse,
                              float depth_diff_threshold, float normal_diff_deg, int32_t gap_size, uint64_t* n_filled);

/* The fused cloud with everything PointCloud holds (PointCloud.h: points, pointViews, pointWeights, colors, normals).
 * Host buffers owned by the caller; any optional pointer may be NULL.  The view lists are stored back to back (CSR): point p's
 * n_views[p] entries follow those of point p-1, image ids ascending like PointCloud::ViewArr (SceneDensify.cpp:3376-3379,
 * 3408-3411); a point merges at most one depth per image, so views_capacity = the number of valid depths is always enough. */
typedef struct {
	uint64_t capacity;        /* in: room for this many points */
	float* xyz;               /* capacity * 3 */
	float* normal;            /* capacity * 3 or NULL */
	uint8_t* bgr;             /* capacity * 3 (B,G,R) or NULL */
	uint32_t* n_views;        /* capacity or NULL */
	uint64_t views_capacity;  /* in: room for this many view entries (0 with NULL lists) */
	uint32_t* view_ids;       /* views_capacity or NULL */
	float* view_weights;      /* views_capacity or NULL: Conf2Weight of the merged estimates (SceneDensify.cpp:154-156) */
	uint64_t n_points, n_depths, n_view_entries; /* out */
} hcmvs_cloud;
/* hcmvs_fuse with the complete cloud.  With cloud->xyz == NULL the call only COUNTS: the fusion runs (with its side effect, the
 * invalidated depths) and n_points / n_depths / n_view_entries come back, no point is produced.  A fusion repeated on the maps a fusion
 * has left makes the same decisions (what it invalidated is simply absent the second time), so a counting call followed by a call with
 * buffers of exactly that size yields the cloud a single call with large enough buffers would have produced -- how a caller avoids
 * reserving the worst case (half a point per pixel of the scene). */
int hcmvs_fuse_cloud(hcmvs_ctx* ctx, const uint32_t* order, int32_t n_order, int32_t n_min_views_fuse, float depth_diff_threshold,
                     float normal_diff_deg, float depthweight, float normalweight, hcmvs_cloud* cloud);

/* MVS::EstimatePointColors (DepthMap.cpp:2125-2161; --estimate-colors 1): per point the colour of the closest of its views,
 * sampled bilinearly from that view's colour image (white when it projects outside).  Views must have been registered with a
 * colour image.  Host arrays: xyz n*3, n_views n, view_ids (CSR as in hcmvs_cloud), out bgr n*3. */
int hcmvs_estimate_point_colors(hcmvs_ctx* ctx, uint64_t n_points, const float* xyz, const uint32_t* n_views, const uint32_t* view_ids,
                                uint8_t* bgr);
/* MVS::EstimatePointNormals (DepthMap.cpp:2221-2269; --estimate-normals 1): normal of the plane fitted by PCA to the
 * n_neighbors nearest points of every point (the reference calls CGAL::pca_estimate_normals with 16), oriented towards the first
 * view of the point.  Computed on the device (exact k-nearest search + PCA, 3 <= n_neighbors <= 32, fewer than 2^31 points);
 * CGAL is absent, so the PCA is restated (parity unpinned).  Host arrays in and out.  The neighbours of a point are the
 * min(n_neighbors, n_points) points with the smallest (squared distance in double, index), the point itself among them.
 * HCMVS_ERR_INVALID, before anything reaches the device, when a coordinate is NaN or infinite (the message names the first
 * such point), when a point has no view or when its first view is not registered; n_points == 0 succeeds and writes nothing. */
int hcmvs_estimate_point_normals(hcmvs_ctx* ctx, uint64_t n_points, const float* xyz, const uint32_t* n_views, const uint32_t* view_ids,
                                 int32_t n_neighbors, float* normal);

/* counters of the last hcmvs_point_cloud_filter call */
typedef struct {
	uint64_t pairs;          /* (point, view) pairs evaluated */
	uint64_t skipped_pairs;  /* view entries naming an image >= n_images or an uncalibrated one: skipped */
	uint64_t fallback_pairs; /* pairs that took the exact path over all points (X behind the camera, outside the binned domain) */
	uint64_t candidates;     /* cone tests run */
	uint64_t hits;           /* votes cast: VISIBLE and not depth-similar (one int32 atomic each) */
	uint64_t device_bytes;   /* device memory the call allocated */
	float ms_device;         /* device time from the first kernel to the last (HIP events) */
} hcmvs_visibility_stats;
/* Scene::PointCloudFilter (SceneDensify.cpp:4188-4320; DensifyPointCloud --filter-point-cloud < 0): the visibility of every point is
 * summed over the cones of all (point X, view j of X) pairs -- apex the camera centre of j, axis through X, half-angle
 * float(ComputeFOV(0) / width), height 1.02 |X - C| -- where every point P inside the cone that is not within 1 % of X's distance gains
 * |views(P)| when behind X and loses |views(X)| when in front; points with visibility <= th_remove are removed by the reference's reverse
 * swap-with-last loop (PointCloud::RemovePoint).  Computed on the device, exactly (integer sums; float32 arithmetic with the association
 * stated in DESIGN.md section 5).  Points as CSR (as in hcmvs_cloud, fewer than 2^32 - 1); per image: wh (width, height; width 0 =
 * uncalibrated, its pairs are skipped), K and R (9 f64 each, at that width x height), C (3 f64).  Out: visibility (n int32) or NULL,
 * kept (n uint32): the indices of the kept points in the reference's output order, *n_kept of them; stats or NULL. */
int hcmvs_point_cloud_filter(hcmvs_ctx* ctx, uint64_t n_points, const float* xyz, const uint32_t* n_views, const uint32_t* view_ids,
                             uint32_t n_images, const int32_t* wh, const double* K, const double* R, const double* C, int32_t th_remove,
                             int32_t* visibility_or_null, uint32_t* kept, uint64_t* n_kept, hcmvs_visibility_stats* stats_or_null);

/* counters of the last hcmvs_sample_mesh call */
typedef struct {
	uint64_t n_faces;           /* faces of the mesh */
	uint64_t n_zero_area_faces; /* faces whose double area is exactly 0 (repeated or collinear vertices) */
	uint64_t n_points;          /* points of the cloud */
	double area;                /* Mesh::ComputeArea: the float32 face areas summed into a double in face order */
	double density;             /* points per square unit the counts were drawn with (0: the area was below ZEROTOLERANCE<float>) */
	float ms_device;            /* device time from the first kernel to the last (HIP events) */
	uint64_t device_bytes;      /* device memory the call allocated */
} hcmvs_mesh_sample_stats;
/* Mesh::SamplePoints (Mesh.cpp:3444-3527; DensifyPointCloud --sample-mesh): a point cloud sampled uniformly on a triangle mesh, on the
 * device.  sample > 0 is a density (points per square unit), sample < 0 a number of points (ROUND2INT(-sample), density = that / the
 * mesh area).  Face f gets (unsigned)(area_f * density) points plus one more with the probability of the fractional part; the cloud
 * comes out in the reference's order (faces ascending).  The reference's random stream is unseeded, so the draws are defined here
 * (counter-based): the cloud depends on (mesh, sample, seed) only.  Host arrays in and out: vertices
 * n_vertices*3, faces n_faces*3 (fewer than 2^31 - 1 faces); texcoords (n_faces*6: u v of the three corners) and texture (tex_h*tex_w*3, B,G,R)
 * both or neither; out xyz capacity*3, face_of_point capacity or NULL, bgr capacity*3 or NULL (written only with a texture); fewer than
 * 2^32 points.  With xyz == NULL the call only COUNTS (*n_points; the same seed gives the same count in the call that fills).
 * capacity < the points needed: HCMVS_ERR_INVALID, *n_points = what is needed.  HCMVS_ERR_INVALID before anything reaches the device,
 * with a message naming the first offender: a vertex coordinate or texture coordinate that is not finite, a vertex index >= n_vertices,
 * n_faces == 0, sample == 0 (or NaN, or below -2^31), a texture without texcoords or texcoords without a texture.  Zero points is success.
 * The work space of the mesh is checked against the free device memory before the first launch, the cloud's before the point pass. */
int hcmvs_sample_mesh(hcmvs_ctx* ctx, uint32_t n_vertices, const float* vertices, uint32_t n_faces, const uint32_t* faces,
                      const float* texcoords_or_null, const uint8_t* texture_bgr_or_null, int32_t tex_w, int32_t tex_h, float sample, uint64_t seed,
                      uint64_t capacity, float* xyz_or_null, uint32_t* face_of_point_or_null, uint8_t* bgr_or_null, uint64_t* n_points,
                      hcmvs_mesh_sample_stats* stats_or_null);

/* the parameters of hcmvs_select_views; hcmvs_default_view_select_params fills the reference's defaults */
typedef struct {
	int32_t n_min_views;        /* OPTDENSE::nMinViews 2: neighbours an image needs before the filter (at most calibrated images - 1) */
	int32_t n_min_point_views;  /* views a point needs to enter an image's points list: nMinViewsTrustPoint > 1 ? it : 2 -> 2 */
	int32_t n_max_views;        /* OPTDENSE::nMaxViews 12: neighbours kept per image, 1..64 */
	int32_t number_views;       /* --number-views 5: source views per image, 0 = all neighbours */
	float optim_angle_deg;      /* OPTDENSE::fOptimAngle 10 */
	float min_angle_deg;        /* OPTDENSE::fMinAngle 3 */
	float max_angle_deg;        /* OPTDENSE::fMaxAngle 65 */
	float min_area;             /* OPTDENSE::fMinArea 0.01 */
	float min_scale;            /* 0.2 (SceneDensify.cpp:319) */
	float max_scale;            /* 3.2 */
	float min_score_ratio;      /* OPTDENSE::fViewMinScoreRatio 0.3 */
	float min_score;            /* OPTDENSE::fViewMinScore 0 */
} hcmvs_view_select_params;
void hcmvs_default_view_select_params(hcmvs_view_select_params* p);

/* what hcmvs_select_views writes: host arrays of the caller, M = n_max_views.  The per-neighbour rows are in decreasing score (ties by
 * ascending image id); the source views of image i are its first n_srcs[i] neighbours.  Rows past n_neighbors[i] are zero. */
typedef struct {
	int32_t* status;          /* n_images: 0 selected; 1 SelectNeighborViews false (<= 3 points, or fewer than min(n_min_views, calibrated - 1)
	                             candidates); 2 no candidate survives FilterNeighborViews, or no source view is left; 3 uncalibrated */
	uint32_t* n_seen;         /* n_images: points seen by the image (nPoints) */
	float* avg_depth;         /* n_images: Image::avgDepth (Scene.cpp:575, :603); 0 for an image that sees no point */
	uint32_t* n_candidates;   /* n_images: neighbours before the filter */
	uint32_t* n_neighbors;    /* n_images: neighbours kept, <= M; 0 unless status is 0 or 2 */
	uint32_t* n_srcs;         /* n_images: source views, <= n_neighbors; 0 unless status is 0 */
	uint32_t* nb_id;          /* n_images * M */
	uint32_t* nb_points;      /* n_images * M: points shared */
	float* nb_scale;          /* n_images * M: average footprint ratio */
	float* nb_angle;          /* n_images * M: average viewing angle, radians */
	float* nb_area;           /* n_images * M: covered area = occupied cells / 256 */
	float* nb_score;          /* n_images * M */
	float* src_scale;         /* n_images * M: of the source views; 1 unless |nb_scale - 1| >= 0.15 (the view is resampled, DepthMap.h:233-238) */
	uint64_t* points_first;   /* n_images + 1, or NULL: the points lists (DepthData::points) as CSR ... */
	uint32_t* point_ids;      /* ... into point_ids (the sum of n_views entries always suffices), or NULL; ascending per image */
} hcmvs_view_selection;
/* counters of the last hcmvs_select_views call */
typedef struct {
	uint64_t pairs;          /* ordered (image, other image, point) records scored */
	uint64_t skipped;        /* view entries naming an image >= n_images or an uncalibrated one: skipped */
	uint64_t chunks;         /* ranges of images the call was split into */
	uint64_t device_bytes;   /* device memory the call allocated */
	float ms_device;         /* device time from the first kernel to the last (HIP events) */
} hcmvs_view_select_stats;
/* DepthMapsData::SelectViews (SceneDensify.cpp:307-327: Scene::SelectNeighborViews, Scene.cpp:545-661, then Scene::FilterNeighborViews,
 * :665-678) and the cut of DepthMapsData::InitViews (SceneDensify.cpp:362-367) for EVERY image of a scene in one call, on the device: the
 * sparse cloud is walked once, not once per image.  Cameras as in hcmvs_point_cloud_filter (wh: width, height, width 0 = uncalibrated;
 * K, R 9 f64 each at that size; C 3 f64; 1 <= n_images < 65 536); the sparse cloud as CSR (xyz n_points*3, n_views, view_ids strictly
 * ascending per point, fewer than 2^32 entries).  The arithmetic is stated in DESIGN.md section 5 (D12): float32 where the reference
 * computes in float32, every sum taken sequentially in ascending point index, so the call is bit-identical run to run and does not depend
 * on how it was split.  A view entry naming an image >= n_images or an uncalibrated one is skipped for scoring (stats->skipped) but still
 * counts towards the point's number of views.  HCMVS_ERR_INVALID before anything reaches the device, with a message naming the first
 * offender: a coordinate or an entry of a calibrated camera that is not finite, view ids that are not strictly ascending, n_max_views
 * outside 1..64, n_images 0 or >= 65 536, 2^32 view entries or more.  n_points == 0 succeeds: every calibrated image gets status 1.
 * The records of the ordered pairs (32 B each with the sort's buffers) are checked against the free device memory; beyond half of it the
 * images are processed in ranges (HCMVS_SELECT_CHUNK=<images>, read at every call, forces the size of a range). */
int hcmvs_select_views(hcmvs_ctx* ctx, uint32_t n_images, const int32_t* wh, const double* K, const double* R, const double* C,
                       uint64_t n_points, const float* xyz, const uint32_t* n_views, const uint32_t* view_ids,
                       const hcmvs_view_select_params* params, const hcmvs_view_selection* out, hcmvs_view_select_stats* stats_or_null);

#ifdef __cplusplus
}
#endif
#endif

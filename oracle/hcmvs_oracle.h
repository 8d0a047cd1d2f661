/*
 * oracle/hcmvs_oracle.h -- TEST INFRASTRUCTURE.  CPU restatement of the HC-MVS (OpenMVS v1.1.1 fork)
 * PatchMatch depth-map estimation, geometric filter and fusion path.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use this library; the
 * product (hc-mvs_amd/, include/) never includes, links or calls it.
 *
 * PARITY UNPINNED: the reference ships no tests, golden vectors or fixtures for this path and cannot be
 * built in this environment (needs OpenCV, Eigen, Boost, CGAL), so this
 * restatement is checked against hand-derived known-answer vectors only (tests/test_oracle_*.py).
 *
 * Citation shorthand (all under /root/reference/frame_main/libs/):
 *   DM.cpp = MVS/DepthMap.cpp, DM.h = MVS/DepthMap.h, SD.cpp = MVS/SceneDensify.cpp,
 *   Util.inl / Types.h / Types.inl / Random.h = Common/...
 *
 * "Defined subset" (SURVEY.md Appendix A): opticalflow=0, use-semantic=0, nOptimize=0;
 * photometric_flow is honoured as the plain (1-pf) scale it amounts to (DM.cpp:892,931).
 */
#ifndef HCMVS_ORACLE_H
#define HCMVS_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HCOR_MAX_VIEWS 16
/* The reference fixes nSizeHalfWindow = 7 and nTexels = 64 at compile time (DM.h:354-358), i.e. --n-adapthalfwin <= 7.
 * BASELINE.json configs[4] asks for an 11x11 patch (adapthalfwin 10, 121 taps): SURVEY.md 8d item 5 has the restatement
 * generalise the two constants.  The patch loops (DM.cpp:486-494, 554-577) are already written for any `a`; what follows the
 * constant is the border every pass keeps clear (DM.cpp:442-447 uses nSizeHalfWindow): max(7, adapthalfwin). */
#define HCOR_MAX_HALF_WINDOW 10
#define HCOR_MAX_TAPS 121    /* (HCOR_MAX_HALF_WINDOW + 1)^2; the reference's nTexels is 64, DM.h:358 */
#define HCOR_HALF_WINDOW 7   /* nSizeHalfWindow, DM.h:354: the border for adapthalfwin <= 7 */
#define HCOR_MAX_NEIGHBORS 32

enum { HCOR_ARITH_REFERENCE = 0, HCOR_ARITH_DEVICE = 1 };
enum { HCOR_ORDER_ZIGZAG = 0, HCOR_ORDER_ROWS = 1 };

/* one calibrated view: x_cam = R (X - C), pixel = K x_cam / z, pixel centres at integers (Camera.h) */
typedef struct {
	int width, height;
	const float* gray;   /* H*W row-major, [0,1] (Types.inl:2354-2400 toGray) */
	const uint8_t* bgr;  /* optional H*W*3 (B,G,R) working-resolution colour image, may be NULL */
	double K[9], R[9], C[3];
} hcor_view;

/* view spread: the maps a source view offers, width x height floats (normal: 3 per pixel); depth == NULL: none */
typedef struct {
	int width, height;
	const float* depth;
	const float* normal;
	const float* conf;
} hcor_spread_map;

/* replaces the OPTDENSE globals (DM.cpp:67-143) for this path */
typedef struct {
	int adapthalfwin;           /* --n-adapthalfwin (DM.cpp:455-461); reference <= 7, generalised to <= HCOR_MAX_HALF_WINDOW */
	int n_estimation_iters;     /* --n-EstimationIters: inner sweeps (SD.cpp:949) */
	int it_external;            /* outer iteration this call is (SD.cpp:758) */
	int n_external_iters;       /* --n-EstimationIters-external: pass C runs when it_external == n-1 */
	int propagate_halfwin;      /* --n-propagatehalfwin (DM.cpp:1071) */
	int propagate_step;         /* --n-propagatestep (DM.cpp:1072) */
	int n_random_iters;         /* nRandomIters = 6 (DM.cpp:120) */
	float ncc_threshold_keep;   /* fNCCThresholdKeep = 0.55 (DM.cpp:117) */
	float random_depth_ratio;   /* fRandomDepthRatio = 0.003 */
	float random_angle1_deg;    /* fRandomAngle1Range = 16 */
	float random_angle2_deg;    /* fRandomAngle2Range = 10 */
	float random_smooth_depth;  /* fRandomSmoothDepth = 0.02 */
	float random_smooth_normal_deg; /* fRandomSmoothNormal = 13 */
	float random_smooth_bonus;  /* fRandomSmoothBonus = 0.93 */
	float photometric_flow;     /* --n-photometric_flow: scores scaled by (1-pf) (DM.cpp:892) */
	uint32_t seed;              /* counter-based RNG seed (replaces mt19937, Random.h:102) */
	int arith_mode;             /* HCOR_ARITH_* */
	int order;                  /* HCOR_ORDER_*: pixel visiting order of the sweeps */
	int n_threads;              /* zig-zag band height = max(64, 8*n_threads) (SD.cpp:835); ROWS order
	                               uses n_threads OpenMP threads and gives the same result for any count */
	int median_blur;            /* 1 = cv::medianBlur(depth,3) at the start of the call (SD.cpp:859) */
	/* restore variant (restore/libs/MVS/DepthMap.cpp:1527-1549): maps of the up-sampled coarser level (W*H depth, W*H*3 normal)
	 * tried as one more hypothesis, with a 0.1 bonus, in the last sweep of the last outer iteration; NULL = frame_main behaviour */
	const float* hint_depth;
	const float* hint_normal;
	/* --ignore-mask-label (DM.cpp:233-248, 319-381; SD.cpp:649-744, 776-860): W*H bytes, 1 = estimated, 0 = ignored; NULL = no mask.
	 * MapMatrix2ZigzagIdx drops the ignored pixels from the visiting order, so no pass writes them: hcor_estimate zeroes their depth,
	 * normal and conf before the median (DepthData::ApplyIgnoreMask) and they end holding the median's depth, normal 0, conf 0. */
	const uint8_t* keep;
	/* --n-viewspread (DM.cpp:1504-1608, hcmvs_spread.inc): one entry per source view, NULL = none.  Active when spread_on, maps are
	 * given and it_external >= 1.  The maps must not alias depth / normal / conf (a sweep must not read what it writes). */
	const hcor_spread_map* spread_maps;
	int spread_on;
	/* depth prior (--n-para_prior, --sigma-prior, --n-photo2geo; ScorePixelImage, DM.cpp:941-954; the term is stated at score_pixel in
	 * hcmvs_oracle.c): W*H floats, NULL = none.  Active when a map is given, para_prior > 0 and it_external >= photo2geo; it applies
	 * at the pixels whose prior is finite and > 0.  An active prior is refused together with view spread
	 * and with a hint on the last outer iteration (return 2), as the library refuses them. */
	const float* prior_map;
	float para_prior;           /* --n-para_prior = 0.5 */
	float sigma_prior;          /* --sigma-prior = 0.2 */
	int photo2geo;              /* --n-photo2geo = 2: first outer iteration that blends the term */
} hcor_params;

void hcor_default_params(hcor_params* p);

/* DepthData::ViewData::ScaleImage (DM.h:233-238): cv::resize(..., Size(), scale, scale, scale>1 ? INTER_CUBIC : INTER_AREA)
 * on an f32 image, restated from OpenCV 4.2's published algorithm (OpenCV is absent: parity unpinned) */
void hcor_resize_size(int w, int h, float scale, int* dw, int* dh);
void hcor_resize_gray(const float* src, int sw, int sh, float scale, float* dst, int dw, int dh);
/* cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_AREA) for dw >= sw, dh >= sh (INTER_AREA enlarging = bilinear kernel with area-mode
 * coefficients), ch interleaved f32 channels: the `restore` variant's up-sampling of the previous level's maps
 * (restore/libs/MVS/SceneDensify.cpp:523-524).  Restated from OpenCV 4.2's published source (parity unpinned). */
void hcor_resize_area_up(const float* src, int sw, int sh, int ch, float* dst, int dw, int dh);

/* The device association tests the two END taps of a patch column for "inside the image" (plus: z keeps its sign between them) where
 * the reference tests every tap (DM.cpp:566).  Counters of the device-mode evaluations since the last reset: patch columns tested,
 * and columns on which the two rules disagree. */
void hcor_inside_rule_stats(uint64_t* columns, uint64_t* differ, int reset);

/* ---- small pieces, exposed for known-answer tests ------------------------------------------- */

/* DM.cpp:354-381 MapMatrix2ZigzagIdx (no mask). coords_xy: 2*w*h uint16 (x,y pairs). returns count */
int hcor_zigzag_coords(int w, int h, int raw_stride, uint16_t* coords_xy);

/* counter-based RNG: uniform u32 for (seed, pixel index, stream, counter) */
uint32_t hcor_rand_u32(uint32_t seed, uint32_t pix, uint32_t stream, uint32_t ctr);

/* OpenCV-compatible helpers restated from their published algorithms (OpenCV itself is absent):
 * BGR->gray 8u fixed point, Sobel 3x3 (BORDER_REFLECT_101) + convertScaleAbs + addWeighted(.5,.5)
 * (SD.cpp:581-595 InitGraMap) and 3x3 median with BORDER_REPLICATE (SD.cpp:859). */
void hcor_bgr2gray_u8(const uint8_t* bgr, int w, int h, uint8_t* gray);
void hcor_gray_f32_to_u8(const float* gray, int w, int h, uint8_t* out);
void hcor_gradient_map(const uint8_t* gray, int w, int h, uint8_t* gra);
void hcor_median3(const float* in, int w, int h, float* out);

/* SD.cpp:783-808: splat sparse points (world XYZ, n of them) as 5x5 blocks; returns dMin/dMax */
void hcor_splat_init(const hcor_view* ref, const float* points_xyz, int n_points, float* depth,
                     float* normal, float* d_min, float* d_max);

/* portable math entry points (tests compare them with libm) */
float hcor_pm_expf(float x);
float hcor_pm_sinf(float x);
float hcor_pm_cosf(float x);
float hcor_pm_acosf(float x);
float hcor_pm_atan2f(float y, float x);

/* DM.cpp:450-519 FillPixelPatch for pixel (x,y): fills weight[n], temp_weight[n] (n = (a+1)^2 taps),
 * returns the number of taps; *sum_weights, *norm_sq0 as cached by the reference.  n_src only selects the
 * device-mode summation layout (segments per view) */
int hcor_fill_patch(const hcor_view* ref, const uint8_t* gra, const hcor_params* p, int n_src, int x, int y,
                    float* weight, float* temp_weight, float* sum_weights, float* norm_sq0);

/* DM.cpp:522-616 + 890-893 ScorePixelImage for one source view, no smoothness neighbours */
float hcor_score_view(const hcor_view* ref, const hcor_view* src, const uint8_t* gra,
                      const hcor_params* p, int x, int y, float depth, const float normal[3]);

/* DM.cpp:987-1046 ScorePixel over all views, no smoothness neighbours */
float hcor_score_pixel(const hcor_view* ref, const hcor_view* srcs, int n_src, const uint8_t* gra,
                       const hcor_params* p, int x, int y, float depth, const float normal[3]);

/* the depth prior's term piece by piece, over the helpers the scorer uses: the validity rule (D11: finite and > 0); out[0] =
 * 1 - para_prior, out[1] = -1 / (2 sigma^2) as the device association holds them; 2 (1 - wP) para_prior of one hypothesis; DM.cpp:950
 * on one view's score (a prior that is not usable leaves the score as it is) */
int hcor_prior_usable(float prior);
void hcor_prior_consts(float para, float sigma, float* out);
float hcor_prior_addend(float prior, float depth, float para, float sigma, int mode);
float hcor_prior_blend(float score, float prior, float depth, float para, float sigma, int mode);
/* hcor_score_pixel with the prior value `prior` at the pixel (p's prior_map is not read; para_prior, sigma_prior, photo2geo are);
 * view_scores (optional): the n_src view scores the aggregation ran over */
float hcor_prior_score_pixel(const hcor_view* ref, const hcor_view* srcs, int n_src, const uint8_t* gra, const hcor_params* p, int x, int y,
                             float depth, const float normal[3], float prior, float* view_scores);

/* Util.inl:614-626 */
void hcor_normal2dir(const float n[3], float p[2], int arith_mode);
void hcor_dir2normal(const float p[2], float n[3], int arith_mode);
/* DM.h:629-634 CorrectNormal for the pixel ray X0 = ((x-cx)/fx,(y-cy)/fy,1) */
void hcor_correct_normal(const hcor_view* ref, int x, int y, float n[3], int arith_mode);
/* DM.cpp:1671-1726 InterpolatePixel: depth at (x,y) of the plane through neighbour (nx,ny,depth,normal) */
float hcor_interpolate_pixel(const hcor_view* ref, int x, int y, int nx, int ny, float depth,
                             const float normal[3], float d_min, float d_max);

/* What the estimator derives from the cameras and the options before any pixel is visited (DM.cpp:386-439, DM.h:412-444; the
 * device association holds A = Hl Hr, Hm and Hr rounded to float), copied out as hcor_estimate holds it -- so that a test can
 * compare the host plan of the product (hc-mvs_amd/csrc/est_plan.h), which derives the same numbers on its own, field by field.
 * spT, spt: R_ref R_j^T and R_ref (C_j - C_ref) of view spread; jifx, jify: 1 / focal of view j. */
typedef struct {
	float Af[HCOR_MAX_VIEWS][9], Hmf[HCOR_MAX_VIEWS][3], Hrf[9];
	double ifx, ify;
	float dMin, dMax, dMinSqr, dMaxSqr;
	float smoothBonusDepth, smoothBonusNormal, smoothSigmaDepth, smoothSigmaNormal;
	float angle1Range, angle2Range;
	float thConfSmall, thConfBig, thConfRand, thRobust;
	double spT[HCOR_MAX_VIEWS][9], spt[HCOR_MAX_VIEWS][3], jifx[HCOR_MAX_VIEWS], jify[HCOR_MAX_VIEWS];
} hcor_est_consts;
void hcor_estimate_consts(const hcor_view* ref, const hcor_view* srcs, int n_src, const hcor_params* p, float d_min, float d_max,
                          hcor_est_consts* out);

/* ---- the path -------------------------------------------------------------------------------- */

/* SD.cpp:758-1072 EstimateDepthMap for one reference view (defined subset).
 * depth/normal/conf: H*W, H*W*3, H*W in/out.  gra: H*W gradient map (SD.cpp:581-595).
 * Runs: [keep-mask applied] -> [median blur] -> pass A (SD.cpp:649-675) -> n_estimation_iters sweeps (SD.cpp:677-686,
 * DM.cpp:1050-1501) -> pass C when it_external == n_external_iters-1 (SD.cpp:688-744).
 * This one path covers every variant the GPU is pinned to: the keep-mask, view spread, the `restore` hint and the depth prior are
 * optional inputs of hcor_params, honoured by the passes in both sweep orders and with any thread count.
 * counts (optional): receives the counters of the call.  Returns 0; 1 for arguments out of range; 2 for an active prior together
 * with view spread or with a hint on the last outer iteration. */
typedef struct {
	uint64_t evals;        /* ScorePixel evaluations */
	uint64_t evals_prior;  /* those that blended the prior's term: the evaluations of pixels with a usable prior while the prior is active */
	uint64_t pixels_prior; /* estimated pixels (kept, inside the border) with a usable prior while the prior is active */
} hcor_counts;
int hcor_estimate(const hcor_view* ref, const hcor_view* srcs, int n_src, const uint8_t* gra,
                  const hcor_params* p, float d_min, float d_max, float* depth, float* normal,
                  float* conf, hcor_counts* counts);
/* The reference's extra sweeps (SD.cpp:983-1031).  depth / normal / conf are taken as the state an estimate leaves between outer
 * iterations (conf = the score): sweeps first_sweep .. first_sweep + n_sweeps - 1, then pass C under hcor_estimate's condition; no
 * mask application, no median, no pass A.  The hint is never offered (p's is not read), as include/hcmvs_hip.h states for the
 * library.  Returns 1 also for first_sweep < 0, n_sweeps < 1, first_sweep + n_sweeps > 63, ncc_threshold_keep not > 0 and for view
 * spread (nothing pins it in this entry). */
int hcor_estimate_sweeps(const hcor_view* ref, const hcor_view* srcs, int n_src, const uint8_t* gra,
                         const hcor_params* p, int first_sweep, int n_sweeps, float d_min, float d_max, float* depth,
                         float* normal, float* conf, hcor_counts* counts);

/* the three passes individually (same arguments), for per-pass parity tests; counts (optional): evals and evals_prior are added to */
void hcor_pass_score(const hcor_view* ref, const hcor_view* srcs, int n_src, const uint8_t* gra,
                     const hcor_params* p, float d_min, float d_max, float* depth, float* normal,
                     float* conf, hcor_counts* counts);
void hcor_pass_sweep(const hcor_view* ref, const hcor_view* srcs, int n_src, const uint8_t* gra,
                     const hcor_params* p, int iter, float d_min, float d_max, float* depth,
                     float* normal, float* conf, hcor_counts* counts);
void hcor_pass_end(const hcor_params* p, int w, int h, float* depth, float* normal, float* conf);

/* view spread (hcmvs_spread.inc).  Counters summed over every call since the last reset: slots scored, slots accepted, slots dropped
 * by the depth <= 0 rule, candidates outside view j's map. */
void hcor_spread_stats(uint64_t* scored, uint64_t* accepted, uint64_t* dropped, uint64_t* outside, int reset);
/* trace of ONE pixel for the known-answer tests (single-threaded runs only): rows of 8 floats, see hcmvs_spread.inc */
void hcor_spread_trace_pixel(int x, int y);
int hcor_spread_trace_get(float* out, int cap);
/* DM.cpp:1590-1592 alone: depth of view src's pixel (nx, ny, nd) seen from ref */
float hcor_spread_transform_depth(const hcor_view* ref, const hcor_view* src, int nx, int ny, float nd, int mode);

/* ---- filter and fuse (hcmvs_fuse.c) ----------------------------------------------------------- */

typedef struct {
	int width, height;
	double K[9], R[9], C[3];
	float* depth;        /* H*W, mutated by fusion (SD.cpp:3448-3449) */
	const float* normal; /* H*W*3 camera space, may be NULL */
	const float* conf;   /* H*W */
	const uint8_t* bgr;  /* H*W*3 or NULL */
	float d_min, d_max;
	int n_neighbors;
	const uint32_t* neighbors; /* image ids, decreasing importance */
} hcor_depthmap;

/* SD.cpp:3006-3259 FilterDepthMap(bAdjust).  neighbor_ids index into maps[].  out_depth/out_conf: H*W.
 * returns 0 if too few neighbours (SD.cpp:3016-3019), 1 otherwise; n_discarded and n_processed as logged */
int hcor_filter_depthmap(const hcor_depthmap* maps, uint32_t ref_id, const uint32_t* neighbor_ids,
                         int n_neighbors, int adjust, int n_min_views, int n_min_views_adjust,
                         float depth_diff_threshold, float* out_depth, float* out_conf,
                         uint64_t* n_processed, uint64_t* n_discarded);

typedef struct {
	uint64_t n_points, capacity;
	float* xyz;       /* capacity*3 */
	float* normal;    /* capacity*3 or NULL */
	uint8_t* bgr;     /* capacity*3 or NULL (stored B,G,R like Interface.h:369) */
	uint32_t* n_views;/* capacity: number of views merged into each point */
	uint64_t n_depths;/* valid depths visited (SD.cpp:3359) */
	/* optional: PointCloud::pointViews / pointWeights stored back to back (point p's n_views[p] entries follow those of p-1) */
	uint64_t views_capacity, n_view_entries;
	uint32_t* view_ids;
	float* view_weights;
	/* optional: which pixels of image claim_image ended up in a fused point (arrDepthIdx != NO_ID), W*H bytes */
	uint32_t claim_image;
	uint8_t* claim_mask;
	/* optional (NULL: not wanted): n_maps pointers, each NULL or W*H values of that image -- per estimate the position in the fusion
	 * order of the pass whose point holds it when the fusion ends (the pass of the point's seed pixel), 0xFFFF = it belongs to no point */
	uint16_t** owner;
} hcor_cloud;

/* MVS::EstimatePointColors (DM.cpp:2125-2161): colour of the closest view of each point, bilinear over 8-bit pixels with every
 * product and sum truncated to 8 bits (Types.inl:2250-2258, Types.h:1931), white outside.  views: CSR like hcor_cloud */
void hcor_estimate_point_colors(const hcor_depthmap* maps, int n_maps, uint64_t n_points, const float* xyz, const uint32_t* n_views,
                                const uint32_t* view_ids, uint8_t* bgr);

/* SD.cpp:3265-3495 FuseDepthMaps.  order: image ids sorted by #neighbours descending (SD.cpp:3302;
 * ties broken by ascending id here -- std::sort leaves them unspecified).  returns 0 ok, 1 = capacity */
/* pixel visiting order of hcor_fuse_depthmaps / hcor_postfilter: 0 raster (the reference's), 1 the hashed order of the C-ABI's
 * hcmvs_set_fuse_order(ctx, 1) */
void hcor_set_fuse_pixel_order(int mode);
int hcor_fuse_depthmaps(hcor_depthmap* maps, int n_maps, const uint32_t* order, int n_order,
                        int n_min_views_fuse, float depth_diff_threshold, float normal_diff_deg,
                        float depthweight, float normalweight, hcor_cloud* cloud);

/* The fork's depth-map post-filters, applied to every image after outer iterations 1 and 2 (SD.cpp:3939-3958):
 *   RemoveSmallSegments as the fork rewrote it (SD.cpp:2048-2275): a complete FuseDepthMaps pass over the current maps of all
 *     images (it zeroes the estimates fused points occlude, in every image, like the final fusion), after which
 *     depthMap_fuse / normalMap_fuse = this image's maps restricted to the pixels that ended up in a fused point;
 *   GapInterpolation (SD.cpp:2280-3001): gaps of depthMap_fuse along rows, then along columns, are filled by linear
 *     interpolation of depth and of the normal's (atan2, acos) direction when they are at most nIpolGapSize = 7 pixels long and
 *     their ends agree within 2.5 x fDepthDiffThreshold, or longer and either that or the gradient-map values at the ends differ
 *     by at most 10 %; the confidence of a filled pixel is the smaller of the two ends'.  Finally depthMap / normalMap take the
 *     fused-and-filled values wherever those are valid (SD.cpp:2989-3000).
 * Restated: the row pass SD.cpp:2293-2447 and the column pass SD.cpp:2560-2713 (their live branches; `u == size.x` and
 * `(u-count) == 0` can not be true inside the loops).  NOT restated: the third, per-pixel pass (SD.cpp:2717-2983): it reads
 * variables that are never initialised (dir1, dirDiffsum, x1_demin ... at SD.cpp:2745-2760, 2782-2791) and divides by counters
 * that may be zero, so it has no defined result to match.  gra: the image's u8 gradient map.  mode: HCOR_ARITH_*.
 * maps[id]'s depth / normal / conf are updated in place; other images' depths may be zeroed by the fusion.  The fusion inside
 * RemoveSmallSegments uses the plain thresholds (SD.cpp:2083, 2177), not the --depthweight / --normalweight ones of FuseDepthMaps. */
int hcor_postfilter(hcor_depthmap* maps, int n_maps, uint32_t id, const uint8_t* gra, const uint32_t* order, int n_order, int n_min_views_fuse,
                    float depth_diff_threshold, float normal_diff_deg, int gap_size, int mode, uint64_t* n_filled);
/* the same, with the owner maps (hcor_cloud::owner) of the fusion inside RemoveSmallSegments: owner NULL = hcor_postfilter */
int hcor_postfilter_owners(hcor_depthmap* maps, int n_maps, uint32_t id, const uint8_t* gra, const uint32_t* order, int n_order, int n_min_views_fuse,
                           float depth_diff_threshold, float normal_diff_deg, int gap_size, int mode, uint64_t* n_filled, uint16_t** owner);

#ifdef __cplusplus
}
#endif
#endif

/*
 * tests/oracle_mask.c -- TEST INFRASTRUCTURE: the oracle's estimate with --ignore-mask-label (DepthMap.cpp:233-248, 319-381;
 * SceneDensify.cpp:649-744, 776-860).  Includes the oracle as it is and restates its three passes over the pixels the keep-mask
 * leaves in the visiting order (MapMatrix2ZigzagIdx drops the others from `coords`):
 *   ApplyIgnoreMask (depth, normal, conf = 0 on ignored pixels) -> median -> score pass -> sweeps -> end pass,
 * where no pass writes an ignored pixel: it ends holding the median's depth, normal 0, conf 0.  The per-pixel bodies are the
 * oracle's own static score_one / process_pixel, so a mask that keeps every pixel computes exactly hcor_estimate.
 * Built with oracle/Makefile's CFLAGS (-ffp-contract=off -mavx2 -mfma) into tests/libhcmvs_oracle_mask.so.
 */
#include "../oracle/hcmvs_oracle.c"

/* keep: w*h bytes, 1 = estimated, 0 = ignored; NULL = no mask */
static inline int kept(const uint8_t* keep, long i) { return !keep || keep[i]; }

void hcor_mask_apply(const uint8_t* keep, int W, int H, float* depth, float* normal, float* conf) {
	for (long i = 0; i < (long)W * H; ++i)
		if (!kept(keep, i)) { depth[i] = 0; normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0; conf[i] = 0; }
}

void hcor_mask_pass_score(const hcor_view* ref, const hcor_view* srcs, int V, const uint8_t* gra, const hcor_params* p, const uint8_t* keep,
                          float dMin, float dMax, float* depth, float* normal, float* conf, uint64_t* evals) {
	const int W = ref->width, H = ref->height;
	uint64_t total = 0;
	const int nt = p->n_threads > 0 ? p->n_threads : 1;
	(void)nt;
#pragma omp parallel num_threads(nt) reduction(+ : total)
	{
		est_ctx c;
		ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
#pragma omp for schedule(dynamic, 4)
		for (int y = 0; y < H; ++y)
			for (int x = 0; x < W; ++x)
				if (kept(keep, (long)y * W + x)) score_one(&c, x, y, depth, normal, conf);
		total += c.evals;
	}
	if (evals) *evals += total;
}

void hcor_mask_pass_sweep(const hcor_view* ref, const hcor_view* srcs, int V, const uint8_t* gra, const hcor_params* p, const uint8_t* keep,
                          int iter, float dMin, float dMax, float* depth, float* normal, float* conf, uint64_t* evals) {
	const int W = ref->width, H = ref->height;
	const int rev = (iter % 2) != 0;
	if (p->order == HCOR_ORDER_ZIGZAG) { /* the zig-zag coords without the ignored pixels, forward or reversed */
		est_ctx c;
		ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
		uint16_t* coords = (uint16_t*)malloc(sizeof(uint16_t) * 2 * (size_t)W * H);
		const int stride = 8 * p->n_threads > 64 ? 8 * p->n_threads : 64;
		const int n = hcor_zigzag_coords(W, H, stride, coords);
		for (int i = 0; i < n; ++i) {
			const int k = rev ? n - 1 - i : i;
			const int x = coords[2 * k], y = coords[2 * k + 1];
			if (kept(keep, (long)y * W + x)) process_pixel(&c, x, y, iter, depth, normal, conf);
		}
		free(coords);
		if (evals) *evals += c.evals;
		return;
	}
	/* rows advancing with a one-pixel lag; an ignored pixel is passed over but its column still counts as done */
	const int nt = p->n_threads > 0 ? p->n_threads : 1;
	atomic_int* progress = (atomic_int*)calloc((size_t)H, sizeof(atomic_int));
	uint64_t total = 0;
#pragma omp parallel num_threads(nt) reduction(+ : total)
	{
		est_ctx c;
		ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
		int tid = 0, nth = 1;
#ifdef _OPENMP
		tid = omp_get_thread_num(); nth = omp_get_num_threads();
#endif
		for (int r = tid; r < H; r += nth) {
			const int y = rev ? H - 1 - r : r;
			for (int q = 0; q < W; ++q) {
				if (r > 0)
					while (atomic_load_explicit(&progress[r - 1], memory_order_acquire) < q + 1) {
					}
				const int x = rev ? W - 1 - q : q;
				if (kept(keep, (long)y * W + x)) process_pixel(&c, x, y, iter, depth, normal, conf);
				atomic_store_explicit(&progress[r], q + 1, memory_order_release);
			}
		}
		total += c.evals;
	}
	free(progress);
	if (evals) *evals += total;
}

void hcor_mask_pass_end(const hcor_params* p, const uint8_t* keep, int W, int H, float* depth, float* normal, float* conf) {
	for (long i = 0; i < (long)W * H; ++i) {
		if (!kept(keep, i)) continue;
		if (depth[i] <= 0 || conf[i] >= p->ncc_threshold_keep) {
			conf[i] = 0; normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0; depth[i] = 0;
		} else {
			conf[i] = conf[i] >= 1.f ? 0.f : 1.f - conf[i];
		}
	}
}

/* hcor_estimate with a keep-mask; conf is in/out like depth and normal (the mask zeroes it on ignored pixels) */
int hcor_mask_estimate(const hcor_view* ref, const hcor_view* srcs, int V, const uint8_t* gra, const hcor_params* p, const uint8_t* keep,
                       float dMin, float dMax, float* depth, float* normal, float* conf, uint64_t* evals) {
	if (V < 1 || V > HCOR_MAX_VIEWS) return 1;
	if (p->adapthalfwin < 1 || p->adapthalfwin > HCOR_MAX_HALF_WINDOW) return 1;
	const int W = ref->width, H = ref->height;
	if (evals) *evals = 0;
	hcor_mask_apply(keep, W, H, depth, normal, conf);
	if (p->median_blur) {
		float* tmp = (float*)malloc(sizeof(float) * (size_t)W * H);
		hcor_median3(depth, W, H, tmp);
		memcpy(depth, tmp, sizeof(float) * (size_t)W * H);
		free(tmp);
	}
	hcor_mask_pass_score(ref, srcs, V, gra, p, keep, dMin, dMax, depth, normal, conf, evals);
	for (int iter = 0; iter < p->n_estimation_iters; ++iter)
		hcor_mask_pass_sweep(ref, srcs, V, gra, p, keep, iter, dMin, dMax, depth, normal, conf, evals);
	if (p->it_external == p->n_external_iters - 1) hcor_mask_pass_end(p, keep, W, H, depth, normal, conf);
	return 0;
}

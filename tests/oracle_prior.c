/*
 * tests/oracle_prior.c -- TEST INFRASTRUCTURE: the oracle's estimate with a depth prior (DensifyPointCloud --n-para_prior, --sigma-prior,
 * --n-photo2geo; ScorePixelImage, DepthMap.cpp:941-954) and with a first-sweep offset (the reference's two extra sweeps,
 * SceneDensify.cpp:983-1031).  Includes the oracle as it is and restates only what the term changes: the per-view blend inside the pixel
 * score, and -- because the oracle's passes call its own pixel score -- the bodies that lead there (the init-score pixel, ProcessPixel
 * without the view-spread and hint blocks, which never come together with a prior, and an estimate entry).
 *
 * The term, from the reference's lines (not from the kernels), per source view, after the (1 - photometric_flow) scale and before the
 * two-best-views aggregation (DepthMap.cpp:987-1046); a view that left early with thRobust (DepthMap.cpp:558, 591) is not blended:
 *     if (it_external >= photo2geo && prior(x0) != 0) {
 *         dd = |prior - depth| / prior                      (Util.inl:658-664 DepthSimilarity)
 *         wP = EXP(-SQUARE(dd) / (2 * SQUARE(sigma_prior)))
 *         score = score * (1 - para_prior) + 2 * (1 - wP) * para_prior
 *     }
 * What the reference leaves undefined is defined as DESIGN.md section 5, D11 states it: the term applies where the prior is finite and
 * > 0 (the reference tests != 0 and asserts > 0); a negative, NaN or infinite prior is "no prior here".  The prior is active when a map
 * is given, para_prior > 0 and it_external >= photo2geo.
 *
 * Arithmetic.  HCOR_ARITH_REFERENCE follows the lines above operation by operation in float, with libm's expf.  HCOR_ARITH_DEVICE states
 * the association of the gfx950 kernels: dd = |prior - depth| / prior with an IEEE division, wP = pm_expf((dd * dd) * k) with
 * k = -1 / (2 * (sigma * sigma)) rounded once on the host, addend = (2 * (1 - wP)) * para_prior computed once per hypothesis,
 * score = score * (1 - para_prior) + addend with (1 - para_prior) rounded once on the host; nothing is fused.
 *
 * Whether a view failed is found without restating the two view scorers: the oracle's scorer is called a second time with one
 * smoothness factor of 0 -- a view that was scored then returns (1 - pf) * 0 = 0, one that left early returns thRobust (> 0).
 *
 * Counters as the library counts them: evals_prior = evaluations (ScorePixel calls) that blended the term, i.e. those of pixels with a
 * usable prior while the prior is active; pixels_prior = estimated pixels with a usable prior (those the init-score pass visits, or the
 * first sweep of a sweeps-only call).
 * Built with oracle/Makefile's CFLAGS (-ffp-contract=off) into tests/libhcmvs_oracle_prior.so (tests/oracle_prior_lib.py).
 */
#include "../oracle/hcmvs_oracle.c"

typedef struct {
	const float* map;  /* W * H, NULL = none */
	float para_prior, sigma_prior;
	int photo2geo;
} hcor_prior;

typedef struct {
	int active;
	const float* map;
	float para, sigma;   /* reference association */
	float keep, sigmaK;  /* device association: 1 - para_prior, -1 / (2 sigma^2) */
	uint64_t evals_prior, pixels_prior;
} prior_ctx;

static void prior_init(prior_ctx* pc, const est_ctx* c, const hcor_prior* pr) {
	memset(pc, 0, sizeof *pc);
	if (!pr) return;
	pc->active = pr->map && pr->para_prior > 0.f && c->p.it_external >= pr->photo2geo;
	pc->map = pr->map; pc->para = pr->para_prior; pc->sigma = pr->sigma_prior;
	pc->keep = 1.f - pr->para_prior;
	pc->sigmaK = -1.f / (2.f * (pr->sigma_prior * pr->sigma_prior));
}

/* what prior_init derives for the device association: out[0] = 1 - para_prior, out[1] = -1 / (2 sigma^2) */
void hcor_prior_consts(float para, float sigma, float* out) {
	est_ctx c;
	memset(&c, 0, sizeof c);
	const float one = 1.f;
	const hcor_prior pr = {&one, para, sigma, 0};
	prior_ctx pc;
	prior_init(&pc, &c, &pr);
	out[0] = pc.keep; out[1] = pc.sigmaK;
}

int hcor_prior_usable(float prior) { return prior > 0.f && prior < INFINITY; } /* D11: finite and > 0 */

/* 2 (1 - wP) para_prior of one hypothesis */
static float prior_addend_of(int mode, float prior, float depth, float para, float sigma, float sigmaK) {
	if (mode == HCOR_ARITH_DEVICE) {
		const float dd = fabsf(prior - depth) / prior;
		const float wP = pm_expf((dd * dd) * sigmaK);
		return (2.f * (1.f - wP)) * para;
	}
	const float dd = fabsf(prior - depth) / prior;                 /* DepthSimilarity */
	const float wP = expf(-SQ(dd) / (2 * SQ(sigma)));              /* DepthMap.cpp:948 */
	return 2 * (1.f - wP) * para;                                  /* DepthMap.cpp:950, the right-hand summand */
}
float hcor_prior_addend(float prior, float depth, float para, float sigma, int mode) {
	return prior_addend_of(mode, prior, depth, para, sigma, -1.f / (2.f * (sigma * sigma)));
}
/* DepthMap.cpp:950 on a view's score */
float hcor_prior_blend(float score, float prior, float depth, float para, float sigma, int mode) {
	if (!hcor_prior_usable(prior)) return score;
	const float add = hcor_prior_addend(prior, depth, para, sigma, mode);
	if (mode == HCOR_ARITH_DEVICE) { const float keep = 1.f - para; return score * keep + add; }
	return score * (1.f - para) + add;
}

/* one view's score with the term: prior = the pixel's prior value, 0 when it has no usable one or the prior is not active */
static float prior_score_view(const est_ctx* c, const prior_ctx* pc, const pix_state* ps, int v, float depth, const float* normal, const float* sf,
                              int nsf, float prior, float addend) {
	const int dev = c->p.arith_mode == HCOR_ARITH_DEVICE;
	const float s = dev ? score_view_dev(c, ps, v, depth, normal, sf, nsf) : score_view_ref(c, ps, v, depth, normal, sf, nsf);
	if (!(prior > 0.f)) return s;
	const float zero = 0.f; /* a view that was scored returns (1 - pf) * 0 here, one that left early thRobust */
	const float probe = dev ? score_view_dev(c, ps, v, depth, normal, &zero, 1) : score_view_ref(c, ps, v, depth, normal, &zero, 1);
	if (probe == c->thRobust) return s;
	return dev ? s * pc->keep + addend : s * (1.f - pc->para) + addend;
}

/* DM.cpp:987-1046 ScorePixel, the oracle's score_pixel with the blended view scores; view_out (optional): the V view scores */
static float prior_score_pixel(est_ctx* c, prior_ctx* pc, const pix_state* ps, float depth, const float* normal, float prior, float* view_out) {
	float sf[HCOR_MAX_NEIGHBORS];
	int nsf = smooth_factors(c, ps, depth, normal, sf);
	if (c->p.arith_mode == HCOR_ARITH_DEVICE) {
		float bySlot[HCOR_MAX_NEIGHBORS];
		int top = 0;
		for (int k = 0; k < HCOR_MAX_NEIGHBORS; ++k) bySlot[k] = 1.f;
		for (int k = 0; k < nsf; ++k) { bySlot[ps->cSlot[k]] = sf[k]; if (ps->cSlot[k] + 1 > top) top = ps->cSlot[k] + 1; }
		float F = 1.f;
		for (int ch = 0; ch * 8 < top; ++ch) {
			const float* f = bySlot + ch * 8;
			const float t = ((f[0] * f[1]) * (f[2] * f[3])) * ((f[4] * f[5]) * (f[6] * f[7]));
			F = ch == 0 ? t : F * t;
		}
		sf[0] = F;
		nsf = 1;
	}
	const float addend = prior > 0.f ? prior_addend_of(c->p.arith_mode, prior, depth, pc->para, pc->sigma, pc->sigmaK) : 0.f;
	float s0 = FLT_MAX, s1 = FLT_MAX;
	for (int v = 0; v < c->V; ++v) {
		const float s = prior_score_view(c, pc, ps, v, depth, normal, sf, nsf, prior, addend);
		if (view_out) view_out[v] = s;
		if (s < s0) { s1 = s0; s0 = s; }
		else if (s < s1) s1 = s;
	}
	c->evals++;
	if (prior > 0.f) pc->evals_prior++;
	if (c->V <= 1) return s0;
	if (s1 >= c->thRobust) return s0;
	return (s0 + s1) / 2;
}

static float prior_at(const prior_ctx* pc, int idx) {
	return pc->active && hcor_prior_usable(pc->map[idx]) ? pc->map[idx] : 0.f;
}

/* ScorePixel over all views without smoothness neighbours, with a prior value at the pixel (known-answer tests); view_scores: V floats */
float hcor_prior_score_pixel(const hcor_view* ref, const hcor_view* srcs, int n_src, const uint8_t* gra, const hcor_params* p, int x, int y,
                             float depth, const float normal[3], float prior, float para, float sigma, int photo2geo, float* view_scores) {
	est_ctx c;
	ctx_init(&c, ref, srcs, n_src, gra, p, 0.f, 1.f);
	const hcor_prior pr = {&prior, para, sigma, photo2geo};
	prior_ctx pc;
	prior_init(&pc, &c, &pr);
	pix_state ps;
	fill_patch(&c, &ps, x, y);
	return prior_score_pixel(&c, &pc, &ps, depth, normal, pc.active && hcor_prior_usable(prior) ? prior : 0.f, view_scores);
}

/* the oracle's score_one (SD.cpp:649-675) calling the score above */
static void prior_score_one(est_ctx* c, prior_ctx* pc, int x, int y, float* depth, float* normal, float* conf) {
	const int W = c->ref->width;
	const int idx = y * W + x;
	if (!border_ok(c, x, y)) {
		depth[idx] = 0; normal[3 * idx] = normal[3 * idx + 1] = normal[3 * idx + 2] = 0; conf[idx] = 2.f;
		return;
	}
	pix_state ps;
	fill_patch(c, &ps, x, y);
	float d = depth[idx];
	float n[3] = {normal[3 * idx], normal[3 * idx + 1], normal[3 * idx + 2]};
	const uint32_t st = STREAM_SCORE(c->p.it_external);
	if (!(c->dMin <= d && d < c->dMax)) {
		d = random_depth(c, rand_unit(hcor_rand_u32(c->p.seed, (uint32_t)idx, st, 0)));
		random_normal(c, ps.viewDir, rand_unit(hcor_rand_u32(c->p.seed, (uint32_t)idx, st, 1)),
		              rand_unit(hcor_rand_u32(c->p.seed, (uint32_t)idx, st, 2)), n);
	} else if (dot3f(n, ps.viewDir) >= 0) {
		random_normal(c, ps.viewDir, rand_unit(hcor_rand_u32(c->p.seed, (uint32_t)idx, st, 1)),
		              rand_unit(hcor_rand_u32(c->p.seed, (uint32_t)idx, st, 2)), n);
	}
	depth[idx] = d; normal[3 * idx] = n[0]; normal[3 * idx + 1] = n[1]; normal[3 * idx + 2] = n[2];
	conf[idx] = prior_score_pixel(c, pc, &ps, d, n, prior_at(pc, idx), NULL);
}

/* the oracle's process_pixel (DM.cpp:1050-1501) calling the score above; count: this sweep counts the pixels with a usable prior */
static void prior_process_pixel(est_ctx* c, prior_ctx* pc, int x, int y, int iter, int count, float* depthMap, float* normalMap, float* confMap) {
	const hcor_view* ref = c->ref;
	const int W = ref->width, H = ref->height, hw7 = border_of(&c->p);
	if (!border_ok(c, x, y)) return;
	pix_state ps;
	fill_patch(c, &ps, x, y);
	const int rev = (iter % 2) != 0;
	int nbx[HCOR_MAX_NEIGHBORS], nby[HCOR_MAX_NEIGHBORS], nbc[HCOR_MAX_NEIGHBORS];
	int nNb = 0;
	if (c->p.it_external >= 1) {
		const float tx = (float)c->gra[y * W + x];
		int phw = tx > 150 ? 5 : c->p.propagate_halfwin;
		if (phw > 7) phw = 7;
		const int step = c->p.propagate_step > 0 ? c->p.propagate_step : 1;
		int cx[HCOR_MAX_NEIGHBORS], cy[HCOR_MAX_NEIGHBORS], nc = 0;
		if (x > phw && y > phw && x < W - phw && y < H - phw) {
			for (int i = 1; i <= phw; i += step) {
				cx[nc] = x; cy[nc++] = y - i;
				cx[nc] = x; cy[nc++] = y + i;
				cx[nc] = x - i; cy[nc++] = y;
				cx[nc] = x + i; cy[nc++] = y;
			}
		} else if (x > hw7 && y > hw7 && x < W - hw7 && y < H - hw7) {
			cx[nc] = x; cy[nc++] = y - 1;
			cx[nc] = x; cy[nc++] = y + 1;
			cx[nc] = x - 1; cy[nc++] = y;
			cx[nc] = x + 1; cy[nc++] = y;
		}
		for (int k = 0; k < nc; ++k) {
			const float nd = depthMap[cy[k] * W + cx[k]];
			if (nd > 0) {
				nbx[nNb] = cx[k]; nby[nNb] = cy[k]; nbc[nNb] = ps.nClose; ++nNb;
				add_close(c, &ps, cx[k], cy[k], nd, normalMap, k);
			}
		}
	} else {
		const int px[4] = {x - 1, x, x + 1, x}, py[4] = {y, y - 1, y, y + 1};
		const int valid[4] = {x > hw7, y > hw7, x < W - hw7, y < H - hw7};
		const int order_fwd[4] = {0, 1, 2, 3}, order_rev[4] = {2, 3, 0, 1};
		const int* ord = rev ? order_rev : order_fwd;
		for (int q = 0; q < 4; ++q) {
			const int k = ord[q];
			if (!valid[k]) continue;
			const float nd = depthMap[py[k] * W + px[k]];
			if (nd > 0) {
				if (q < 2) { nbx[nNb] = px[k]; nby[nNb] = py[k]; nbc[nNb] = ps.nClose; ++nNb; }
				add_close(c, &ps, px[k], py[k], nd, normalMap, q);
			}
		}
	}
	const int idx = y * W + x;
	const float prior = prior_at(pc, idx);
	if (count && prior > 0.f) pc->pixels_prior++;
	float conf = confMap[idx], depth = depthMap[idx];
	float normal[3] = {normalMap[3 * idx], normalMap[3 * idx + 1], normalMap[3 * idx + 2]};
	init_plane(&ps, depth, normal);
	for (int q = 0; q < nNb; ++q) { /* propagation, DM.cpp:1406-1440 */
		if (confMap[nby[q] * W + nbx[q]] >= c->p.ncc_threshold_keep) continue;
		const int k = nbc[q];
		ps.cDepth[k] = interpolate_pixel(c, &ps, nbx[q], nby[q], ps.cDepth[k], ps.cNormal[k]);
		correct_normal(c->mt, ps.viewDir, ps.cNormal[k]);
		init_plane(&ps, ps.cDepth[k], ps.cNormal[k]);
		const float nconf = prior_score_pixel(c, pc, &ps, ps.cDepth[k], ps.cNormal[k], prior, NULL);
		if (conf > nconf) {
			conf = nconf; depth = ps.cDepth[k];
			normal[0] = ps.cNormal[k][0]; normal[1] = ps.cNormal[k][1]; normal[2] = ps.cNormal[k][2];
		}
	}
	const uint32_t st = STREAM_SWEEP(c->p.it_external, iter); /* refinement, DM.cpp:1442-1501 */
	const uint32_t seed = c->p.seed;
	unsigned idxScaleRange = 0;
	int done = 0;
	for (;;) {
		if (conf <= c->thConfSmall) idxScaleRange = 2;
		else if (conf <= c->thConfBig) idxScaleRange = 1;
		else if (conf >= c->thConfRand) {
			int again = 0;
			for (int it = 0; it < c->p.n_random_iters; ++it) {
				const float nd = random_depth(c, rand_unit(hcor_rand_u32(seed, (uint32_t)idx, st, 3u * it)));
				float nn[3];
				random_normal(c, ps.viewDir, rand_unit(hcor_rand_u32(seed, (uint32_t)idx, st, 3u * it + 1)),
				              rand_unit(hcor_rand_u32(seed, (uint32_t)idx, st, 3u * it + 2)), nn);
				const float nconf = prior_score_pixel(c, pc, &ps, nd, nn, prior, NULL);
				if (conf > nconf) {
					conf = nconf; depth = nd; normal[0] = nn[0]; normal[1] = nn[1]; normal[2] = nn[2];
					if (conf < c->thConfRand) { again = 1; break; }
				}
			}
			if (again) continue;
			done = 1;
		}
		break;
	}
	if (!done) {
		float scaleRange = 1.f / (float)(1u << idxScaleRange);
		const float depthRange = depth * c->p.random_depth_ratio;
		float p[2];
		normal2dir(c->mt, normal, p);
		for (int it = 0; it < c->p.n_random_iters; ++it) {
			const uint32_t cb = 64u + 3u * it;
			const float nd = depth + (depthRange * scaleRange) * (2.f * rand_unit(hcor_rand_u32(seed, (uint32_t)idx, st, cb)) - 1.f);
			if (!(c->dMin <= nd && nd < c->dMax)) continue;
			const float np[2] = {
				p[0] + (c->angle1Range * scaleRange) * (2.f * rand_unit(hcor_rand_u32(seed, (uint32_t)idx, st, cb + 1)) - 1.f),
				p[1] + (c->angle2Range * scaleRange) * (2.f * rand_unit(hcor_rand_u32(seed, (uint32_t)idx, st, cb + 2)) - 1.f)};
			float nn[3];
			dir2normal(c->mt, np, nn);
			if (dot3f(nn, ps.viewDir) >= 0) continue;
			init_plane(&ps, nd, nn);
			const float nconf = prior_score_pixel(c, pc, &ps, nd, nn, prior, NULL);
			if (conf > nconf) {
				conf = nconf; depth = nd; normal[0] = nn[0]; normal[1] = nn[1]; normal[2] = nn[2];
				p[0] = np[0]; p[1] = np[1];
				++idxScaleRange;
				scaleRange = 1.f / (float)(1u << idxScaleRange);
			}
		}
	}
	confMap[idx] = conf; depthMap[idx] = depth;
	normalMap[3 * idx] = normal[0]; normalMap[3 * idx + 1] = normal[1]; normalMap[3 * idx + 2] = normal[2];
}

/* One estimate of ref against srcs with the prior `pr` (NULL or map == NULL: none).
 *   sweeps_only == 0: hcor_estimate's passes -- mask, median, init score, sweeps 0 .. n_estimation_iters - 1, end pass when
 *                     it_external == n_external_iters - 1 (first_sweep and n_sweeps are not used);
 *   sweeps_only != 0: the maps are taken as the state an estimate leaves between outer iterations (depth, normal, conf = the score):
 *                     sweeps first_sweep .. first_sweep + n_sweeps - 1, then the end pass under the same condition.
 * The pixels are visited in raster order (reversed on odd sweeps): one of the orders the oracle's sweeps are invariant under
 * (hcor_pass_sweep).  The hint and view spread of p are refused with an active prior (return 2), as the library refuses them.
 * stats (optional): evals, evals_prior, pixels_prior. */
int hcor_prior_estimate(const hcor_view* ref, const hcor_view* srcs, int V, const uint8_t* gra, const hcor_params* p, float dMin, float dMax,
                        float* depth, float* normal, float* conf, const hcor_prior* pr, int sweeps_only, int first_sweep, int n_sweeps,
                        uint64_t* stats) {
	if (V < 1 || V > HCOR_MAX_VIEWS) return 1;
	if (p->adapthalfwin < 1 || p->adapthalfwin > HCOR_MAX_HALF_WINDOW) return 1;
	if (!(p->ncc_threshold_keep > 0.f)) return 1; /* thRobust > 0: what tells a failed view from a scored one above */
	if (sweeps_only && (first_sweep < 0 || n_sweeps < 1 || first_sweep + n_sweeps > 63)) return 1;
	const int W = ref->width, H = ref->height;
	est_ctx c;
	ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
	prior_ctx pc;
	prior_init(&pc, &c, pr);
	if (pc.active && (c.spread || (!sweeps_only && p->hint_depth && p->hint_normal && p->it_external == p->n_external_iters - 1))) return 2;
	if (c.spread || p->hint_depth) return 1; /* this entry has neither block */
	if (!sweeps_only) {
		for (long i = 0; i < (long)W * H; ++i) /* DepthData::ApplyIgnoreMask */
			if (!kept(p, i)) { depth[i] = 0; normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0; conf[i] = 0; }
		if (p->median_blur) {
			float* tmp = (float*)malloc(sizeof(float) * (size_t)W * H);
			hcor_median3(depth, W, H, tmp);
			memcpy(depth, tmp, sizeof(float) * (size_t)W * H);
			free(tmp);
		}
		for (int y = 0; y < H; ++y)
			for (int x = 0; x < W; ++x)
				if (kept(p, (long)y * W + x)) {
					prior_score_one(&c, &pc, x, y, depth, normal, conf);
					if (border_ok(&c, x, y) && prior_at(&pc, y * W + x) > 0.f) pc.pixels_prior++;
				}
		first_sweep = 0; n_sweeps = p->n_estimation_iters;
	}
	for (int iter = first_sweep; iter < first_sweep + n_sweeps; ++iter) {
		const int rev = (iter % 2) != 0;
		for (long i = 0; i < (long)W * H; ++i) {
			const long k = rev ? (long)W * H - 1 - i : i;
			const int x = (int)(k % W), y = (int)(k / W);
			if (kept(p, k)) prior_process_pixel(&c, &pc, x, y, iter, sweeps_only && iter == first_sweep, depth, normal, conf);
		}
	}
	if (p->it_external == p->n_external_iters - 1) hcor_pass_end(p, W, H, depth, normal, conf);
	if (stats) { stats[0] = c.evals; stats[1] = pc.evals_prior; stats[2] = pc.pixels_prior; }
	return 0;
}

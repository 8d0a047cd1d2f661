/*
 * tests/oracle_geo.c -- TEST INFRASTRUCTURE: the oracle's estimate with the geometric-consistency term (DensifyPointCloud --geo-consistency;
 * DESIGN.md section 5, D14).  Includes the oracle as it is and restates only what the term changes: the per-view blend inside the pixel
 * score, and -- because the oracle's passes call its own pixel score -- the bodies that lead there (the init-score pixel, ProcessPixel
 * without the view-spread and hint blocks, which never come together with the term, and an estimate entry).
 *
 * The term, from D14 (not from the kernels).  The pixel's weight goes by its texture g = gra[y * W + x]: w = para_tapa where
 * g < txthreshold, else para_tapa2 where g < txthreshold2, else 0 (DepthMap.cpp:917-928); a pixel with w == 0 is a plain pixel.  Per
 * (hypothesis (d, n), source view j), all in float, fmaf where written, IEEE divisions and square roots, nothing else fused:
 *   1. H = the hypothesis' homography as the scorer forms it; X = (fmaf(H1, y, fmaf(H0, x, H2)), ..), iz = 1 / Xz, x1 = (Xx iz, Xy iz)
 *   2. fu = floorf(x1x + 0.5f), fv likewise; NEUTRAL when view j offers no maps, when !(fu >= 0 && fv >= 0 && fu < w_j && fv < h_j), or
 *      when z = D_j[fv * w_j + fu] is not finite and > 0
 *   3. Xc0 = ((x1x - cx_j) * z) * ifx_j, Xc1 = ((x1y - cy_j) * z) * ify_j; p_i = fmaf(B_i2, z, fmaf(B_i1, Xc1, fmaf(B_i0, Xc0, b_i)));
 *      NEUTRAL when !(p2 > 0); ip = 1 / p2, ex = x - p0 * ip, ey = y - p1 * ip, e = sqrtf(fmaf(ey, ey, ex * ex))
 *   4. m_i = fmaf(Rr_i2, N2, fmaf(Rr_i1, N1, Rr_i0 * N0)) with N = N_j[fu, fv]; nn = fmaf(n2, n2, fmaf(n1, n1, n0 * n0)), mm likewise,
 *      q = nn * mm; NEUTRAL when !(q > 0); c = fminf(1, |fmaf(n2, m2, fmaf(n1, m1, n0 * m0))| / sqrtf(q))
 *   5. geo = e < max_px ? e / max_px + (1 - c) : 2; a neutral pair has geo = 1
 *   6. s = s * (1 - w) + w * geo on a view that was scored (a failed view stays thRobust), 1 - w rounded once
 * with B = K_i R_i R_j^T, b = K_i R_i (C_j - C_i), Rr = R_i R_j^T, cx_j .. ify_j computed in double and rounded to float once.
 * The homography is the device association's (HCOR_ARITH_DEVICE is required while the term is active): D14 defines the term on the
 * floats the scorer holds.
 *
 * Whether a view failed is found without restating the view scorer: it is called a second time with one smoothness factor of 0 -- a
 * view that was scored then returns (1 - pf) * 0 = 0, one that left early returns thRobust (> 0).
 *
 * Counters as the library counts them -- evals, evals_geo (evaluations of pixels with w > 0 while the term is active), pixels_geo
 * (estimated pixels with w > 0) -- and, for the tests' conditions on their inputs, the blended pairs by class and the estimated pixels
 * by weight.  Built with oracle/Makefile's CFLAGS (-ffp-contract=off) into tests/libhcmvs_oracle_geo.so (tests/oracle_geo_lib.py).
 */
#include "../oracle/hcmvs_oracle.c"

typedef struct {
	int on;
	float para_tapa, para_tapa2, txthreshold, txthreshold2;
	int photo2geo;
	float max_px;
} hcor_geo_params;

enum { GEO_CONSISTENT = 0, GEO_WORST, GEO_OUTSIDE, GEO_NODEPTH, GEO_BEHIND, GEO_NOMAPS, GEO_CLASSES };

typedef struct { float cx, cy, ifx, ify, B[9], b[3], Rr[9]; } geo_view;

typedef struct {
	int active;
	hcor_geo_params gp;
	const hcor_spread_map* maps; /* one entry per source view */
	geo_view gv[HCOR_MAX_VIEWS];
	float keep1, keep2;
	uint64_t evals_geo, pixels_geo, pixels_w[3]; /* pixels_w: para_tapa, para_tapa2, 0 */
	uint64_t pairs[GEO_CLASSES];     /* the blended pairs by class */
	uint64_t pairs_all[GEO_CLASSES]; /* the pairs of the pixels with a weight by class, those of failed views (never blended) included */
} geo_ctx;

/* B, b, Rr and the intrinsics of view j as D14 holds them: double, rounded once */
static void geo_view_of(const hcor_view* ref, const hcor_view* s, geo_view* g) {
	double KR[9], B[9], Rr[9];
	mat3_mul(ref->K, ref->R, KR);
	mat3_mul_bt(KR, s->R, B);
	mat3_mul_bt(ref->R, s->R, Rr);
	const double dC[3] = {s->C[0] - ref->C[0], s->C[1] - ref->C[1], s->C[2] - ref->C[2]};
	for (int i = 0; i < 9; ++i) { g->B[i] = (float)B[i]; g->Rr[i] = (float)Rr[i]; }
	for (int i = 0; i < 3; ++i) g->b[i] = (float)(KR[i * 3] * dC[0] + KR[i * 3 + 1] * dC[1] + KR[i * 3 + 2] * dC[2]);
	g->cx = (float)s->K[2]; g->cy = (float)s->K[5]; g->ifx = (float)(1.0 / s->K[0]); g->ify = (float)(1.0 / s->K[4]);
}
/* out: cx, cy, ifx, ify, B[9], b[3], Rr[9] (25 floats) */
void hcor_geo_view_consts(const hcor_view* ref, const hcor_view* src, float* out) {
	geo_view g;
	geo_view_of(ref, src, &g);
	out[0] = g.cx; out[1] = g.cy; out[2] = g.ifx; out[3] = g.ify;
	memcpy(out + 4, g.B, sizeof g.B); memcpy(out + 13, g.b, sizeof g.b); memcpy(out + 16, g.Rr, sizeof g.Rr);
}

static void geo_init(geo_ctx* gc, const est_ctx* c, const hcor_geo_params* gp, const hcor_spread_map* maps) {
	memset(gc, 0, sizeof *gc);
	if (!gp) return;
	gc->gp = *gp; gc->maps = maps;
	int offers = 0;
	for (int v = 0; maps && v < c->V; ++v) offers = offers || maps[v].depth != NULL;
	gc->active = gp->on && c->p.it_external >= gp->photo2geo && offers;
	gc->keep1 = 1.f - gp->para_tapa; gc->keep2 = 1.f - gp->para_tapa2;
	for (int v = 0; v < c->V; ++v) geo_view_of(c->ref, &c->srcs[v], &gc->gv[v]);
}

/* the pixel's weight by its texture (DepthMap.cpp:917-928); which (optional): 0 para_tapa, 1 para_tapa2, 2 none */
static float geo_weight(const hcor_geo_params* gp, uint8_t gra, float* keep, int* which) {
	const float g = (float)gra;
	const int k = g < gp->txthreshold ? 0 : (g < gp->txthreshold2 ? 1 : 2);
	if (which) *which = k;
	if (keep) *keep = 1.f - (k == 0 ? gp->para_tapa : gp->para_tapa2);
	return k == 0 ? gp->para_tapa : (k == 1 ? gp->para_tapa2 : 0.f);
}
float hcor_geo_weight(const hcor_geo_params* gp, int gra) { return geo_weight(gp, (uint8_t)gra, NULL, NULL); }

/* steps 2-5 for where the centre pixel landed (x1x, x1y) in view j: geo, its class, and (optional) e and c */
static float geo_value(const geo_view* g, const hcor_spread_map* m, float max_px, float px, float py, float x1x, float x1y, const float* normal,
                       int* cls, float* e_out, float* c_out) {
	if (e_out) *e_out = 0.f;
	if (c_out) *c_out = 0.f;
	if (!m || !m->depth) { *cls = GEO_NOMAPS; return 1.f; }
	const float fu = floorf(x1x + 0.5f), fv = floorf(x1y + 0.5f);
	if (!(fu >= 0.f && fv >= 0.f && fu < (float)m->width && fv < (float)m->height)) { *cls = GEO_OUTSIDE; return 1.f; }
	const size_t at = (size_t)(int)fv * (size_t)m->width + (size_t)(int)fu;
	const float z = m->depth[at];
	if (!(z > 0.f && z < INFINITY)) { *cls = GEO_NODEPTH; return 1.f; }
	const float N0 = m->normal[3 * at], N1 = m->normal[3 * at + 1], N2 = m->normal[3 * at + 2];
	const float Xc0 = ((x1x - g->cx) * z) * g->ifx, Xc1 = ((x1y - g->cy) * z) * g->ify;
	float p[3], mm3[3];
	for (int i = 0; i < 3; ++i) {
		p[i] = fmaf(g->B[3 * i + 2], z, fmaf(g->B[3 * i + 1], Xc1, fmaf(g->B[3 * i], Xc0, g->b[i])));
		mm3[i] = fmaf(g->Rr[3 * i + 2], N2, fmaf(g->Rr[3 * i + 1], N1, g->Rr[3 * i] * N0));
	}
	if (!(p[2] > 0.f)) { *cls = GEO_BEHIND; return 1.f; }
	const float ip = 1.0f / p[2];
	const float ex = px - p[0] * ip, ey = py - p[1] * ip;
	const float e = sqrtf(fmaf(ey, ey, ex * ex));
	const float n0 = normal[0], n1 = normal[1], n2 = normal[2];
	const float nn = fmaf(n2, n2, fmaf(n1, n1, n0 * n0)), mm = fmaf(mm3[2], mm3[2], fmaf(mm3[1], mm3[1], mm3[0] * mm3[0]));
	const float q = nn * mm;
	if (!(q > 0.f)) { *cls = GEO_BEHIND; return 1.f; }
	const float dt = fmaf(n2, mm3[2], fmaf(n1, mm3[1], n0 * mm3[0]));
	const float cs = fminf(1.f, fabsf(dt) / sqrtf(q));
	if (e_out) *e_out = e;
	if (c_out) *c_out = cs;
	if (e < max_px) { *cls = GEO_CONSISTENT; return e / max_px + (1.f - cs); }
	*cls = GEO_WORST;
	return 2.f;
}

/* step 1, then geo_value, for source view v of the estimate */
static float geo_pair(const est_ctx* c, const geo_ctx* gc, const pix_state* ps, int v, float depth, const float* normal, int* cls, float* e_out,
                      float* c_out) {
	float H[9];
	device_H(c, ps, v, depth, normal, H);
	const float px = (float)ps->x, py = (float)ps->y;
	const float Xx = fmaf(H[1], py, fmaf(H[0], px, H[2]));
	const float Xy = fmaf(H[4], py, fmaf(H[3], px, H[5]));
	const float Xz = fmaf(H[7], py, fmaf(H[6], px, H[8]));
	const float iz = 1.0f / Xz;
	return geo_value(&gc->gv[v], gc->maps ? &gc->maps[v] : NULL, gc->gp.max_px, px, py, Xx * iz, Xy * iz, normal, cls, e_out, c_out);
}

/* one pair on hand-built inputs (known-answer tests): ref against ONE source view with the map `map` (NULL or depth == NULL: no maps);
 * out: geo, class, e, c, x1x, x1y */
void hcor_geo_pair(const hcor_view* ref, const hcor_view* src, const hcor_spread_map* map, const hcor_params* p, int x, int y, float depth,
                   const float normal[3], float max_px, float* out) {
	est_ctx c;
	ctx_init(&c, ref, src, 1, NULL, p, 0.f, 1.f);
	geo_ctx gc;
	hcor_geo_params gp = {1, 0.25f, 0.15f, 150.f, 160.f, 0, max_px};
	geo_init(&gc, &c, &gp, map);
	pix_state ps;
	memset(&ps, 0, sizeof ps);
	ps.x = x; ps.y = y;
	/* the view ray of the pixel, as fill_patch leaves it (device_H reads it) */
	ps.viewDir[0] = (float)(((double)x - ref->K[2]) * c.ifx); ps.viewDir[1] = (float)(((double)y - ref->K[5]) * c.ify); ps.viewDir[2] = 1.f;
	float H[9];
	device_H(&c, &ps, 0, depth, normal, H);
	const float px = (float)x, py = (float)y;
	const float iz = 1.0f / fmaf(H[7], py, fmaf(H[6], px, H[8]));
	out[4] = fmaf(H[1], py, fmaf(H[0], px, H[2])) * iz; out[5] = fmaf(H[4], py, fmaf(H[3], px, H[5])) * iz;
	int cls = 0;
	out[0] = geo_pair(&c, &gc, &ps, 0, depth, normal, &cls, &out[2], &out[3]);
	out[1] = (float)cls;
}
/* step 6 */
float hcor_geo_blend(float s, float w, float geo) { const float keep = 1.f - w; return s * keep + w * geo; }

/* DM.cpp:987-1046 ScorePixel, the oracle's score_pixel_views with the blended view scores; w: the pixel's weight, 0 for a plain pixel */
static float geo_score_pixel(est_ctx* c, geo_ctx* gc, const pix_state* ps, float depth, const float* normal, float w, float keep) {
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
	const int dev = c->p.arith_mode == HCOR_ARITH_DEVICE;
	float s0 = FLT_MAX, s1 = FLT_MAX;
	for (int v = 0; v < c->V; ++v) {
		float s = dev ? score_view_dev(c, ps, v, depth, normal, sf, nsf, 0.f) : score_view_ref(c, ps, v, depth, normal, sf, nsf, 0.f);
		if (w > 0.f) {
			const float zero = 0.f; /* a view that was scored returns (1 - pf) * 0 here, one that left early thRobust */
			const float probe = dev ? score_view_dev(c, ps, v, depth, normal, &zero, 1, 0.f) : score_view_ref(c, ps, v, depth, normal, &zero, 1, 0.f);
			int cls = 0;
			const float geo = geo_pair(c, gc, ps, v, depth, normal, &cls, NULL, NULL);
			gc->pairs_all[cls]++;
			if (probe != c->thRobust) {
				gc->pairs[cls]++;
				s = s * keep + w * geo;
			}
		}
		if (s < s0) { s1 = s0; s0 = s; }
		else if (s < s1) s1 = s;
	}
	c->evals++;
	if (w > 0.f) gc->evals_geo++;
	if (c->V <= 1) return s0;
	if (s1 >= c->thRobust) return s0;
	return (s0 + s1) / 2;
}

static float geo_w_at(const geo_ctx* gc, const est_ctx* c, long idx, float* keep) {
	*keep = 1.f;
	return gc->active ? geo_weight(&gc->gp, c->gra[idx], keep, NULL) : 0.f;
}

/* the oracle's score_one (SD.cpp:649-675) calling the score above */
static void geo_score_one(est_ctx* c, geo_ctx* gc, int x, int y, float* depth, float* normal, float* conf) {
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
	float keep;
	const float w = geo_w_at(gc, c, idx, &keep);
	conf[idx] = geo_score_pixel(c, gc, &ps, d, n, w, keep);
}

/* the oracle's process_pixel (DM.cpp:1050-1501) calling the score above */
static void geo_process_pixel(est_ctx* c, geo_ctx* gc, int x, int y, int iter, float* depthMap, float* normalMap, float* confMap) {
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
	float keep;
	const float w = geo_w_at(gc, c, idx, &keep);
	float conf = confMap[idx], depth = depthMap[idx];
	float normal[3] = {normalMap[3 * idx], normalMap[3 * idx + 1], normalMap[3 * idx + 2]};
	init_plane(&ps, depth, normal);
	for (int q = 0; q < nNb; ++q) { /* propagation, DM.cpp:1406-1440 */
		if (confMap[nby[q] * W + nbx[q]] >= c->p.ncc_threshold_keep) continue;
		const int k = nbc[q];
		ps.cDepth[k] = interpolate_pixel(c, &ps, nbx[q], nby[q], ps.cDepth[k], ps.cNormal[k]);
		correct_normal(c->mt, ps.viewDir, ps.cNormal[k]);
		init_plane(&ps, ps.cDepth[k], ps.cNormal[k]);
		const float nconf = geo_score_pixel(c, gc, &ps, ps.cDepth[k], ps.cNormal[k], w, keep);
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
				const float nconf = geo_score_pixel(c, gc, &ps, nd, nn, w, keep);
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
			const float nconf = geo_score_pixel(c, gc, &ps, nd, nn, w, keep);
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

/* One estimate of ref against srcs with the term gp (NULL: off) and the source views' maps (NULL: none; one entry per source view,
 * depth == NULL: that view offers none): hcor_estimate's passes -- mask, median, init score, sweeps 0 .. n_estimation_iters - 1, end
 * pass when it_external == n_external_iters - 1.  The pixels are visited in raster order (reversed on odd sweeps): one of the orders
 * the oracle's sweeps are invariant under (hcor_pass_sweep).  With the term active, the hint, view spread and a depth prior of p are
 * refused (return 2), as the library refuses them; this entry has none of the three blocks (return 1).
 * stats (optional, 18 entries): evals, evals_geo, pixels_geo, the blended pairs by class (consistent, worst, outside, no depth,
 * behind or degenerate, no maps), the estimated pixels by weight (para_tapa, para_tapa2, 0), the pairs of the pixels with a weight by
 * class, failed views included.  A view whose centre pixel lands outside view j's image has failed, so no BLENDED pair is ever of the
 * class `outside`; the class occurs among the pairs the scorer evaluates. */
int hcor_geo_estimate(const hcor_view* ref, const hcor_view* srcs, int V, const uint8_t* gra, const hcor_params* p, float dMin, float dMax,
                      float* depth, float* normal, float* conf, const hcor_geo_params* gp, const hcor_spread_map* maps, uint64_t* stats) {
	if (V < 1 || V > HCOR_MAX_VIEWS) return 1;
	if (p->adapthalfwin < 1 || p->adapthalfwin > HCOR_MAX_HALF_WINDOW) return 1;
	if (!(p->ncc_threshold_keep > 0.f)) return 1; /* thRobust > 0: what tells a failed view from a scored one above */
	const int W = ref->width, H = ref->height;
	est_ctx c;
	ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
	geo_ctx gc;
	geo_init(&gc, &c, gp, maps);
	const int hint = p->hint_depth && p->hint_normal && p->it_external == p->n_external_iters - 1;
	if (gc.active && (c.spread || hint || c.prior)) return 2;
	if (c.spread || p->hint_depth || c.prior) return 1;
	if (gc.active && p->arith_mode != HCOR_ARITH_DEVICE) return 1;
	for (long i = 0; i < (long)W * H; ++i) /* DepthData::ApplyIgnoreMask */
		if (!kept(p, i)) { depth[i] = 0; normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0; conf[i] = 0; }
	if (p->median_blur) {
		float* tmp = (float*)malloc(sizeof(float) * (size_t)W * H);
		hcor_median3(depth, W, H, tmp);
		memcpy(depth, tmp, sizeof(float) * (size_t)W * H);
		free(tmp);
	}
	for (int y = 0; y < H; ++y)
		for (int x = 0; x < W; ++x) {
			const long i = (long)y * W + x;
			if (!kept(p, i)) continue;
			geo_score_one(&c, &gc, x, y, depth, normal, conf);
			if (gc.active && border_ok(&c, x, y)) {
				int which;
				if (geo_weight(&gc.gp, gra[i], NULL, &which) > 0.f) gc.pixels_geo++;
				gc.pixels_w[which]++;
			}
		}
	for (int iter = 0; iter < p->n_estimation_iters; ++iter) {
		const int rev = (iter % 2) != 0;
		for (long i = 0; i < (long)W * H; ++i) {
			const long k = rev ? (long)W * H - 1 - i : i;
			if (kept(p, k)) geo_process_pixel(&c, &gc, (int)(k % W), (int)(k / W), iter, depth, normal, conf);
		}
	}
	if (p->it_external == p->n_external_iters - 1) hcor_pass_end(p, W, H, depth, normal, conf);
	if (stats) {
		stats[0] = c.evals; stats[1] = gc.evals_geo; stats[2] = gc.pixels_geo;
		for (int k = 0; k < GEO_CLASSES; ++k) stats[3 + k] = gc.pairs[k];
		for (int k = 0; k < 3; ++k) stats[9 + k] = gc.pixels_w[k];
		for (int k = 0; k < GEO_CLASSES; ++k) stats[12 + k] = gc.pairs_all[k];
	}
	return 0;
}

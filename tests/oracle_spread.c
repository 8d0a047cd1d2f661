/*
 * tests/oracle_spread.c -- TEST INFRASTRUCTURE: the oracle's estimate with view spread (DensifyPointCloud --n-viewspread,
 * DepthMap.cpp:1504-1608).  Includes the oracle as it is and restates its ProcessPixel with the spread block inserted between the
 * refinement trials and the `restore` hint; the sweep drivers (zig-zag, row-pipelined) are the oracle's, calling that body.
 *
 * The block, from the reference's lines (not from the kernels): from outer iteration 1 on, a pixel that did not leave through the
 * `return` of the full-random branch (DepthMap.cpp:1464) goes through its source views j = 1..V in order.  For each view that spreads:
 *   x1 = H_j(depth, normal) (x, y, 1) divided through, truncated to int (DepthMap.cpp:1515-1521);
 *   neighbors / neighborsClose / candidate are emptied (1523-1527);
 *   (x1.x, x1.y-1), (x1.x, x1.y+1), (x1.x-1, x1.y), (x1.x+1, x1.y) are candidates when 7 < x1.x < W-7 and 7 < x1.y < H-7, W x H the
 *   REFERENCE image's size (1532-1537, both sweep directions alike);
 *   a candidate with a positive depth in view j's map becomes a slot: that depth, view j's stored normal (not rotated) and
 *   X = TransformPointI2C(nx, depth) (1539-1554);
 *   the slots run in order; one whose conf in view j's map is >= fNCCThresholdKeep is skipped; otherwise its depth becomes the z of
 *   W2C_ref(float3(I2W_j(nx, depth))) (1590-1592), CorrectNormal, InitPlane, ScorePixel, accepted when conf > nconf (1583-1605).
 *
 * What the reference leaves undefined is defined here as DESIGN.md section 5, D10 states it:
 *   a view spreads iff it has spread maps of its own image size; a view that does not is passed over altogether (the smoothness
 *   set stays what it was); candidates must also lie inside view j's map (counted otherwise); X uses view j's own intrinsics; a
 *   slot whose transformed depth is not > 0 is not scored (counted) and stays in the smoothness set uncorrected; an x1 that is not
 *   finite yields no candidates.
 *
 * Arithmetic.  HCOR_ARITH_REFERENCE follows the lines above operation by operation.  HCOR_ARITH_DEVICE states the association of
 * the gfx950 kernel:
 *   x1: H in float as for every score (device_H), X = (fmaf(H1, y, fmaf(H0, x, H2)), fmaf(H4, y, fmaf(H3, x, H5)),
 *       fmaf(H7, y, fmaf(H6, x, H8))), x1 = (Xx * (1 / Xz), Xy * (1 / Xz)); the rim test is done on the floats
 *       (8 <= x1.x < W - 7: the same set as 7 < (int)x1.x < W - 7 for every finite value);
 *   X of a slot: ((nx - cx_j) * z * (1 / fx_j), (ny - cy_j) * z * (1 / fy_j), z) in double, rounded to float;
 *   transformed depth: with T = R_ref R_j^T (cv::Matx product, k ascending) and t = R_ref (C_j - C_ref) (row times the difference
 *       vector, left to right), both in double on the host, and Xc the double point above:
 *       z' = (float)(((T[6] * Xc0 + T[7] * Xc1) + T[8] * Xc2) + t[2])  -- no float3 in between.
 * Built with oracle/Makefile's CFLAGS (-ffp-contract=off) into tests/libhcmvs_oracle_spread.so.
 */
#include "../oracle/hcmvs_oracle.c"

/* the maps view j offers as a source view: width x height floats (normal: 3 per pixel); depth == NULL: none */
typedef struct {
	int width, height;
	const float* depth;
	const float* normal;
	const float* conf;
} hcor_spread_map;

/* counters, summed over every call since the last reset */
static unsigned long long g_sp_scored, g_sp_accepted, g_sp_dropped, g_sp_outside;
void hcor_spread_stats(uint64_t* scored, uint64_t* accepted, uint64_t* dropped, uint64_t* outside, int reset) {
	if (scored) *scored = __atomic_load_n(&g_sp_scored, __ATOMIC_RELAXED);
	if (accepted) *accepted = __atomic_load_n(&g_sp_accepted, __ATOMIC_RELAXED);
	if (dropped) *dropped = __atomic_load_n(&g_sp_dropped, __ATOMIC_RELAXED);
	if (outside) *outside = __atomic_load_n(&g_sp_outside, __ATOMIC_RELAXED);
	if (reset) {
		__atomic_store_n(&g_sp_scored, 0ull, __ATOMIC_RELAXED); __atomic_store_n(&g_sp_accepted, 0ull, __ATOMIC_RELAXED);
		__atomic_store_n(&g_sp_dropped, 0ull, __ATOMIC_RELAXED); __atomic_store_n(&g_sp_outside, 0ull, __ATOMIC_RELAXED);
	}
}

/* trace of ONE pixel for the known-answer tests (single-threaded runs only): rows of 8 floats
 *   kind 0  pixel:  sweep, returned through the full-random branch (0/1), conf before the block, 0, 0, 0, 0
 *   kind 1  view:   view index (0-based), x1.x, x1.y (ints; -1 when x1 is not finite), candidates, slots, 0, 0
 *   kind 2  slot:   view index, nx, ny, state (0 skipped by conf, 1 dropped by depth, 2 scored), transformed depth, nconf, accepted
 *   kind 3  hint:   sweep, size of the smoothness set the hint sees, 0 ... */
#define SP_TRACE_ROWS 256
static int g_tr_x = -1, g_tr_y = -1, g_tr_n;
static float g_tr[SP_TRACE_ROWS][8];
void hcor_spread_trace_pixel(int x, int y) { g_tr_x = x; g_tr_y = y; g_tr_n = 0; }
int hcor_spread_trace_get(float* out, int cap) {
	const int n = g_tr_n < cap ? g_tr_n : cap;
	memcpy(out, g_tr, sizeof(float) * 8 * (size_t)n);
	return g_tr_n;
}
static void tr_put(int on, float k, float a, float b, float c, float d, float e, float f, float g) {
	if (!on || g_tr_n >= SP_TRACE_ROWS) return;
	float* r = g_tr[g_tr_n++];
	r[0] = k; r[1] = a; r[2] = b; r[3] = c; r[4] = d; r[5] = e; r[6] = f; r[7] = g;
}

typedef struct {
	const hcor_spread_map* sm; /* [V] or NULL */
	int on;
	double T[HCOR_MAX_VIEWS][9], t[HCOR_MAX_VIEWS][3]; /* R_ref R_j^T, R_ref (C_j - C_ref) */
	double jifx[HCOR_MAX_VIEWS], jify[HCOR_MAX_VIEWS];
} spread_ctx;

static int spreads(const est_ctx* c, const spread_ctx* sc, int v) {
	return sc->on && sc->sm && sc->sm[v].depth && sc->sm[v].normal && sc->sm[v].conf && sc->sm[v].width == c->srcs[v].width &&
	       sc->sm[v].height == c->srcs[v].height;
}
static void spread_init(spread_ctx* sc, const est_ctx* c, const hcor_spread_map* sm, int on) {
	memset(sc, 0, sizeof *sc);
	sc->sm = sm; sc->on = on && sm && c->p.it_external >= 1;
	for (int v = 0; v < c->V; ++v) {
		const hcor_view* s = &c->srcs[v];
		mat3_mul_bt(c->ref->R, s->R, sc->T[v]);
		const double dC[3] = {s->C[0] - c->ref->C[0], s->C[1] - c->ref->C[1], s->C[2] - c->ref->C[2]};
		for (int i = 0; i < 3; ++i) sc->t[v][i] = c->ref->R[i * 3] * dC[0] + c->ref->R[i * 3 + 1] * dC[1] + c->ref->R[i * 3 + 2] * dC[2];
		sc->jifx[v] = 1.0 / s->K[0]; sc->jify[v] = 1.0 / s->K[4];
	}
}

/* DepthMap.cpp:1515-1521: where the pixel projects to in view v under its current estimate; 0 when x1 is not finite */
static int spread_x1(const est_ctx* c, const pix_state* ps, int v, float depth, const float* normal, float* x1x, float* x1y) {
	float H[9];
	if (c->p.arith_mode == HCOR_ARITH_DEVICE) {
		device_H(c, ps, v, depth, normal, H);
		const float px = (float)ps->x, py = (float)ps->y;
		const float Xx = fmaf(H[1], py, fmaf(H[0], px, H[2]));
		const float Xy = fmaf(H[4], py, fmaf(H[3], px, H[5]));
		const float Xz = fmaf(H[7], py, fmaf(H[6], px, H[8]));
		const float iz = 1.0f / Xz;
		*x1x = Xx * iz; *x1y = Xy * iz;
	} else {
		/* DepthMap.h:565-574 ComputeHomographyMatrix, Util.inl:255-259 ProjectVertex_3x3_2_3, Types.h:1275 Point2f(Point3f) */
		const double n[3] = {normal[0], normal[1], normal[2]};
		const double inv = 1.0 / ((n[0] * ps->X0[0] + n[1] * ps->X0[1] + n[2] * ps->X0[2]) * (double)depth);
		double M[9], Hd[9];
		for (int i = 0; i < 3; ++i)
			for (int j = 0; j < 3; ++j) M[i * 3 + j] = c->Hl[v][i * 3 + j] + c->Hm[v][i] * (n[j] * inv);
		mat3_mul(M, c->Hr, Hd);
		for (int i = 0; i < 9; ++i) H[i] = (float)Hd[i];
		const float px = (float)ps->x, py = (float)ps->y;
		const float X[3] = {H[0] * px + H[1] * py + H[2], H[3] * px + H[4] * py + H[5], H[6] * px + H[7] * py + H[8]};
		*x1x = X[0] / X[2]; *x1y = X[1] / X[2];
	}
	return isfinite(*x1x) && isfinite(*x1y);
}

/* DepthMap.cpp:1590-1592 */
static float spread_depth(const est_ctx* c, const spread_ctx* sc, int v, int nx, int ny, float nd) {
	const hcor_view* s = &c->srcs[v];
	const double z = nd;
	if (c->p.arith_mode == HCOR_ARITH_DEVICE) {
		const double X0 = ((double)nx - s->K[2]) * z * sc->jifx[v], X1 = ((double)ny - s->K[5]) * z * sc->jify[v];
		const double* T = sc->T[v];
		return (float)(((T[6] * X0 + T[7] * X1) + T[8] * z) + sc->t[v][2]);
	}
	const double Xc[3] = {((double)nx - s->K[2]) * z / s->K[0], ((double)ny - s->K[5]) * z / s->K[4], z}; /* Camera.h:306-312 */
	float Xw[3]; /* Point3f(R.t() * X + C), Camera.h:314-316 */
	for (int i = 0; i < 3; ++i) Xw[i] = (float)(((s->R[i] * Xc[0] + s->R[3 + i] * Xc[1]) + s->R[6 + i] * Xc[2]) + s->C[i]);
	const double d[3] = {(double)Xw[0] - c->ref->C[0], (double)Xw[1] - c->ref->C[1], (double)Xw[2] - c->ref->C[2]}; /* Camera.h:356-358 */
	return (float)((c->ref->R[6] * d[0] + c->ref->R[7] * d[1]) + c->ref->R[8] * d[2]);
}

/* the block itself; conf / depth / normal are the pixel's estimate, updated in place */
static void spread_block(est_ctx* c, const spread_ctx* sc, pix_state* ps, int tr, float* conf, float* depth, float* normal) {
	const hcor_view* ref = c->ref;
	const int W = ref->width, H = ref->height;
	for (int v = 0; v < c->V; ++v) {
		if (!spreads(c, sc, v)) continue;
		const hcor_spread_map* m = &sc->sm[v];
		float x1x, x1y;
		const int fin = spread_x1(c, ps, v, *depth, normal, &x1x, &x1y);
		ps->nClose = 0; /* neighbors, neighborsClose, candidate .Empty() */
		int cx[4], cy[4], nc = 0, ix = -1, iy = -1;
		/* 7 < (int)x1 < size - 7 on the floats: (int) truncates towards zero, so for finite values the two tests pick the same set */
		if (fin && x1x >= (float)(HCOR_HALF_WINDOW + 1) && x1y >= (float)(HCOR_HALF_WINDOW + 1) && x1x < (float)(W - HCOR_HALF_WINDOW) &&
		    x1y < (float)(H - HCOR_HALF_WINDOW)) {
			ix = (int)x1x; iy = (int)x1y;
			cx[0] = ix; cy[0] = iy - 1;
			cx[1] = ix; cy[1] = iy + 1;
			cx[2] = ix - 1; cy[2] = iy;
			cx[3] = ix + 1; cy[3] = iy;
			nc = 4;
		} else if (fin && fabsf(x1x) < 1e9f && fabsf(x1y) < 1e9f) { ix = (int)x1x; iy = (int)x1y; }
		int sx[4], sy[4], sk[4], ns = 0;
		for (int k = 0; k < nc; ++k) {
			if (cx[k] < 0 || cy[k] < 0 || cx[k] >= m->width || cy[k] >= m->height) { /* D10: inside view j's map */
				__atomic_fetch_add(&g_sp_outside, 1ull, __ATOMIC_RELAXED);
				continue;
			}
			const size_t nidx = (size_t)cy[k] * m->width + cx[k];
			const float nd = m->depth[nidx];
			if (!(nd > 0)) continue;
			const int q = ps->nClose++;
			ps->cSlot[q] = k;
			ps->cDepth[q] = nd;
			ps->cNormal[q][0] = m->normal[3 * nidx]; ps->cNormal[q][1] = m->normal[3 * nidx + 1]; ps->cNormal[q][2] = m->normal[3 * nidx + 2];
			const double z = nd;
			const hcor_view* s = &c->srcs[v];
			if (c->p.arith_mode == HCOR_ARITH_DEVICE) {
				ps->cX[q][0] = (float)(((double)cx[k] - s->K[2]) * z * sc->jifx[v]);
				ps->cX[q][1] = (float)(((double)cy[k] - s->K[5]) * z * sc->jify[v]);
			} else {
				ps->cX[q][0] = (float)(((double)cx[k] - s->K[2]) * z / s->K[0]);
				ps->cX[q][1] = (float)(((double)cy[k] - s->K[5]) * z / s->K[4]);
			}
			ps->cX[q][2] = (float)z;
			sx[ns] = cx[k]; sy[ns] = cy[k]; sk[ns] = q; ++ns;
		}
		tr_put(tr, 1, (float)v, (float)ix, (float)iy, (float)nc, (float)ns, 0, 0);
		for (int q = 0; q < ns; ++q) {
			const size_t nidx = (size_t)sy[q] * m->width + sx[q];
			if (m->conf[nidx] >= c->p.ncc_threshold_keep) { tr_put(tr, 2, (float)v, (float)sx[q], (float)sy[q], 0, 0, 0, 0); continue; }
			const int k = sk[q];
			const float nd = spread_depth(c, sc, v, sx[q], sy[q], ps->cDepth[k]);
			if (!(nd > 0)) { /* D10: the reference asserts this in debug builds only */
				__atomic_fetch_add(&g_sp_dropped, 1ull, __ATOMIC_RELAXED);
				tr_put(tr, 2, (float)v, (float)sx[q], (float)sy[q], 1, nd, 0, 0);
				continue;
			}
			ps->cDepth[k] = nd;
			correct_normal(c->mt, ps->viewDir, ps->cNormal[k]);
			init_plane(ps, nd, ps->cNormal[k]);
			const float nconf = score_pixel(c, ps, nd, ps->cNormal[k]);
			__atomic_fetch_add(&g_sp_scored, 1ull, __ATOMIC_RELAXED);
			const int acc = *conf > nconf;
			if (acc) {
				*conf = nconf; *depth = nd;
				normal[0] = ps->cNormal[k][0]; normal[1] = ps->cNormal[k][1]; normal[2] = ps->cNormal[k][2];
				__atomic_fetch_add(&g_sp_accepted, 1ull, __ATOMIC_RELAXED);
			}
			tr_put(tr, 2, (float)v, (float)sx[q], (float)sy[q], 2, nd, nconf, (float)acc);
		}
	}
}

/* DepthMap.cpp:1050-1608 ProcessPixel: the oracle's process_pixel restated, with the spread block in front of the hint */
static void process_pixel_spread(est_ctx* c, const spread_ctx* sc, int x, int y, int iter, float* depthMap, float* normalMap, float* confMap) {
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
	float conf = confMap[idx], depth = depthMap[idx];
	float normal[3] = {normalMap[3 * idx], normalMap[3 * idx + 1], normalMap[3 * idx + 2]};
	init_plane(&ps, depth, normal);
	for (int q = 0; q < nNb; ++q) {
		if (confMap[nby[q] * W + nbx[q]] >= c->p.ncc_threshold_keep) continue;
		const int k = nbc[q];
		ps.cDepth[k] = interpolate_pixel(c, &ps, nbx[q], nby[q], ps.cDepth[k], ps.cNormal[k]);
		correct_normal(c->mt, ps.viewDir, ps.cNormal[k]);
		init_plane(&ps, ps.cDepth[k], ps.cNormal[k]);
		const float nconf = score_pixel(c, &ps, ps.cDepth[k], ps.cNormal[k]);
		if (conf > nconf) {
			conf = nconf; depth = ps.cDepth[k];
			normal[0] = ps.cNormal[k][0]; normal[1] = ps.cNormal[k][1]; normal[2] = ps.cNormal[k][2];
		}
	}
	const uint32_t st = STREAM_SWEEP(c->p.it_external, iter);
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
				const float nconf = score_pixel(c, &ps, nd, nn);
				if (conf > nconf) {
					conf = nconf; depth = nd; normal[0] = nn[0]; normal[1] = nn[1]; normal[2] = nn[2];
					if (conf < c->thConfRand) { again = 1; break; }
				}
			}
			if (again) continue;
			done = 1; /* the `return` of DepthMap.cpp:1464 */
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
			const float nconf = score_pixel(c, &ps, nd, nn);
			if (conf > nconf) {
				conf = nconf; depth = nd; normal[0] = nn[0]; normal[1] = nn[1]; normal[2] = nn[2];
				p[0] = np[0]; p[1] = np[1];
				++idxScaleRange;
				scaleRange = 1.f / (float)(1u << idxScaleRange);
			}
		}
	}
	const int tr = x == g_tr_x && y == g_tr_y;
	/* DepthMap.cpp:1504-1608 */
	if (sc->on) {
		tr_put(tr, 0, (float)iter, (float)done, conf, 0, 0, 0, 0);
		if (!done) spread_block(c, sc, &ps, tr, &conf, &depth, normal);
	}
	if (c->p.hint_depth && c->p.hint_normal && c->p.it_external == c->p.n_external_iters - 1 && iter == c->p.n_estimation_iters - 1 &&
	    c->p.hint_depth[idx] > 0) {
		tr_put(tr, 3, (float)iter, (float)ps.nClose, 0, 0, 0, 0, 0);
		float nn[3] = {c->p.hint_normal[3 * idx], c->p.hint_normal[3 * idx + 1], c->p.hint_normal[3 * idx + 2]};
		const float nd = interpolate_pixel(c, &ps, x, y, c->p.hint_depth[idx], nn);
		correct_normal(c->mt, ps.viewDir, nn);
		init_plane(&ps, nd, nn);
		const float nconf = score_pixel(c, &ps, nd, nn);
		if (conf > nconf - 0.1f) { conf = nconf; depth = nd; normal[0] = nn[0]; normal[1] = nn[1]; normal[2] = nn[2]; }
	}
	confMap[idx] = conf; depthMap[idx] = depth;
	normalMap[3 * idx] = normal[0]; normalMap[3 * idx + 1] = normal[1]; normalMap[3 * idx + 2] = normal[2];
}

/* hcor_pass_sweep with the body above: the same zig-zag and row-pipelined drivers */
static inline int sp_kept(const uint8_t* keep, long i) { return !keep || keep[i]; }
void hcor_spread_pass_sweep(const hcor_view* ref, const hcor_view* srcs, int V, const uint8_t* gra, const hcor_params* p, const hcor_spread_map* sm,
                            int on, const uint8_t* keep, int iter, float dMin, float dMax, float* depth, float* normal, float* conf, uint64_t* evals) {
	const int W = ref->width, H = ref->height;
	const int rev = (iter % 2) != 0;
	if (p->order == HCOR_ORDER_ZIGZAG) {
		est_ctx c;
		ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
		spread_ctx sc;
		spread_init(&sc, &c, sm, on);
		uint16_t* coords = (uint16_t*)malloc(sizeof(uint16_t) * 2 * (size_t)W * H);
		const int stride = 8 * p->n_threads > 64 ? 8 * p->n_threads : 64;
		const int n = hcor_zigzag_coords(W, H, stride, coords);
		for (int i = 0; i < n; ++i) {
			const int k = rev ? n - 1 - i : i;
			if (sp_kept(keep, (long)coords[2 * k + 1] * W + coords[2 * k])) process_pixel_spread(&c, &sc, coords[2 * k], coords[2 * k + 1], iter, depth, normal, conf);
		}
		free(coords);
		if (evals) *evals += c.evals;
		return;
	}
	const int nt = p->n_threads > 0 ? p->n_threads : 1;
	atomic_int* progress = (atomic_int*)calloc((size_t)H, sizeof(atomic_int));
	uint64_t total = 0;
#pragma omp parallel num_threads(nt) reduction(+ : total)
	{
		est_ctx c;
		ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
		spread_ctx sc;
		spread_init(&sc, &c, sm, on);
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
				if (sp_kept(keep, (long)y * W + x)) process_pixel_spread(&c, &sc, x, y, iter, depth, normal, conf);
				atomic_store_explicit(&progress[r], q + 1, memory_order_release);
			}
		}
		total += c.evals;
	}
	free(progress);
	if (evals) *evals += total;
}

/* hcor_estimate with view spread: sm[v] are the maps source view v offers (NULL / depth NULL: none), on = --n-viewspread.
 * The spread maps must not alias depth / normal / conf (a sweep must not read what it writes).  keep: optional keep-mask of the
 * reference view (--ignore-mask-label; 1 = estimated), handled as tests/oracle_mask.c handles it; conf is in/out with one. */
int hcor_spread_estimate(const hcor_view* ref, const hcor_view* srcs, int V, const uint8_t* gra, const hcor_params* p, const hcor_spread_map* sm,
                         int on, const uint8_t* keep, float dMin, float dMax, float* depth, float* normal, float* conf, uint64_t* evals) {
	if (V < 1 || V > HCOR_MAX_VIEWS) return 1;
	if (p->adapthalfwin < 1 || p->adapthalfwin > HCOR_MAX_HALF_WINDOW) return 1;
	const int W = ref->width, H = ref->height;
	if (evals) *evals = 0;
	if (keep) /* DepthData::ApplyIgnoreMask */
		for (long i = 0; i < (long)W * H; ++i)
			if (!keep[i]) { depth[i] = 0; normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0; conf[i] = 0; }
	if (p->median_blur) {
		float* tmp = (float*)malloc(sizeof(float) * (size_t)W * H);
		hcor_median3(depth, W, H, tmp);
		memcpy(depth, tmp, sizeof(float) * (size_t)W * H);
		free(tmp);
	}
	if (!keep) hcor_pass_score(ref, srcs, V, gra, p, dMin, dMax, depth, normal, conf, evals);
	else {
		est_ctx c;
		ctx_init(&c, ref, srcs, V, gra, p, dMin, dMax);
		for (int y = 0; y < H; ++y)
			for (int x = 0; x < W; ++x)
				if (keep[(long)y * W + x]) score_one(&c, x, y, depth, normal, conf);
		if (evals) *evals += c.evals;
	}
	for (int iter = 0; iter < p->n_estimation_iters; ++iter)
		hcor_spread_pass_sweep(ref, srcs, V, gra, p, sm, on, keep, iter, dMin, dMax, depth, normal, conf, evals);
	if (p->it_external == p->n_external_iters - 1) {
		if (!keep) hcor_pass_end(p, W, H, depth, normal, conf);
		else
			for (long i = 0; i < (long)W * H; ++i) {
				if (!keep[i]) continue;
				if (depth[i] <= 0 || conf[i] >= p->ncc_threshold_keep) { conf[i] = 0; normal[3 * i] = normal[3 * i + 1] = normal[3 * i + 2] = 0; depth[i] = 0; }
				else conf[i] = conf[i] >= 1.f ? 0.f : 1.f - conf[i];
			}
	}
	return 0;
}

/* DepthMap.cpp:1590-1592 alone, for the known-answer tests: depth of view j's pixel (nx, ny, nd) seen from ref */
float hcor_spread_transform_depth(const hcor_view* ref, const hcor_view* src, int nx, int ny, float nd, int mode) {
	hcor_params p;
	hcor_default_params(&p);
	p.arith_mode = mode; p.it_external = 1;
	est_ctx c;
	ctx_init(&c, ref, src, 1, NULL, &p, 1.f, 2.f);
	spread_ctx sc;
	spread_init(&sc, &c, NULL, 0);
	return spread_depth(&c, &sc, 0, nx, ny, nd);
}

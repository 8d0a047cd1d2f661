/*
 * oracle/hcmvs_spread.inc -- TEST INFRASTRUCTURE: view spread (DensifyPointCloud --n-viewspread, DepthMap.cpp:1504-1608), the block
 * process_pixel runs between the refinement trials and the `restore` hint when hcor_params carries spread maps.  Not a translation
 * unit of its own: hcmvs_oracle.c includes it ahead of process_pixel, for the oracle's static per-pixel functions.
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
 */

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

/* est_ctx holds the set-up (ctx_init): spread, spT = R_ref R_j^T, spt = R_ref (C_j - C_ref), jifx / jify = 1 / f of view j */
static int spreads(const est_ctx* c, int v) {
	const hcor_spread_map* sm = c->p.spread_maps;
	return c->spread && sm[v].depth && sm[v].normal && sm[v].conf && sm[v].width == c->srcs[v].width && sm[v].height == c->srcs[v].height;
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
static float spread_depth(const est_ctx* c, int v, int nx, int ny, float nd) {
	const hcor_view* s = &c->srcs[v];
	const double z = nd;
	if (c->p.arith_mode == HCOR_ARITH_DEVICE) {
		const double X0 = ((double)nx - s->K[2]) * z * c->jifx[v], X1 = ((double)ny - s->K[5]) * z * c->jify[v];
		const double* T = c->spT[v];
		return (float)(((T[6] * X0 + T[7] * X1) + T[8] * z) + c->spt[v][2]);
	}
	const double Xc[3] = {((double)nx - s->K[2]) * z / s->K[0], ((double)ny - s->K[5]) * z / s->K[4], z}; /* Camera.h:306-312 */
	float Xw[3]; /* Point3f(R.t() * X + C), Camera.h:314-316 */
	for (int i = 0; i < 3; ++i) Xw[i] = (float)(((s->R[i] * Xc[0] + s->R[3 + i] * Xc[1]) + s->R[6 + i] * Xc[2]) + s->C[i]);
	const double d[3] = {(double)Xw[0] - c->ref->C[0], (double)Xw[1] - c->ref->C[1], (double)Xw[2] - c->ref->C[2]}; /* Camera.h:356-358 */
	return (float)((c->ref->R[6] * d[0] + c->ref->R[7] * d[1]) + c->ref->R[8] * d[2]);
}

/* the block itself; conf / depth / normal are the pixel's estimate, updated in place */
static void spread_block(est_ctx* c, pix_state* ps, int tr, float* conf, float* depth, float* normal) {
	const hcor_view* ref = c->ref;
	const int W = ref->width, H = ref->height;
	for (int v = 0; v < c->V; ++v) {
		if (!spreads(c, v)) continue;
		const hcor_spread_map* m = &c->p.spread_maps[v];
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
				ps->cX[q][0] = (float)(((double)cx[k] - s->K[2]) * z * c->jifx[v]);
				ps->cX[q][1] = (float)(((double)cy[k] - s->K[5]) * z * c->jify[v]);
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
			const float nd = spread_depth(c, v, sx[q], sy[q], ps->cDepth[k]);
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

/* DepthMap.cpp:1590-1592 alone, for the known-answer tests: depth of view j's pixel (nx, ny, nd) seen from ref */
float hcor_spread_transform_depth(const hcor_view* ref, const hcor_view* src, int nx, int ny, float nd, int mode) {
	hcor_params p;
	hcor_default_params(&p);
	p.arith_mode = mode; p.it_external = 1;
	est_ctx c;
	ctx_init(&c, ref, src, 1, NULL, &p, 1.f, 2.f);
	return spread_depth(&c, 0, nx, ny, nd);
}

/*
 * hc-mvs_amd/csrc/handoff_device.h -- the per-pixel arithmetic of the hand-off between two levels of the coarse-to-fine schedule, shared
 * by the host form (hcmvs_handoff_maps, a plain loop) and the device form (handoff_kernels.hip): one destination pixel of one image,
 * depth and normal together.  Usable from plain C++ (no HIP) and from device code.
 *
 *   init mode  (--n-initTriangulate 0, SceneDensify.cpp:527-553): the previous level's maps become the initial maps -- as they are when
 *              the sizes agree, else cv::resize INTER_CUBIC (Keys kernel, A = -0.75, pixel centres aligned, replicated border); a depth
 *              that is not > 0 becomes 0, the normal of a kept depth is brought to length 1.
 *   hint mode  (the `restore` variant, restore/libs/MVS/SceneDensify.cpp:508-532): cv::resize INTER_AREA enlarging (the bilinear kernel
 *              with "area mode" coefficients, as hcmvs_resize_area_up states it); a pixel whose depth is not > 0 or whose normal has no
 *              length offers no hint (depth 0), the others get the normal at length 1.
 *
 * Every multiply and add is its own IEEE f32 operation (the callers are built with -ffp-contract=off); float division and sqrtf are
 * correctly rounded on both sides.  The destination coordinate is mapped in double, as cv::resize does.
 */
#ifndef HCMVS_HANDOFF_DEVICE_H
#define HCMVS_HANDOFF_DEVICE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HCMVS_HANDOFF_FN __host__ __device__ __forceinline__
#else
#define HCMVS_HANDOFF_FN inline
#endif

namespace hcmvs {

enum { kHandoffInit = 0, kHandoffHint = 1 };

// sizes and the four ratios of one item, taken once on the host: rx = (double)sw / dw, ix = (double)dw / sw, ry / iy alike
struct HandoffGeom {
	int32_t sw, sh, dw, dh;
	double rx, ry, ix, iy;
};
inline HandoffGeom handoff_geom(int sw, int sh, int dw, int dh) {
	HandoffGeom g;
	g.sw = sw; g.sh = sh; g.dw = dw; g.dh = dh;
	g.rx = (double)sw / dw; g.ry = (double)sh / dh;
	g.ix = (double)dw / sw; g.iy = (double)dh / sh;
	return g;
}

// what one destination pixel gets, and what it adds to the item's range and counters
struct HandoffPixel {
	float d, n[3]; // the values stored
	float raw;     // the resampled depth before the clean-up (hint mode: what widens the range)
	bool valid;    // d > 0
	bool clamped;  // the resampled depth was not > 0 although a source sample that entered it was
	bool rescaled; // the normal was divided by its length
};

HCMVS_HANDOFF_FN void handoff_cubic_weights(float t, float* w) {
	const float A = -0.75f;
	w[0] = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A;
	w[1] = ((A + 2) * t - (A + 3)) * t * t + 1;
	w[2] = ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1;
	w[3] = 1.f - w[0] - w[1] - w[2];
}
// destination coordinate x of an axis with ratio = source size / destination size: the four source indices (clamped) and their weights
HCMVS_HANDOFF_FN void handoff_cubic_axis(int x, double ratio, int ssize, int* idx, float* w) {
	const float f = (float)((x + 0.5) * ratio - 0.5);
	const int i = (int)floorf(f);
	handoff_cubic_weights(f - i, w);
	for (int k = 0; k < 4; ++k) {
		const int s = i - 1 + k;
		idx[k] = s < 0 ? 0 : (s > ssize - 1 ? ssize - 1 : s);
	}
}
// channel c of a map with ch interleaved channels: rows outer, columns inner, both sums from 0
HCMVS_HANDOFF_FN float handoff_cubic_sample(const float* src, int sw, int ch, int c, const int* xi, const int* yi, const float* wx, const float* wy) {
	float acc = 0.f;
	for (int j = 0; j < 4; ++j) {
		const float* S = src + (size_t)yi[j] * sw * ch;
		float row = 0.f;
		for (int i = 0; i < 4; ++i) row += wx[i] * S[(size_t)xi[i] * ch + c];
		acc += wy[j] * row;
	}
	return acc;
}

// INTER_AREA enlarging, one axis: the left / upper source index and the weight of its right / lower partner
HCMVS_HANDOFF_FN void handoff_area_axis(int d, double scale, double inv, int ssize, bool columns, int* s, float* f) {
	int si = (int)floor(d * scale);
	float ff = (float)((d + 1) - (si + 1) * inv);
	ff = ff <= 0 ? 0.f : ff - floorf(ff);
	if (columns && si >= ssize - 1) { ff = 0.f; si = ssize - 1; } // no right partner: the sample alone
	*s = si; *f = ff;
}
struct HandoffAreaTaps {
	int sx, r0, r1; // left column; upper and lower row, both clamped
	float a0, a1, b0, b1;
	bool alone;     // sx is the last column
};
HCMVS_HANDOFF_FN HandoffAreaTaps handoff_area_taps(const HandoffGeom& g, int x, int y) {
	HandoffAreaTaps t;
	int sy;
	handoff_area_axis(x, g.rx, g.ix, g.sw, true, &t.sx, &t.a1);
	handoff_area_axis(y, g.ry, g.iy, g.sh, false, &sy, &t.b1);
	t.a0 = 1.f - t.a1; t.b0 = 1.f - t.b1;
	t.r0 = sy < 0 ? 0 : (sy > g.sh - 1 ? g.sh - 1 : sy);
	t.r1 = sy + 1 < 0 ? 0 : (sy + 1 > g.sh - 1 ? g.sh - 1 : sy + 1);
	t.alone = t.sx + 1 >= g.sw;
	return t;
}
HCMVS_HANDOFF_FN float handoff_area_sample(const float* src, int sw, int ch, int c, const HandoffAreaTaps& t) {
	const float* S0 = src + ((size_t)t.r0 * sw + t.sx) * ch + c;
	const float* S1 = src + ((size_t)t.r1 * sw + t.sx) * ch + c;
	const float h0 = t.alone ? S0[0] : S0[0] * t.a0 + S0[ch] * t.a1;
	const float h1 = t.alone ? S1[0] : S1[0] * t.a0 + S1[ch] * t.a1;
	return h0 * t.b0 + h1 * t.b1;
}
// the enlarged depth alone (what widens the range in hint mode)
HCMVS_HANDOFF_FN float handoff_hint_raw_depth(const HandoffGeom& g, const float* sd, int x, int y) {
	return handoff_area_sample(sd, g.sw, 1, 0, handoff_area_taps(g, x, y));
}

// init mode, destination pixel (x, y): sd is the source depth (sw * sh), sn the source normal (sw * sh * 3)
HCMVS_HANDOFF_FN void handoff_init_pixel(const HandoffGeom& g, const float* sd, const float* sn, int x, int y, HandoffPixel& o) {
	bool tap = false;
	if (g.sw == g.dw && g.sh == g.dh) {
		const size_t at = (size_t)y * g.sw + x;
		o.raw = sd[at];
		o.n[0] = sn[3 * at]; o.n[1] = sn[3 * at + 1]; o.n[2] = sn[3 * at + 2];
		tap = o.raw > 0.f;
	} else {
		int xi[4], yi[4];
		float wx[4], wy[4];
		handoff_cubic_axis(x, g.rx, g.sw, xi, wx);
		handoff_cubic_axis(y, g.ry, g.sh, yi, wy);
		o.raw = handoff_cubic_sample(sd, g.sw, 1, 0, xi, yi, wx, wy);
		for (int c = 0; c < 3; ++c) o.n[c] = handoff_cubic_sample(sn, g.sw, 3, c, xi, yi, wx, wy);
		for (int j = 0; j < 4; ++j)
			for (int i = 0; i < 4; ++i) tap = tap || sd[(size_t)yi[j] * g.sw + xi[i]] > 0.f;
	}
	o.valid = o.raw > 0.f;
	o.d = o.valid ? o.raw : 0.f; // NaN included
	o.clamped = !o.valid && tap;
	o.rescaled = false;
	if (o.d == 0.f) return;
	const float len = sqrtf(o.n[0] * o.n[0] + o.n[1] * o.n[1] + o.n[2] * o.n[2]);
	if (len > 0.f) { o.n[0] /= len; o.n[1] /= len; o.n[2] /= len; o.rescaled = true; }
}

// hint mode, destination pixel (x, y)
HCMVS_HANDOFF_FN void handoff_hint_pixel(const HandoffGeom& g, const float* sd, const float* sn, int x, int y, HandoffPixel& o) {
	const HandoffAreaTaps t = handoff_area_taps(g, x, y);
	o.raw = handoff_area_sample(sd, g.sw, 1, 0, t);
	for (int c = 0; c < 3; ++c) o.n[c] = handoff_area_sample(sn, g.sw, 3, c, t);
	const float* S0 = sd + (size_t)t.r0 * g.sw + t.sx;
	const float* S1 = sd + (size_t)t.r1 * g.sw + t.sx;
	const bool tap = S0[0] > 0.f || S1[0] > 0.f || (!t.alone && (S0[1] > 0.f || S1[1] > 0.f));
	const float len = sqrtf(o.n[0] * o.n[0] + o.n[1] * o.n[1] + o.n[2] * o.n[2]);
	o.clamped = !(o.raw > 0.f) && tap;
	o.valid = o.raw > 0.f && len > 0.f;
	o.rescaled = o.valid;
	o.d = o.valid ? o.raw : 0.f;
	if (o.valid) { o.n[0] /= len; o.n[1] /= len; o.n[2] /= len; } // the mix of two unit normals is shorter than 1
}

// ---- the range of hint mode -------------------------------------------------------------------------------------------------------
// The host form folds the enlarged depths hd in raster order into the range it was given:
//     lo = lo > hd ? hd : lo;      hi = hi > hd ? hi : hd;
// A NaN never enters lo (lo > NaN is false) but it REPLACES hi (hi > NaN is false), and whatever follows replaces it again (NaN > hd
// is false): hi ends as the fold over the values behind the last NaN, started from the first of them -- or as NaN when the last pixel
// is one.  Without a NaN it is the plain maximum of the given hi and every hd.  Ordering floats as unsigned integers (sign bit flipped
// for positives, all bits for negatives) reproduces both comparisons for everything that is not NaN, so the device reduces
//     min and max of the ordered keys of the non-NaN values, and the largest raster index + 1 of a NaN (0 = none)
// and, only when there was a NaN, folds the pixels behind the last one again.  A range given as NaN is refused (handoff_plan.h).
HCMVS_HANDOFF_FN uint32_t handoff_order_key(float v) {
	union { float f; uint32_t u; } b;
	b.f = v;
	return (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
}
HCMVS_HANDOFF_FN float handoff_key_value(uint32_t k) {
	union { float f; uint32_t u; } b;
	b.u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
	return b.f;
}
constexpr uint32_t kHandoffKeyMinIdentity = 0xFFFFFFFFu, kHandoffKeyMaxIdentity = 0u; // neither is the key of a number

// what the pixels of an item (or of one workgroup of it) reduce to on the device; the host form fills the counters only
struct HandoffResult {
	uint32_t lo, hi;      // init mode: bits of the smallest / largest cleaned depth (>= 0: they order like the floats; identities FLT_MAX, 0);
	                      // hint mode: ordered keys (identities above)
	uint32_t lastNaN;     // hint mode: raster index + 1 of the last enlarged depth that is NaN, 0 = none
	uint32_t tailHi;      // hint mode, lastNaN != 0: bits of the fold over the pixels behind it
	unsigned long long valid, clamped, rescaled;
};
// the item's range and status from its result slot.  Init mode: d_min / d_max are written unless the map holds no valid depth.  Hint
// mode: they are read and widened.  A d_min that would be <= 0 (or -0) comes back as +0, a d_max of -0 as +0.
inline bool handoff_finish(int mode, const HandoffResult& r, float* d_min, float* d_max) {
	union { float f; uint32_t u; } b;
	if (mode == kHandoffInit) {
		b.u = r.hi; const float hi = b.f;
		b.u = r.lo; const float lo = b.f;
		if (!(hi > 0.f)) return false;
		*d_min = lo * 0.9f; *d_max = hi * 1.1f;
		return true;
	}
	float lo = *d_min, hi = *d_max;
	if (r.lo != kHandoffKeyMinIdentity) { const float v = handoff_key_value(r.lo); lo = lo > v ? v : lo; }
	if (r.lastNaN) { b.u = r.tailHi; hi = b.f; }
	else if (r.hi != kHandoffKeyMaxIdentity) { const float v = handoff_key_value(r.hi); hi = hi > v ? hi : v; }
	*d_min = lo > 0.f ? lo : 0.f;
	*d_max = hi == 0.f ? 0.f : hi;
	return true;
}

} // namespace hcmvs
#endif

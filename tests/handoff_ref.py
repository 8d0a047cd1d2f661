"""The hand-off between two pyramid levels (include/hcmvs_hip.h, hcmvs_handoff_maps) restated in numpy float32 from the rule, not from
the library's code: every multiply and add is one float32 operation, the destination coordinate is mapped in float64.  Also the maps the
tests hand over, and the ctypes face of tests/handoff_shim.cpp.  Shared by test_handoff_host.py and test_gpu_handoff.py."""
import ctypes as C
import os
import subprocess

import numpy as np

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hc-mvs_amd", "csrc")
SHIM_SRC = os.path.join(HERE, "handoff_shim.cpp")
SHIM_DEPS = [SHIM_SRC, os.path.join(CSRC, "handoff_plan.h"), os.path.join(CSRC, "handoff_device.h"), os.path.join(CSRC, "carve.h"),
             os.path.join(ROOT, "hc-mvs_amd", "host", "scene_io.h")]
SHIM_PATH = os.path.join(HERE, "libhandoff_shim.so")

# source -> destination, (w, h) each: the shapes the tests cover
INIT_SHAPES = [((37, 29), (74, 58)),      # exact x 2
               ((37, 29), (61, 47)),      # independent ratios
               ((37, 29), (37, 29)),      # the copy path
               ((61, 47), (37, 29)),      # shrinking
               ((1, 1), (5, 3)),          # every tap clamped
               ((3, 2), (200, 3))]
HINT_SHAPES = [((37, 29), (74, 58)),
               ((37, 29), (61, 47)),
               ((37, 29), (37, 40)),      # dw == sw only
               ((1, 1), (5, 3)),
               ((16, 16), (16, 16))]      # equal size
CONTENTS = ["mixed", "clean", "nan_last", "empty"]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def cubic_axis(ssize, dsize):
    """per destination coordinate: four clamped source indices (4, dsize) and their weights (4, dsize) float32; Keys kernel A = -0.75"""
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * (float(ssize) / float(dsize)) - 0.5).astype(F)
    i = np.floor(f)
    t = f - i                                           # float32 - float32
    i = i.astype(np.int64)
    A = F(-0.75)
    t1 = t + F(1)
    w0 = ((A * t1 - F(5) * A) * t1 + F(8) * A) * t1 - F(4) * A
    w1 = ((A + F(2)) * t - (A + F(3))) * t * t + F(1)
    u = F(1) - t
    w2 = ((A + F(2)) * u - (A + F(3))) * u * u + F(1)
    w3 = F(1) - w0 - w1 - w2
    idx = np.stack([np.clip(i - 1 + k, 0, ssize - 1) for k in range(4)])
    w = np.stack([w0, w1, w2, w3])
    assert w.dtype == F
    return idx, w


def resize_cubic(src, dw, dh):
    """cv::resize INTER_CUBIC of (h, w) or (h, w, ch) float32: rows outer, columns inner, both sums from 0, replicated border.  Also
    returns whether any of the 16 samples of a pixel is > 0 (first channel)"""
    s = np.ascontiguousarray(src, F)
    s3 = s[:, :, None] if s.ndim == 2 else s
    sh, sw = s3.shape[:2]
    xi, wx = cubic_axis(sw, dw)
    yi, wy = cubic_axis(sh, dh)
    out = np.empty((dh, dw, s3.shape[2]), F)
    tap = np.zeros((dh, dw), bool)
    with np.errstate(all="ignore"):
        for c in range(s3.shape[2]):
            acc = np.zeros((dh, dw), F)
            for j in range(4):
                rows = s3[yi[j], :, c]                  # (dh, sw)
                row = np.zeros((dh, dw), F)
                for i in range(4):
                    row = row + wx[i][None, :] * rows[:, xi[i]]
                    if c == 0:
                        tap |= rows[:, xi[i]] > 0
                acc = acc + wy[j][:, None] * row
            assert acc.dtype == F
            out[:, :, c] = acc
    return (out[:, :, 0] if s.ndim == 2 else out), tap


def area_axis(ssize, dsize, columns):
    """INTER_AREA enlarging: per destination coordinate the left / upper source index and the weight of its partner"""
    d = np.arange(dsize, dtype=np.float64)
    scale, inv = float(ssize) / float(dsize), float(dsize) / float(ssize)
    s = np.floor(d * scale)
    f = ((d + 1) - (s + 1) * inv).astype(F)
    f = np.where(f <= 0, F(0), f - np.floor(f)).astype(F)
    s = s.astype(np.int64)
    if columns:
        last = s >= ssize - 1
        f = np.where(last, F(0), f).astype(F)
        s = np.where(last, ssize - 1, s)
    return s, f


def area_up(src, dw, dh):
    """cv::resize INTER_AREA enlarging of (h, w) or (h, w, ch).  Also returns whether any sample that entered a pixel is > 0 (first channel)"""
    s = np.ascontiguousarray(src, F)
    s3 = s[:, :, None] if s.ndim == 2 else s
    sh, sw = s3.shape[:2]
    assert dw >= sw and dh >= sh
    sx, a1 = area_axis(sw, dw, True)
    sy, b1 = area_axis(sh, dh, False)
    a0, b0 = F(1) - a1, F(1) - b1
    r0, r1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    alone = sx + 1 >= sw
    sx1 = np.minimum(sx + 1, sw - 1)
    out = np.empty((dh, dw, s3.shape[2]), F)
    with np.errstate(all="ignore"):
        for c in range(s3.shape[2]):
            ch = s3[:, :, c]
            h = []
            for r in (r0, r1):
                left, right = ch[r][:, sx], ch[r][:, sx1]
                h.append(np.where(alone[None, :], left, left * a0[None, :] + right * a1[None, :]))
            res = h[0] * b0[:, None] + h[1] * b1[:, None]
            assert res.dtype == F
            out[:, :, c] = res
    d = s3[:, :, 0]
    tap = (d[r0][:, sx] > 0) | (d[r1][:, sx] > 0) | (~alone[None, :] & ((d[r0][:, sx1] > 0) | (d[r1][:, sx1] > 0)))
    return (out[:, :, 0] if s.ndim == 2 else out), tap


def _length(n):
    with np.errstate(all="ignore"):
        return np.sqrt(n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2])


def handoff_init(depth, normal, dw, dh):
    """init mode.  dict(depth, normal, d_min, d_max (None when empty), status, n_valid, n_clamped, n_rescaled, raw, n_negative)"""
    d = np.ascontiguousarray(depth, F); n = np.ascontiguousarray(normal, F)
    sh, sw = d.shape
    if (sw, sh) == (dw, dh):
        raw, nn, tap = d.copy(), n.copy(), d > 0
    else:
        raw, tap = resize_cubic(d, dw, dh)
        nn, _ = resize_cubic(n, dw, dh)
    valid = raw > 0
    out = np.where(valid, raw, F(0)).astype(F)
    ln = _length(nn)
    scale = (out != 0) & (ln > 0)
    with np.errstate(all="ignore"):
        nn = np.where(scale[..., None], nn / ln[..., None], nn).astype(F)
    lo, hi = out.min(), out.max()
    ok = bool(hi > 0)
    return dict(depth=out, normal=nn, d_min=F(lo) * F(0.9) if ok else None, d_max=F(hi) * F(1.1) if ok else None, status=0 if ok else 1,
                n_valid=int(valid.sum()), n_clamped=int((~valid & tap).sum()), n_rescaled=int(scale.sum()), raw=raw,
                n_negative=int((raw < 0).sum()))


def handoff_hint(depth, normal, dw, dh, d_min, d_max):
    """hint mode: the range (d_min, d_max) is widened by every enlarged depth before the clean-up, in raster order"""
    raw, tap = area_up(depth, dw, dh)
    nn, _ = area_up(normal, dw, dh)
    lo, hi = F(d_min), F(d_max)
    for hd in raw.reshape(-1):                          # the comparisons as they stand: a NaN replaces hi and is replaced in turn
        lo = hd if lo > hd else lo
        hi = hi if hi > hd else hd
    ln = _length(nn)
    valid = (raw > 0) & (ln > 0)
    out = np.where(valid, raw, F(0)).astype(F)
    with np.errstate(all="ignore"):
        nn = np.where(valid[..., None], nn / ln[..., None], nn).astype(F)
    return dict(depth=out, normal=nn, d_min=lo if lo > 0 else F(0), d_max=F(0) if hi == 0 else hi, status=0, n_valid=int(valid.sum()),
                n_clamped=int((~(raw > 0) & tap).sum()), n_rescaled=int(valid.sum()), raw=raw, n_negative=int((raw < 0).sum()))


def handoff(mode, depth, normal, dw, dh, d_min=0.0, d_max=0.0):
    return handoff_init(depth, normal, dw, dh) if mode == "init" else handoff_hint(depth, normal, dw, dh, d_min, d_max)


def same_bits(a, b):
    """bit for bit, a NaN equal to any NaN (its sign and payload are the processor's business)"""
    a = np.ascontiguousarray(a, F); b = np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the maps handed over ---------------------------------------------------------------------------------------------------------

STEP_AT = (12, 9)       # (x, y) of the depth 1 of the 1 -> 9 step in maps of at least 24 x 16


def make_maps(w, h, content, seed=0, hint=False):
    """(depth (h, w), normal (h, w, 3)) of the previous level.  `mixed`: depths in 1..9 with 10 % holes, normals of length 0.5..1.5,
    and -- where the map is large enough -- a 1 -> 9 step beside a hole, a NaN depth, a NaN normal and a zero normal under valid depths
    (hint: also a negative depth).  `clean`: holes only.  `nan_last`: the last depth is NaN.  `empty`: no depth at all"""
    rng = np.random.RandomState(1000 * w + 10 * h + seed)
    d = rng.uniform(1.0, 9.0, (h, w)).astype(F)
    n = rng.normal(size=(h, w, 3)).astype(F)
    n /= np.linalg.norm(n, axis=-1, keepdims=True).astype(F)
    n = (n * rng.uniform(0.5, 1.5, (h, w, 1))).astype(F)
    if content == "empty":
        return np.zeros((h, w), F), n
    d[rng.uniform(size=(h, w)) < 0.1] = 0
    if content == "nan_last":
        d[-1, -1] = np.nan
        return d, n
    if content == "mixed" and w >= 24 and h >= 16:
        x, y = STEP_AT
        d[y - 3:y + 4, x - 2:x] = 1.0; d[y - 3:y + 4, x] = 1.0; d[y - 3:y + 4, x + 1] = 9.0; d[y - 3:y + 4, x + 2:x + 6] = 0.0
        d[3, 20] = np.nan
        d[5, 3] = 4.0; n[5, 3] = np.nan
        d[6, 21] = 5.0; n[6, 21, 1] = np.nan
        d[13, 20] = 6.0; n[13, 20] = 0.0
        if hint:
            d[14, 4] = -3.0
    return d, n


# ---- the shim ---------------------------------------------------------------------------------------------------------------------

ARGS = np.dtype([("src_depth", "<u8"), ("src_normal", "<u8"), ("dst_depth", "<u8"), ("dst_normal", "<u8"), ("sw", "<i4"), ("sh", "<i4"),
                 ("dw", "<i4"), ("dh", "<i4"), ("d_min", "<f4"), ("d_max", "<f4")])
_shim = None


def shim():
    global _shim
    if _shim is None:
        if not os.path.exists(SHIM_PATH) or any(os.path.getmtime(d) > os.path.getmtime(SHIM_PATH) for d in SHIM_DEPS):
            # -ffp-contract=off as the library
            subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", SHIM_PATH, SHIM_SRC])
        L = C.CDLL(SHIM_PATH)
        vp = C.c_void_p
        L.hs_layout.argtypes = [vp]; L.hs_layout.restype = None
        L.hs_check.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_int]
        L.hs_first.argtypes = [vp, C.c_int, vp]; L.hs_first.restype = None
        L.hs_geom.argtypes = [C.c_int] * 4 + [vp]; L.hs_geom.restype = None
        L.hs_driver_hand_over.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp]
        lay = np.zeros(6, np.int32)
        L.hs_layout(lay.ctypes.data)
        assert lay[0] == ARGS.itemsize
        L.layout = dict(block=int(lay[1]), chunk=int(lay[2]), max_items=int(lay[3]))
        _shim = L
    return _shim


def plan_args(items):
    """items: dicts(src_depth, src_normal, dst_depth, dst_normal [addresses as integers], src_w, src_h, dst_w, dst_h[, d_min, d_max])"""
    a = np.zeros(max(len(items), 1), ARGS)
    for r, it in zip(a, items):
        r["src_depth"], r["src_normal"], r["dst_depth"], r["dst_normal"] = it["src_depth"], it["src_normal"], it["dst_depth"], it["dst_normal"]
        r["sw"], r["sh"], r["dw"], r["dh"] = it["src_w"], it["src_h"], it["dst_w"], it["dst_h"]
        r["d_min"], r["d_max"] = it.get("d_min", 0.0), it.get("d_max", 0.0)
    return a


def plan_check(items, mode, n=None):
    """(refused, reason) of handoff_check"""
    a = plan_args(items or [])
    why = C.create_string_buffer(200)
    rc = shim().hs_check(a.ctypes.data if items is not None else None, len(items) if n is None else n, mode, why, 200)
    return bool(rc), why.value.decode()


def plan_first(items):
    a = plan_args(items)
    first = np.zeros(len(items) + 1, np.int32)
    shim().hs_first(a.ctypes.data, len(items), first.ctypes.data)
    return first


def driver_hand_over(depth, normal, dw, dh):
    """the stand-alone driver's own hand-off on the host: (status 0 / 3, depth, normal, d_min, d_max)"""
    d = np.ascontiguousarray(depth, F); n = np.ascontiguousarray(normal, F)
    od = np.empty((dh, dw), F); on = np.empty((dh, dw, 3), F); rng = np.full(2, -1.0, F)
    rc = shim().hs_driver_hand_over(d.ctypes.data, n.ctypes.data, d.shape[1], d.shape[0], od.ctypes.data, on.ctypes.data, dw, dh, rng.ctypes.data)
    return rc, od, on, rng[0], rng[1]


# ---- what the hand-off refuses --------------------------------------------------------------------------------------------------------

def good_item(sw=8, sh=6, dw=16, dh=12):
    bufs = [np.zeros((sh, sw), F), np.zeros((sh, sw, 3), F), np.zeros((dh, dw), F), np.zeros((dh, dw, 3), F)]
    it = dict(src_depth=bufs[0].ctypes.data, src_normal=bufs[1].ctypes.data, dst_depth=bufs[2].ctypes.data, dst_normal=bufs[3].ctypes.data,
              src_w=sw, src_h=sh, dst_w=dw, dst_h=dh, d_min=1.0, d_max=2.0)
    return it, bufs


def refusals():
    """(name, items, mode, n or None): everything the hand-off refuses before it reads or writes"""
    out = []
    keep = []

    def item(**kw):
        it, bufs = good_item()
        keep.append(bufs)
        it.update(kw)
        return it

    for k in ("src_depth", "src_normal", "dst_depth", "dst_normal"):
        out.append(("null " + k, [item(), item(**{k: 0})], 0, None))
    for k in ("src_w", "src_h", "dst_w", "dst_h"):
        out.append((k + " = 0", [item(**{k: 0})], 0, None))
        out.append((k + " < 0", [item(**{k: -4})], 1, None))
    out.append(("2^29 source pixels", [item(src_w=1 << 15, src_h=1 << 14)], 0, None))
    out.append(("2^29 destination pixels", [item(dst_w=1 << 15, dst_h=1 << 14)], 0, None))
    out.append(("hint narrower", [item(dst_w=7)], 1, None))
    out.append(("hint lower", [item(dst_h=5)], 1, None))
    out.append(("hint NaN range", [item(d_max=float("nan"))], 1, None))
    a = item()
    out.append(("in place depth", [dict(a, dst_depth=a["src_depth"], dst_w=8, dst_h=6)], 0, None))
    out.append(("in place normal", [dict(a, dst_normal=a["src_normal"] + 12, dst_w=8, dst_h=6)], 0, None))
    out.append(("destination depth inside its own normal", [dict(a, dst_depth=a["dst_normal"] + 16 * 12 * 12 - 4)], 0, None))
    b, c = item(), item()
    out.append(("destination over another item's source", [b, dict(c, dst_depth=b["src_depth"] + 4 * 8 * 6 - 4)], 0, None))
    out.append(("two items share a destination", [b, dict(c, dst_normal=b["dst_normal"])], 1, None))
    out.append(("unknown mode", [item()], 2, None))
    out.append(("negative mode", [item()], -1, None))
    out.append(("no items", [item()], 0, 0))
    out.append(("too many items", [item()], 0, 65))
    out.append(("null items", None, 0, 1))
    return out, keep

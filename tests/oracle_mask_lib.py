"""ctypes binding of the masked estimate of the CPU oracle (tests/oracle_mask.c -> tests/libhcmvs_oracle_mask.so), plus numpy
restatements of what --ignore-mask-label does before the estimate: the label list (Util::strSplit + atoi) and cv::resize
INTER_NEAREST of the label image (OpenCV's resizeNN).  Test infrastructure only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_mask.c")
LIB_PATH = os.path.join(HERE, "libhcmvs_oracle_mask.so")


def oracle_cflags():
    """oracle/Makefile's CFLAGS, exactly (-ffp-contract=off -mavx2 -mfma keep the device-association mode bit-reproducible)"""
    with open(os.path.join(O.ORACLE_DIR, "Makefile")) as f:
        for line in f:
            m = re.match(r"\s*CFLAGS\s*=\s*(.*)$", line)
            if m:
                return m.group(1).split()
    raise RuntimeError("oracle/Makefile has no CFLAGS line")


def build(force=False):
    deps = [SRC] + [os.path.join(O.ORACLE_DIR, f) for f in os.listdir(O.ORACLE_DIR) if f.endswith((".c", ".h"))]
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in deps):
        cc = os.environ.get("CC", "gcc")
        subprocess.check_call([cc] + oracle_cflags() + ["-shared", "-o", LIB_PATH, SRC, "-lm"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        fp, u8p, vp = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(O.View)
        L.hcor_mask_estimate.argtypes = [vp, vp, C.c_int, u8p, C.POINTER(O.Params), u8p, C.c_float, C.c_float, fp, fp, fp,
                                         C.POINTER(C.c_uint64)]
        L.hcor_mask_estimate.restype = C.c_int
        _lib = L
    return _lib


def estimate(views, params, d_min, d_max, depth, normal, keep=None, gra=None):
    """oracle_lib.estimate with a keep-mask (h, w) u8 (1 = estimated, 0 = ignored; None = no mask).  Returns depth, normal, conf, evals."""
    ref = O.make_view(views[0]); srcs = O.make_view_array(views[1:])
    h, w = views[0]["gray"].shape
    if gra is None:
        gra = O.gradient_map(views[0]["gray"])
    d = np.ascontiguousarray(depth, np.float32).copy()
    n = np.ascontiguousarray(normal, np.float32).copy()
    c = np.zeros((h, w), np.float32)
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    ev = C.c_uint64(0)
    rc = lib().hcor_mask_estimate(C.byref(ref), srcs, len(views) - 1, O.u8ptr(gra), C.byref(params), None if k is None else O.u8ptr(k),
                                  d_min, d_max, O.fptr(d), O.fptr(n), O.fptr(c), C.byref(ev))
    assert rc == 0
    return d, n, c, ev.value


# ---- what happens before the estimate (numpy restatements) ---------------------------------------------------------------------

def parse_labels(arg):
    """--ignore-mask-label: Util::strSplit(s, ",") keeping empty tokens (libs/Common/Util.h:530-545), each token through atoi
    (DepthMap.cpp:319-348).  An empty string means no mask at all (None)."""
    if not arg:
        return None
    return [atoi(t) for t in arg.split(",")]


def atoi(t):
    """C atoi: leading blanks, an optional sign, the digits that follow; 0 when there are none (the value wraps to int32 as glibc's
    strtol-based atoi does for what fits in a long)"""
    m = re.match(r"\s*([+-]?\d+)", t)
    if not m:
        return 0
    v = int(m.group(1))
    v = max(min(v, (1 << 63) - 1), -(1 << 63))       # strtol saturates to LONG_MIN / LONG_MAX
    return ((v + (1 << 31)) % (1 << 32)) - (1 << 31)  # (int) of the long


def resize_nn(labels, w, h):
    """cv::resize(labels, Size(w, h), 0, 0, INTER_NEAREST): resizeNN with ifx = 1 / (w / sw), sx = min(floor(x * ifx), sw - 1)"""
    lab = np.asarray(labels)
    sh, sw = lab.shape
    if (sw, sh) == (w, h):
        return lab.copy()
    ifx = 1.0 / (w / sw); ify = 1.0 / (h / sh)
    sx = np.minimum(np.floor(np.arange(w, dtype=np.float64) * ifx).astype(np.int64), sw - 1)
    sy = np.minimum(np.floor(np.arange(h, dtype=np.float64) * ify).astype(np.int64), sh - 1)
    return lab[sy[:, None], sx[None, :]]


def keep_mask(labels, ignore, w, h):
    """DepthEstimator::ImportIgnoreMask: 1 where the resampled label equals none of the ignored labels"""
    r = resize_nn(np.asarray(labels, np.uint16), w, h).astype(np.int64)
    keep = np.ones((h, w), np.uint8)
    for v in ignore or []:
        keep[r == int(v)] = 0
    return keep


def median3_window_valid(keep, depth_init):
    """per pixel: how many of the 9 values of its 3x3 median window (edges replicated, as medianBlur does) come from pixels that are
    not ignored and hold a positive initial depth"""
    h, w = keep.shape
    ok = ((keep != 0) & (np.asarray(depth_init) > 0)).astype(np.int32)
    pad = np.pad(ok, 1, mode="edge")
    return sum(pad[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))

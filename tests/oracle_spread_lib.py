"""ctypes binding of the CPU oracle's estimate with view spread (tests/oracle_spread.c -> tests/libhcmvs_oracle_spread.so; DensifyPointCloud
--n-viewspread, DepthMap.cpp:1504-1608).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O
from oracle_mask_lib import oracle_cflags

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_spread.c")
LIB_PATH = os.path.join(HERE, "libhcmvs_oracle_spread.so")


class SpreadMap(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("depth", C.POINTER(C.c_float)), ("normal", C.POINTER(C.c_float)),
                ("conf", C.POINTER(C.c_float))]


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
        fp, u8p, vp, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(O.View), C.POINTER(C.c_uint64)
        L.hcor_spread_estimate.argtypes = [vp, vp, C.c_int, u8p, C.POINTER(O.Params), C.POINTER(SpreadMap), C.c_int, u8p, C.c_float, C.c_float,
                                           fp, fp, fp, u64p]
        L.hcor_spread_estimate.restype = C.c_int
        L.hcor_spread_stats.argtypes = [u64p, u64p, u64p, u64p, C.c_int]
        L.hcor_spread_stats.restype = None
        L.hcor_spread_trace_pixel.argtypes = [C.c_int, C.c_int]
        L.hcor_spread_trace_pixel.restype = None
        L.hcor_spread_trace_get.argtypes = [fp, C.c_int]
        L.hcor_spread_trace_get.restype = C.c_int
        L.hcor_spread_transform_depth.argtypes = [vp, vp, C.c_int, C.c_int, C.c_float, C.c_int]
        L.hcor_spread_transform_depth.restype = C.c_float
        _lib = L
    return _lib


def make_maps(maps):
    """maps: one entry per source view, None or (depth (h, w), normal (h, w, 3), conf (h, w)).  Returns the ctypes array (keeps the arrays
    alive); the size of an entry is the size of its depth map -- a view spreads only when that equals its image size."""
    arr = (SpreadMap * max(len(maps), 1))()
    keep = []
    for i, m in enumerate(maps):
        if m is None:
            continue
        d = np.ascontiguousarray(m[0], np.float32); n = np.ascontiguousarray(m[1], np.float32); c = np.ascontiguousarray(m[2], np.float32)
        assert n.shape == d.shape + (3,) and c.shape == d.shape
        arr[i].height, arr[i].width = d.shape
        arr[i].depth = O.fptr(d); arr[i].normal = O.fptr(n); arr[i].conf = O.fptr(c)
        keep += [d, n, c]
    arr._keep = keep
    return arr


def stats(reset=False):
    """(slots scored, slots accepted, slots dropped by the depth <= 0 rule, candidates outside view j's map) since the last reset"""
    v = [C.c_uint64() for _ in range(4)]
    lib().hcor_spread_stats(*[C.byref(x) for x in v], int(reset))
    return tuple(int(x.value) for x in v)


def estimate(views, params, d_min, d_max, depth, normal, maps=None, on=True, keep=None, gra=None, conf=None):
    """oracle_lib.estimate with view spread: maps as make_maps takes them (None: no view has maps), on = --n-viewspread.
    Returns depth, normal, conf, evals."""
    ref = O.make_view(views[0]); srcs = O.make_view_array(views[1:])
    h, w = views[0]["gray"].shape
    if gra is None:
        gra = O.gradient_map(views[0]["gray"])
    d = np.ascontiguousarray(depth, np.float32).copy()
    n = np.ascontiguousarray(normal, np.float32).copy()
    c = np.zeros((h, w), np.float32) if conf is None else np.ascontiguousarray(conf, np.float32).copy()
    sm = None if maps is None else make_maps(maps)
    assert maps is None or len(maps) == len(views) - 1
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    ev = C.c_uint64(0)
    rc = lib().hcor_spread_estimate(C.byref(ref), srcs, len(views) - 1, O.u8ptr(gra), C.byref(params), sm, int(bool(on)),
                                    None if k is None else O.u8ptr(k), d_min, d_max, O.fptr(d), O.fptr(n), O.fptr(c), C.byref(ev))
    assert rc == 0
    return d, n, c, ev.value


def trace(x, y):
    """start tracing pixel (x, y) (single-threaded runs only); trace_rows() returns what the runs since then recorded"""
    lib().hcor_spread_trace_pixel(int(x), int(y))


def trace_rows():
    buf = np.zeros((256, 8), np.float32)
    n = lib().hcor_spread_trace_get(O.fptr(buf), 256)
    return buf[:min(n, 256)].copy()


def transform_depth(ref, src, nx, ny, nd, mode=O.ARITH_REFERENCE):
    """DepthMap.cpp:1590-1592: the depth of view src's pixel (nx, ny, nd) in ref's camera frame"""
    r = O.make_view(ref); s = O.make_view(src)
    return float(lib().hcor_spread_transform_depth(C.byref(r), C.byref(s), int(nx), int(ny), C.c_float(nd), int(mode)))

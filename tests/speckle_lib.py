"""ctypes face of tests/speckle_plan_shim.cpp (hc-mvs_amd/csrc/speckle_plan.h) and tests/speckle_host_shim.cpp (speckle_host.h), each
built with g++ alone: no HIP, no library.  Shared by test_speckle_plan.py and test_speckle_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("speckle_plan.h", "speckle_host.h", "carve.h")]

ARGS = np.dtype([("depth", "<u8"), ("normal", "<u8"), ("conf", "<u8"), ("labels", "<u8"), ("w", "<i4"), ("h", "<i4")])
LAYOUT = ("result", "items", "first", "staged", "partials", "labels", "sizes", "bytes")
COUNTERS = ("n_valid", "n_removed", "n_segments", "n_small", "largest")

_lib = None
_host = None


def _build(stem):
    src, out = os.path.join(HERE, stem + ".cpp"), os.path.join(HERE, "lib" + stem + ".so")
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [src] + HDRS):
        # -ffp-contract=off as the library
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", out, src])
    return C.CDLL(out)


def lib():
    """the plan shim"""
    global _lib
    if _lib is None:
        L = _build("speckle_plan_shim")
        vp = C.c_void_p
        L.ss_constants.argtypes = [vp]; L.ss_constants.restype = None
        L.ss_default_threshold.restype = C.c_float
        L.ss_check.argtypes = [vp, C.c_int, C.c_float, C.c_char_p, C.c_int]
        L.ss_tiles.argtypes = [vp, C.c_int, vp, vp]
        L.ss_layout.argtypes = [C.c_int, C.c_uint64, C.c_uint64, vp]; L.ss_layout.restype = None
        L.ss_joined.argtypes = [C.c_float] * 3
        _lib = L
    return _lib


def host_lib():
    """the host-form shim"""
    global _host
    if _host is None:
        L = _build("speckle_host_shim")
        vp = C.c_void_p
        L.ss_host.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_float, C.c_uint32, vp]; L.ss_host.restype = None
        _host = L
    return _host


def constants():
    out = np.zeros(9, np.int32)
    lib().ss_constants(out.ctypes.data)
    return dict(zip(("args_bytes", "tile_w", "tile_h", "block", "max_items", "item_bytes", "partial_bytes", "result_bytes", "scratch_per_pixel"),
                    (int(v) for v in out)))


def args(items):
    """items: list of (depth, normal, conf, labels, w, h), addresses as integers"""
    a = np.zeros(max(len(items), 1), ARGS)
    for k, it in enumerate(items):
        a[k] = tuple(it)
    return a


def check(items, thr, n=None):
    """the reason a call is refused, or '' (items None: a null pointer)"""
    buf = C.create_string_buffer(200)
    if items is None:
        rc = lib().ss_check(None, 1 if n is None else n, thr, buf, 200)
    else:
        a = args(items)
        rc = lib().ss_check(a.ctypes.data, len(items) if n is None else n, thr, buf, 200)
    why = buf.value.decode()
    assert (rc == 0) == (why == "")
    return why


def tiles(items):
    a = args(items)
    n = len(items)
    first = np.zeros(n + 1, np.int64); pixel0 = np.zeros(n + 1, np.int64)
    fits = lib().ss_tiles(a.ctypes.data, n, first.ctypes.data, pixel0.ctypes.data)
    return first, pixel0, bool(fits)


def layout(n, n_tiles, n_pixels):
    out = np.zeros(8, np.uint64)
    lib().ss_layout(n, n_tiles, n_pixels, out.ctypes.data)
    return dict(zip(LAYOUT, (int(v) for v in out)))


def host(depth, normal=None, conf=None, thr=None, speckle_size=100, want_labels=True):
    """speckle_host on copies of the arrays: dict(depth, normal, conf, labels, stats)"""
    d = np.array(depth, np.float32, order="C")
    n = None if normal is None else np.array(normal, np.float32, order="C")
    c = None if conf is None else np.array(conf, np.float32, order="C")
    lab = np.full(d.shape, -7, np.int32) if want_labels else None
    cnt = np.zeros(5, np.uint64)
    thr = lib().ss_default_threshold() if thr is None else thr
    host_lib().ss_host(d.shape[1], d.shape[0], d.ctypes.data, None if n is None else n.ctypes.data, None if c is None else c.ctypes.data,
                  None if lab is None else lab.ctypes.data, thr, int(speckle_size), cnt.ctypes.data)
    return dict(depth=d, normal=n, conf=c, labels=lab, stats=dict(zip(COUNTERS, (int(v) for v in cnt))))

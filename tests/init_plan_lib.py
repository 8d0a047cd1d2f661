"""ctypes face of tests/init_plan_shim.cpp (hc-mvs_amd/csrc/init_plan.h + the set-up half of tri_init.cpp, built with g++ alone: no HIP, no
library) and the host loop's rule restated in numpy over the shim's tables.  Shared by test_init_plan.py and test_gpu_init_device.py."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc")
SRCS = [os.path.join(HERE, "init_plan_shim.cpp"), os.path.join(CSRC, "tri_init.cpp")]
HDRS = [os.path.join(CSRC, h) for h in ("init_plan.h", "tri_init.h", "carve.h")]
LIB_PATH = os.path.join(HERE, "libinit_plan_shim.so")

FACE = np.dtype([("X", "<i8", 3), ("Y", "<i8", 3), ("C", "<i8", 3), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"),
                 ("nn", "<f4", 3), ("np", "<f4", 3), ("index", "<i4"), ("pad", "<i4")])

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in SRCS + HDRS):
            # -ffp-contract=off as the library: the planes are float expressions
            subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH] + SRCS)
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.ip_tile_shape.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ip_tile_shape.restype = None
        L.ip_tri_plan.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, C.c_int, C.POINTER(C.c_int), vp, vp]
        L.ip_splat_plan.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        L.ip_splat_plan.restype = None
        L.ip_bin.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), vp, vp, C.c_longlong]
        L.ip_bin.restype = C.c_longlong
        L.ip_layout.argtypes = [C.c_ulonglong] * 3 + [vp]
        L.ip_layout.restype = None
        assert L.ip_face_bytes() == FACE.itemsize
        _lib = L
    return _lib


def tile_shape():
    w, h = C.c_int(), C.c_int()
    lib().ip_tile_shape(C.byref(w), C.byref(h))
    return w.value, h.value


def _cam(K, R, Cc):
    return [np.ascontiguousarray(a, np.float64) for a in (K, R, Cc)]


def tri_table(w, h, K, R, Cc, pts, avg_depth=0.0, add_corners=True):
    """the face table of the triangulation: dict(faces FACE[n], n_used, lo, hi, cam (fx, fy, cx, cy) f32), or None when no point is in front"""
    K, R, Cc = _cam(K, R, Cc)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    cap = 2 * (len(pts) + 4) + 16       # a triangulation of m points in a rectangle has fewer than 2 m faces
    faces = np.zeros(cap, FACE)
    used = C.c_int()
    rng = np.zeros(2, np.float32); cam = np.zeros(4, np.float32)
    n = lib().ip_tri_plan(w, h, K.ctypes.data, R.ctypes.data, Cc.ctypes.data, pts.ctypes.data, len(pts), avg_depth, int(add_corners), faces.ctypes.data, cap,
                          C.byref(used), rng.ctypes.data, cam.ctypes.data)
    if n < 0:
        return None
    assert n <= cap
    return dict(faces=faces[:n], n_used=used.value, lo=rng[0], hi=rng[1], cam=cam)


def splat_table(w, h, K, R, Cc, pts):
    """dict(xy (n, 2) i32, d (n,) f32, box (n, 4) i32 half open, lo, hi)"""
    K, R, Cc = _cam(K, R, Cc)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = len(pts)
    xy = np.zeros((n, 2), np.int32); d = np.zeros(n, np.float32); box = np.zeros((n, 4), np.int32); rng = np.zeros(2, np.float32)
    lib().ip_splat_plan(w, h, K.ctypes.data, R.ctypes.data, Cc.ctypes.data, pts.ctypes.data, n, xy.ctypes.data, d.ctypes.data, box.ctypes.data, rng.ctypes.data)
    return dict(xy=xy, d=d, box=box, lo=rng[0], hi=rng[1])


def face_boxes(faces):
    return np.stack([faces["x0"], faces["y0"], faces["x1"], faces["y1"]], -1).astype(np.int32)


def bin_tiles(w, h, boxes):
    """(tilesX, tilesY, first, items) of bin_tiles over boxes (n, 4)"""
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
    tw, th = tile_shape()
    n_tiles = ((w + tw - 1) // tw) * ((h + th - 1) // th)
    first = np.zeros(n_tiles + 1, np.uint32)
    tx, ty = C.c_int(), C.c_int()
    n = lib().ip_bin(w, h, boxes.ctypes.data, len(boxes), C.byref(tx), C.byref(ty), first.ctypes.data, None, 0)
    assert n >= 0
    items = np.zeros(max(n, 1), np.uint32)
    assert lib().ip_bin(w, h, boxes.ctypes.data, len(boxes), C.byref(tx), C.byref(ty), first.ctypes.data, items.ctypes.data, n) == n
    assert tx.value * ty.value == n_tiles
    return tx.value, ty.value, first, items[:n]


def layout(table_bytes, n_tiles, n_entries):
    out = np.zeros(5, np.uint64)
    lib().ip_layout(table_bytes, n_tiles, n_entries, out.ctypes.data)
    return [int(v) for v in out]


def raster_faces(tab, w, h):
    """The host loop's rule over a face table, in numpy: faces in table order, a later one overwrites, z > 0.  float32 throughout, the
    expression left to right.  Returns (depth, normal, hits)."""
    depth = np.zeros((h, w), np.float32); normal = np.zeros((h, w, 3), np.float32)
    fx, fy, cx, cy = (np.float32(v) for v in tab["cam"])
    one = np.float32(1)
    hits = 0
    for f in tab["faces"]:
        x0, y0, x1, y1 = int(f["x0"]), int(f["y0"]), int(f["x1"]), int(f["y1"])
        if x0 >= x1 or y0 >= y1:
            continue
        X, Y, Cc = f["X"], f["Y"], f["C"]
        xs = (np.arange(x0, x1, dtype=np.int64) << 4)[None, :]
        ys = (np.arange(y0, y1, dtype=np.int64) << 4)[:, None]
        m = np.ones((y1 - y0, x1 - x0), bool)
        for k in range(3):
            dx, dy = X[k] - X[(k + 1) % 3], Y[k] - Y[(k + 1) % 3]
            m &= Cc[k] + dx * ys - dy * xs > 0
        X0x = ((np.arange(x0, x1).astype(np.float32) - cx) / fx)[None, :]
        X0y = ((np.arange(y0, y1).astype(np.float32) - cy) / fy)[:, None]
        npv = f["np"]
        with np.errstate(all="ignore"):
            z = one / ((npv[0] * X0x + npv[1] * X0y) + npv[2] * one)
        assert z.dtype == np.float32
        m &= z > 0
        hits += int(m.sum())
        depth[y0:y1, x0:x1][m] = z[m]
        normal[y0:y1, x0:x1][m] = f["nn"]
    return depth, normal, hits


def raster_splats(tab, w, h):
    """the splat's rule: points in order, a later one overwrites its clamped 5 x 5 block.  Returns (depth, hits)"""
    depth = np.zeros((h, w), np.float32)
    hits = 0
    for (x0, y0, x1, y1), d in zip(tab["box"], tab["d"]):
        if x0 >= x1 or y0 >= y1:
            continue
        depth[y0:y1, x0:x1] = d
        hits += int((y1 - y0) * (x1 - x0))
    return depth, hits

"""ctypes binding of the oracle variant with the geometric-consistency term (tests/oracle_geo.c -> tests/libhcmvs_oracle_geo.so).  Test
infrastructure only; the flags are those of oracle/Makefile (-ffp-contract=off is the one that matters)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_geo.c")
LIB_PATH = os.path.join(HERE, "libhcmvs_oracle_geo.so")

CLASSES = ("consistent", "worst", "outside", "nodepth", "behind", "nomaps")
GEO_DEFAULTS = dict(on=0, para_tapa=0.25, para_tapa2=0.15, txthreshold=150.0, txthreshold2=160.0, photo2geo=2, max_px=3.0)


class GeoParams(C.Structure):
    _fields_ = [("on", C.c_int), ("para_tapa", C.c_float), ("para_tapa2", C.c_float), ("txthreshold", C.c_float), ("txthreshold2", C.c_float),
                ("photo2geo", C.c_int), ("max_px", C.c_float)]


def geo_params(**kw):
    p = GeoParams()
    for k, v in dict(GEO_DEFAULTS, **kw).items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def _cflags():
    """CFLAGS of oracle/Makefile"""
    with open(os.path.join(O.ORACLE_DIR, "Makefile")) as f:
        m = re.search(r"^CFLAGS\s*=\s*(.*)$", f.read(), re.M)
    return m.group(1).split()


def build():
    deps = [SRC] + [os.path.join(O.ORACLE_DIR, n) for n in ("hcmvs_oracle.c", "hcmvs_spread.inc", "hcmvs_oracle.h", "portable_math.h", "Makefile")]
    if os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return
    tmp = "%s.%d.tmp" % (LIB_PATH, os.getpid())
    subprocess.check_call([os.environ.get("CC", "gcc")] + _cflags() + ["-shared", "-o", tmp, SRC, "-lm"])
    os.replace(tmp, LIB_PATH)


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        fp = C.POINTER(C.c_float)
        L.hcor_geo_view_consts.argtypes = [C.POINTER(O.View), C.POINTER(O.View), fp]
        L.hcor_geo_view_consts.restype = None
        L.hcor_geo_weight.argtypes = [C.POINTER(GeoParams), C.c_int]
        L.hcor_geo_weight.restype = C.c_float
        L.hcor_geo_pair.argtypes = [C.POINTER(O.View), C.POINTER(O.View), C.POINTER(O.SpreadMap), C.POINTER(O.Params), C.c_int, C.c_int, C.c_float, fp,
                                    C.c_float, fp]
        L.hcor_geo_pair.restype = None
        L.hcor_geo_blend.argtypes = [C.c_float, C.c_float, C.c_float]
        L.hcor_geo_blend.restype = C.c_float
        L.hcor_geo_estimate.argtypes = [C.POINTER(O.View), C.POINTER(O.View), C.c_int, C.POINTER(C.c_uint8), C.POINTER(O.Params), C.c_float, C.c_float,
                                        fp, fp, fp, C.POINTER(GeoParams), C.POINTER(O.SpreadMap), C.POINTER(C.c_uint64)]
        L.hcor_geo_estimate.restype = C.c_int
        _lib = L
    return _lib


def view_consts(ref, src):
    """dict(cx, cy, ifx, ify, B (3, 3), b (3,), Rr (3, 3)) of source view src against ref, as D14 holds them (float32)"""
    out = np.zeros(25, np.float32)
    r = O.make_view(ref); s = O.make_view(src)
    lib().hcor_geo_view_consts(C.byref(r), C.byref(s), O.fptr(out))
    return dict(cx=out[0], cy=out[1], ifx=out[2], ify=out[3], B=out[4:13].reshape(3, 3).copy(), b=out[13:16].copy(), Rr=out[16:25].reshape(3, 3).copy())


def weight(gra, **kw):
    gp = geo_params(**kw)
    return float(lib().hcor_geo_weight(C.byref(gp), int(gra)))


def pair(ref, src, maps, x, y, depth, normal, max_px=3.0, params=None):
    """one (hypothesis, source view) pair: maps = None or (depth, normal, conf) of the source view.
    Returns dict(geo, cls (a name of CLASSES), e, c, x1 (x, y))"""
    r = O.make_view(ref); s = O.make_view(src)
    p = params if params is not None else O.default_params(arith_mode=O.ARITH_DEVICE)
    sm = O.make_maps([maps])
    n = np.ascontiguousarray(normal, np.float32)
    out = np.zeros(6, np.float32)
    lib().hcor_geo_pair(C.byref(r), C.byref(s), sm, C.byref(p), int(x), int(y), C.c_float(depth), O.fptr(n), C.c_float(max_px), O.fptr(out))
    return dict(geo=float(out[0]), cls=CLASSES[int(out[1])], e=float(out[2]), c=float(out[3]), x1=(float(out[4]), float(out[5])))


def blend(s, w, geo):
    return float(lib().hcor_geo_blend(C.c_float(s), C.c_float(w), C.c_float(geo)))


def estimate(views, params, d_min, d_max, depth, normal, maps=None, geo=None, keep=None, gra=None):
    """hcor_geo_estimate on views[0] (ref) against views[1:].  maps: one entry per source view, None or (depth, normal, conf) at the view's
    size (None: no view offers maps); geo: dict of GeoParams fields (None: the term is off).  The maps are copied.
    Returns depth, normal, conf, dict(evals, evals_geo, pixels_geo, pairs = the blended pairs by class, pixels_w = (para_tapa, para_tapa2,
    0), pairs_all = the pairs of the pixels with a weight by class, failed views included)."""
    ref = O.make_view(views[0]); srcs = O.make_view_array(views[1:])
    h, w = views[0]["gray"].shape
    if gra is None:
        gra = O.gradient_map(views[0]["gray"])
    gra = np.ascontiguousarray(gra, np.uint8)
    d = np.ascontiguousarray(depth, np.float32).copy()
    n = np.ascontiguousarray(normal, np.float32).copy()
    c = np.zeros((h, w), np.float32)
    p = O.Params.from_buffer_copy(params)
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    if k is not None:
        p.keep = O.u8ptr(k)
    assert maps is None or len(maps) == len(views) - 1
    sm = None if maps is None else O.make_maps(maps)
    gp = geo_params(**(geo or {}))
    st = (C.c_uint64 * 18)()
    rc = lib().hcor_geo_estimate(C.byref(ref), srcs, len(views) - 1, O.u8ptr(gra), C.byref(p), d_min, d_max, O.fptr(d), O.fptr(n), O.fptr(c),
                                 C.byref(gp) if geo is not None else None, sm, st)
    assert rc == 0, rc
    return d, n, c, dict(evals=int(st[0]), evals_geo=int(st[1]), pixels_geo=int(st[2]), pairs={k: int(st[3 + i]) for i, k in enumerate(CLASSES)},
                         pixels_w=(int(st[9]), int(st[10]), int(st[11])), pairs_all={k: int(st[12 + i]) for i, k in enumerate(CLASSES)})

"""ctypes binding of the oracle variant with a depth prior (tests/oracle_prior.c -> tests/libhcmvs_oracle_prior.so).  Test infrastructure
only; the flags are those of oracle/Makefile (-ffp-contract=off is the one that matters)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "oracle_prior.c")
LIB_PATH = os.path.join(HERE, "libhcmvs_oracle_prior.so")


class Prior(C.Structure):
    _fields_ = [("map", C.POINTER(C.c_float)), ("para_prior", C.c_float), ("sigma_prior", C.c_float), ("photo2geo", C.c_int)]


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
        L.hcor_prior_usable.argtypes = [C.c_float]
        L.hcor_prior_usable.restype = C.c_int
        L.hcor_prior_consts.argtypes = [C.c_float, C.c_float, fp]
        L.hcor_prior_consts.restype = None
        L.hcor_prior_addend.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]
        L.hcor_prior_addend.restype = C.c_float
        L.hcor_prior_blend.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int]
        L.hcor_prior_blend.restype = C.c_float
        L.hcor_prior_score_pixel.argtypes = [C.POINTER(O.View), C.POINTER(O.View), C.c_int, C.POINTER(C.c_uint8), C.POINTER(O.Params), C.c_int, C.c_int,
                                             C.c_float, fp, C.c_float, C.c_float, C.c_float, C.c_int, fp]
        L.hcor_prior_score_pixel.restype = C.c_float
        L.hcor_prior_estimate.argtypes = [C.POINTER(O.View), C.POINTER(O.View), C.c_int, C.POINTER(C.c_uint8), C.POINTER(O.Params), C.c_float, C.c_float,
                                          fp, fp, fp, C.POINTER(Prior), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.hcor_prior_estimate.restype = C.c_int
        _lib = L
    return _lib


PRIOR_DEFAULTS = dict(para_prior=0.5, sigma_prior=0.2, photo2geo=2)


def usable(x):
    return bool(lib().hcor_prior_usable(C.c_float(x)))


def consts(para, sigma):
    """(1 - para_prior, -1 / (2 sigma^2)) as the oracle derives them for the device association"""
    out = (C.c_float * 2)()
    lib().hcor_prior_consts(C.c_float(para), C.c_float(sigma), out)
    return float(out[0]), float(out[1])


def addend(prior, depth, para, sigma, mode):
    return float(lib().hcor_prior_addend(C.c_float(prior), C.c_float(depth), C.c_float(para), C.c_float(sigma), int(mode)))


def blend(score, prior, depth, para, sigma, mode):
    return float(lib().hcor_prior_blend(C.c_float(score), C.c_float(prior), C.c_float(depth), C.c_float(para), C.c_float(sigma), int(mode)))


def score_pixel(views, params, x, y, depth, normal, prior, para=0.5, sigma=0.2, photo2geo=2, gra=None):
    """ScorePixel of views[0] against views[1:] at (x, y), no smoothness neighbours, with the prior value `prior` at the pixel.
    Returns (score, the V blended view scores)"""
    ref = O.make_view(views[0]); srcs = O.make_view_array(views[1:])
    if gra is None:
        gra = O.gradient_map(views[0]["gray"])
    n = np.ascontiguousarray(normal, np.float32)
    vs = np.zeros(len(views) - 1, np.float32)
    s = lib().hcor_prior_score_pixel(C.byref(ref), srcs, len(views) - 1, O.u8ptr(gra), C.byref(params), int(x), int(y), C.c_float(depth), O.fptr(n),
                                     C.c_float(prior), C.c_float(para), C.c_float(sigma), int(photo2geo), O.fptr(vs))
    return float(s), vs


def estimate(views, params, d_min, d_max, depth, normal, conf=None, prior=None, para_prior=0.5, sigma_prior=0.2, photo2geo=2, keep=None, gra=None,
             sweeps=None):
    """hcor_prior_estimate on views[0] (ref) against views[1:].  prior: (h, w) float32 or None.  sweeps = (first_sweep, n_sweeps) runs the
    sweeps-only entry on depth, normal and conf (the state an estimate leaves between outer iterations).  The maps are copied.
    Returns depth, normal, conf, dict(evals, evals_prior, pixels_prior)."""
    ref = O.make_view(views[0]); srcs = O.make_view_array(views[1:])
    h, w = views[0]["gray"].shape
    if gra is None:
        gra = O.gradient_map(views[0]["gray"])
    d = np.ascontiguousarray(depth, np.float32).copy()
    n = np.ascontiguousarray(normal, np.float32).copy()
    c = np.zeros((h, w), np.float32) if conf is None else np.ascontiguousarray(conf, np.float32).copy()
    p = O.Params.from_buffer_copy(params)
    k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    if k is not None:
        p.keep = O.u8ptr(k)
    pr = Prior(); pr.para_prior = para_prior; pr.sigma_prior = sigma_prior; pr.photo2geo = photo2geo
    pm = None
    if prior is not None:
        pm = np.ascontiguousarray(prior, np.float32)
        assert pm.shape == (h, w)
        pr.map = O.fptr(pm)
    st = (C.c_uint64 * 3)()
    first, count = sweeps if sweeps is not None else (0, 0)
    rc = lib().hcor_prior_estimate(C.byref(ref), srcs, len(views) - 1, O.u8ptr(gra), C.byref(p), d_min, d_max, O.fptr(d), O.fptr(n), O.fptr(c),
                                   C.byref(pr), int(sweeps is not None), int(first), int(count), st)
    assert rc == 0, rc
    return d, n, c, dict(evals=int(st[0]), evals_prior=int(st[1]), pixels_prior=int(st[2]))

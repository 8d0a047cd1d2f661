"""What the geometric-consistency term adds to the host plans (hc-mvs_amd/csrc/est_plan.h, sweep_plan.h), on the
CPU: the refusals of the options, the activity rule, the batch-level refusals, GeoView against numpy in double and against the oracle
variant's own derivation, the term's constants, the aliasing rule, where the GeoItem lies, and the GEO kernel instances -- one exists if
and only if the PRIOR instance of the same shape does.  tests/geo_plan_shim.cpp is compiled with g++ alone, with -ffp-contract=off as the
library is: no HIP, no library."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import oracle_geo_lib as G

synth = importlib.import_module("hc-mvs_amd.synth")

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc")
SRC = os.path.join(HERE, "geo_plan_shim.cpp")
HDRS = [os.path.join(CSRC, h) for h in ("est_plan.h", "pm_types.h", "sweep_plan.h", "carve.h")] + [os.path.join(os.path.dirname(HERE), "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libgeo_plan_shim.so")
f32 = np.float32
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.gp_check_params.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float]
    L.gp_view.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.gp_view.restype = None
    L.gp_consts.argtypes = [C.c_float] * 5 + [C.c_int, C.POINTER(C.c_float)]
    L.gp_check_batch.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.gp_layout.argtypes = [C.POINTER(C.c_int)]
    L.gp_layout.restype = None
    L.gp_overlap.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_int]
    L.gp_resolve.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_int)]
    L.gp_resolve.restype = None
    L.gp_plan.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    return L


def test_the_refusals_of_the_options(lib):
    ok = (0.25, 0.15, 150.0, 160.0, 2, 3.0)
    assert lib.gp_check_params(*ok) == 0 and lib.gp_check_params(0.0, 1.0, -5.0, 1e9, 0, 1e-6) == 0 and lib.gp_check_params(0.26, 0.26, 150, 160, 1, 3) == 0
    for bad in (-0.001, 1.001, NAN, INF, -INF):
        assert lib.gp_check_params(bad, 0.15, 150, 160, 2, 3) == 1 and lib.gp_check_params(0.25, bad, 150, 160, 2, 3) == 1
    for bad in (NAN, INF, -INF):
        assert lib.gp_check_params(0.25, 0.15, bad, 160, 2, 3) == 2 and lib.gp_check_params(0.25, 0.15, 150, bad, 2, 3) == 2
    for bad in (0.0, -3.0, NAN, INF):
        assert lib.gp_check_params(0.25, 0.15, 150, 160, 2, bad) == 3
    assert lib.gp_check_params(0.25, 0.15, 150, 160, -1, 3) == 4
    assert lib.gp_check_params(2.0, 0.15, NAN, 160, -1, 0) == 1        # the first broken rule is reported


def test_the_activity_rule(lib):
    assert lib.gp_offers(1, 0) == 1 and lib.gp_offers(0, 0) == 0 and lib.gp_offers(1, 1) == 0
    for on, p2g, it, offers, want in ((1, 2, 2, 1, 1), (1, 2, 3, 1, 1), (1, 2, 1, 1, 0), (0, 2, 2, 1, 0), (1, 2, 2, 0, 0), (1, 0, 0, 1, 1), (1, 1, 1, 1, 1)):
        assert lib.gp_active(on, p2g, it, offers) == want


def _cam(v):
    return (C.c_double * 21)(*np.concatenate([np.asarray(v["K"], np.float64).ravel(), np.asarray(v["R"], np.float64).ravel(), np.asarray(v["C"], np.float64).ravel()]))


def test_geoview_against_numpy_in_double_and_against_the_oracle_variant(lib):
    views = synth.make_views(96, 80, 90.0, 5, seed=21)
    ref = views[0]
    Ki, Ri, Ci = (np.asarray(ref[k], np.float64) for k in ("K", "R", "C"))
    for s in views[1:]:
        Kj, Rj, Cj = (np.asarray(s[k], np.float64) for k in ("K", "R", "C"))
        out = (C.c_float * 27)()
        lib.gp_view(_cam(ref), _cam(s), 77, 55, out)
        got = np.array(out[:], np.float32)
        assert (got[0], got[1]) == (77, 55)
        B = Ki @ Ri @ Rj.T; b = Ki @ Ri @ (Cj - Ci); Rr = Ri @ Rj.T
        want = np.concatenate([[Kj[0, 2], Kj[1, 2], 1.0 / Kj[0, 0], 1.0 / Kj[1, 1]], B.ravel(), b, Rr.ravel()])
        # numpy's products associate as the plan's do not have to: equal to a float32 ulp or two, in double
        np.testing.assert_allclose(got[2:].astype(np.float64), want, rtol=3e-7, atol=1e-9 * np.abs(want).max())
        o = G.view_consts(ref, s)     # the oracle variant's derivation: the same bits
        mine = np.concatenate([[o["cx"], o["cy"], o["ifx"], o["ify"]], o["B"].ravel(), o["b"], o["Rr"].ravel()]).astype(np.float32)
        assert np.array_equal(got[2:], mine)
    # a point of view j's camera lands where the two cameras say: X = R_j^T Xc + C_j, pixel = K_i R_i (X - C_i)
    s = views[2]
    Kj, Rj, Cj = (np.asarray(s[k], np.float64) for k in ("K", "R", "C"))
    Xc = np.array([0.3, -0.2, 4.0])
    X = Rj.T @ Xc + Cj
    p = Ki @ Ri @ (X - Ci)
    o = G.view_consts(ref, s)
    q = o["B"].astype(np.float64) @ Xc + o["b"].astype(np.float64)
    np.testing.assert_allclose(q[:2] / q[2], p[:2] / p[2], atol=1e-3)


def test_the_constants(lib):
    out = (C.c_float * 7)()
    assert lib.gp_consts(0.25, 0.15, 150, 160, 3.0, -1, out) == -1
    assert out[:] == [0.25, float(f32(0.15)), 0.75, float(f32(1) - f32(0.15)), 150.0, 160.0, 3.0]
    assert lib.gp_consts(0.26, 0.26, 10, 20, 2.5, 4, out) == 4
    assert out[:] == [float(f32(0.26)), float(f32(0.26)), float(f32(1) - f32(0.26)), float(f32(1) - f32(0.26)), 10.0, 20.0, 2.5]


def check_batch(lib, flags):
    at = C.c_int(-7)
    rc = lib.gp_check_batch((C.c_int * (4 * len(flags)))(*itertools.chain(*flags)), len(flags), C.byref(at))
    return rc, at.value


def test_the_batch_refusals(lib):
    assert check_batch(lib, [(1, 0, 0, 0)]) == (0, -1)
    assert check_batch(lib, [(0, 1, 1, 1), (0, 0, 1, 0)]) == (0, -1)          # the term active nowhere: nothing is refused
    assert check_batch(lib, [(1, 1, 0, 0)]) == (1, 0)
    assert check_batch(lib, [(1, 0, 1, 0)]) == (2, 0)
    assert check_batch(lib, [(1, 0, 0, 1)]) == (3, 0)
    assert check_batch(lib, [(1, 0, 0, 0), (0, 0, 0, 0), (0, 1, 0, 0)]) == (1, 2)      # anywhere in the batch
    assert check_batch(lib, [(0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 0)]) == (2, 1)      # the hint first, then view spread, then the prior
    assert check_batch(lib, [(0, 0, 0, 1), (1, 0, 0, 0)]) == (3, 0)


def test_the_geoitem_lies_behind_the_prioritem_inside_the_slot(lib):
    out = (C.c_int * 8)()
    lib.gp_layout(out)
    est, dv, pi, gi, gv, entries, at, slot = out[:]
    assert entries == 18 and at == 16 * dv + pi and at % 8 == 0 and at + gi <= slot == entries * dv and gv % 8 == 0
    assert lib.gp_sweep_item_geo(1) == 1 and lib.gp_sweep_item_geo(0) == 0


def test_the_aliasing_rule(lib):
    w, h, sw, sh = 96, 80, 64, 48
    n, m = w * h, sw * sh
    io = [1 << 20, 2 << 20, 3 << 20]

    def run(sp, active=1, io=io):
        return lib.gp_overlap(w, h, (C.c_uint64 * 3)(*io), sw, sh, (C.c_uint64 * 2)(*sp), active)
    assert run([8 << 20, 9 << 20]) == -1
    assert run([io[0] + 4 * n, 9 << 20]) == -1 and run([io[0] + 4 * n - 1, 9 << 20]) == 0       # the depth map read touches the depth written
    assert run([8 << 20, io[1] + 12 * n - 1]) == 0 and run([8 << 20, io[2] - 12 * m + 1]) == 0  # the normal map read, against normal and conf
    assert run([io[0], io[1]], active=0) == -1                                                 # an item without the term reads nothing


def test_a_geo_instance_exists_exactly_where_the_prior_instance_does(lib):
    count = 0
    for nw, big, two, pack, hint, mask, spread in itertools.product(range(0, 6), *[(0, 1)] * 6):
        prior = lib.gp_exists(nw, big, two, pack, hint, mask, spread, 1, 0)
        geo = lib.gp_exists(nw, big, two, pack, hint, mask, spread, 0, 1)
        assert prior == geo
        assert geo == (lib.gp_exists(nw, big, two, pack, hint, mask, spread, 0, 0) and not (hint or spread))
        assert lib.gp_exists(nw, big, two, pack, hint, mask, spread, 1, 1) == 0           # never with the prior
        count += geo
    assert count == 48


def test_resolve_and_plan_carry_the_bit(lib):
    out = (C.c_int * 10)()
    for requested, V, big, mask in itertools.product((0, 1, 2, 3, 4, 9), (1, 3, 8, 10, 16), (0, 1), (0, 1)):
        lib.gp_resolve(requested, V, big, 0, mask, 0, 0, 1, out)
        geo = out[:]
        lib.gp_resolve(requested, V, big, 0, mask, 0, 1, 0, out)
        prior = out[:]
        assert geo[8] == 1 and geo[7] == 0 and geo[9] == 1 and geo[:7] == prior[:7]          # the same shape as the PRIOR launch
        lib.gp_resolve(requested, V, big, 0, mask, 0, 0, 0, out)
        assert out[8] == 0 and out[:7] == geo[:7]
    items = [(66, 82, 3, 0, 0), (66, 82, 3, 0, 1), (98, 130, 3, 1, 0)]              # an item with the term between two without
    flat = (C.c_int * 15)(*itertools.chain(*items))
    for per_launch in (0, 1, 2):
        plan = (C.c_int * 40)()
        n = lib.gp_plan(flat, 3, 3, per_launch, plan, 8)
        assert n >= 1 and all(plan[5 * i + 3] == 1 and plan[5 * i + 4] == 1 for i in range(n))
        assert sum(plan[5 * i + 1] for i in range(n)) == 3
    plain = (C.c_int * 15)(*itertools.chain(*[(r, c, v, m, 0) for r, c, v, m, _ in items]))
    plan = (C.c_int * 40)()
    n = lib.gp_plan(plain, 3, 3, 0, plan, 8)
    assert all(plan[5 * i + 3] == 0 for i in range(n))

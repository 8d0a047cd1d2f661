"""What the depth prior adds to the host plans (hc-mvs_amd/csrc/est_plan.h, sweep_plan.h), on the CPU: the refusals of the prior options,
the active-prior rule, the batch-level refusals with the hint and with view spread, the term's constants bit for bit against the oracle's
own derivation (oracle/hcmvs_oracle.c), the range of the sweeps-only call, the PRIOR kernel instances and the first-sweep offset.
tests/prior_plan_shim.cpp is compiled with g++ alone, with -ffp-contract=off as the library is: no HIP, no library."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc")
SRC = os.path.join(HERE, "prior_plan_shim.cpp")
HDRS = [os.path.join(CSRC, h) for h in ("est_plan.h", "pm_types.h", "sweep_plan.h", "carve.h")] + [os.path.join(os.path.dirname(HERE), "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libprior_plan_shim.so")
f32 = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.pp_check_params.argtypes = [C.c_float, C.c_float, C.c_int]
    L.pp_active.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_int]
    L.pp_consts.argtypes = [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_float)]
    L.pp_check_batch.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.pp_layout.argtypes = [C.POINTER(C.c_int)]
    L.pp_layout.restype = None
    L.pp_resolve.argtypes = [C.c_int] * 7 + [C.POINTER(C.c_int)]
    L.pp_resolve.restype = None
    L.pp_plan.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int]
    return L


def test_the_three_refusals_of_the_options(lib):
    assert lib.pp_check_params(0.5, 0.2, 2) == 0 and lib.pp_check_params(0.0, 1e-6, 0) == 0 and lib.pp_check_params(1.0, 5.0, 100) == 0
    for para in (-0.001, 1.001, float("nan"), float("inf"), float("-inf")):
        assert lib.pp_check_params(para, 0.2, 2) == 1
    for sigma in (0.0, -0.2, float("nan"), float("inf")):
        assert lib.pp_check_params(0.5, sigma, 2) == 2
    assert lib.pp_check_params(0.5, 0.2, -1) == 3
    assert lib.pp_check_params(2.0, 0.0, -1) == 1        # the first broken rule is reported


def test_the_active_prior_rule(lib):
    for registered, para, p2g, it, want in ((1, 0.5, 2, 2, 1), (1, 0.5, 2, 3, 1), (1, 0.5, 2, 1, 0), (0, 0.5, 2, 2, 0), (1, 0.0, 2, 2, 0), (1, 0.5, 0, 0, 1),
                                            (1, 1e-6, 1, 1, 1)):
        assert lib.pp_active(registered, para, 0.2, p2g, it) == want


def test_the_constants_against_the_oracle(lib):
    rng = np.random.default_rng(5)
    cases = [(0.5, 0.2), (0.4, 0.2), (1.0, 0.05), (1e-3, 3.0)] + [(float(f32(rng.uniform(0, 1))), float(f32(rng.uniform(0.01, 2)))) for _ in range(50)]
    for para, sigma in cases:
        out = (C.c_float * 3)()
        assert lib.pp_consts(para, sigma, 4, out) == 4
        keep, sig = O.prior_consts(para, sigma)
        assert (float(out[0]), float(out[1]), float(out[2])) == (keep, float(f32(para)), sig)
        assert keep == float(f32(1) - f32(para)) and sig == float(f32(-1) / (f32(2) * (f32(sigma) * f32(sigma))))
    assert lib.pp_consts(0.5, 0.2, -1, (C.c_float * 3)()) == -1


def check_batch(lib, flags):
    at = C.c_int(-7)
    rc = lib.pp_check_batch((C.c_int * (3 * len(flags)))(*itertools.chain(*flags)), len(flags), C.byref(at))
    return rc, at.value


def test_the_hint_and_spread_refusals(lib):
    assert check_batch(lib, [(1, 0, 0)]) == (0, -1)
    assert check_batch(lib, [(0, 1, 1), (0, 1, 0)]) == (0, -1)                 # no prior anywhere: the hint and view spread as before
    assert check_batch(lib, [(1, 1, 0)]) == (1, 0)
    assert check_batch(lib, [(1, 0, 1)]) == (2, 0)
    assert check_batch(lib, [(0, 0, 0), (1, 0, 0), (0, 0, 1)]) == (2, 2)       # a batch is one set of launches
    assert check_batch(lib, [(0, 0, 1), (0, 1, 0), (1, 0, 0)]) == (1, 1)       # the hint is named first


def test_the_range_of_the_sweeps_only_call(lib):
    top = lib.pp_max_sweep_index()
    assert top == 62                                                           # stream it_external * 64 + 1 + index stays below the next iteration's 64
    assert lib.pp_check_sweeps(0, 1) == 0 and lib.pp_check_sweeps(5, 2) == 0 and lib.pp_check_sweeps(top, 1) == 0 and lib.pp_check_sweeps(0, top + 1) == 0
    for first, n in ((-1, 2), (0, 0), (3, -1), (top + 1, 1), (top, 2), (0, top + 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.pp_check_sweeps(first, n) == 1


def test_the_structures_keep_their_layout(lib):
    out = (C.c_int * 5)()
    lib.pp_layout(out)
    assert list(out) == [280, 60, 24, 18, 16 * 60]                             # EstConst and DevView as before; the PriorItem lies behind the 16 views
    assert out[4] % 8 == 0 and (out[3] * out[1]) % 8 == 0                      # ... 8-byte aligned in every slot
    assert lib.pp_sweep_item_prior(1) == 1 and lib.pp_sweep_item_prior(0) == 0


def test_prior_instances_exist_exactly_as_stated(lib):
    n_plain = n_prior = 0
    for nw, big, two, pack, hint, mask, spread in itertools.product(range(0, 6), *[(0, 1)] * 6):
        plain = lib.pp_exists(nw, big, two, pack, hint, mask, spread, 0)
        assert plain == lib.pp_exists_default(nw, big, two, pack, hint, mask, spread)
        prior = lib.pp_exists(nw, big, two, pack, hint, mask, spread, 1)
        assert prior == int(bool(plain) and not hint and not spread)
        n_plain += plain; n_prior += prior
    assert (n_plain, n_prior, n_plain + n_prior) == (152, 48, 200)


def test_resolve_and_plan_carry_the_prior_and_the_first_sweep(lib):
    out = (C.c_int * 9)()
    for requested, V, big, mask in itertools.product(range(0, 6), (1, 3, 8, 10, 16), (0, 1), (0, 1)):
        lib.pp_resolve(requested, V, big, 0, mask, 0, 1, out)
        assert out[7] == 1 and out[8] == 1                                     # every instance a prior launch resolves to exists
        plain = (C.c_int * 9)()
        lib.pp_resolve(requested, V, big, 0, mask, 0, 0, plain)
        assert list(out[:7]) == list(plain[:7]) and plain[7] == 0              # ... and is the plain one plus the flag
    items = [(66, 82, 3, 0, 0, 0, 0), (66, 82, 3, 0, 1, 0, 1)]
    flat = (C.c_int * 14)(*itertools.chain(*items))
    res = (C.c_int * 40)()
    n = lib.pp_plan(flat, 2, 2, 5, 1, res, 8)                                  # per-sweep launches: sweeps 5 and 6
    assert n == 2 and [res[0], res[1], res[5], res[6]] == [5, 1, 6, 1] and res[3] == 1 and res[4] == 1 and res[8] == 1
    n = lib.pp_plan(flat, 2, 2, 5, 2, res, 8)                                  # one launch: first 5, count 2
    assert n == 1 and [res[0], res[1], res[3], res[4]] == [5, 2, 1, 1]
    flat0 = (C.c_int * 7)(*items[0])
    n = lib.pp_plan(flat0, 1, 3, 0, 1, res, 8)                                 # no prior, no offset: as before
    assert n == 3 and [res[0], res[5], res[10]] == [0, 1, 2] and res[3] == 0

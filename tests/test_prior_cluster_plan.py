"""What the inlier clustering adds to the host half of hcmvs_generate_plane_prior_device
(hc-mvs_amd/csrc/prior_gen_plan.h), on the CPU: the refusals of cluster_mul, the cell edge against numpy (a product that underflows to 0
included), the cap, and the sizes and offsets of the two structs against the binding.  tests/prior_cluster_plan_shim.cpp is compiled with g++
alone, with -ffp-contract=off as the library is; the same file is also built as a stand-alone program under the address and
undefined-behaviour sanitizers and run once."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import plane_prior_cluster_ref as cref

binding = importlib.import_module("hc-mvs_amd.binding")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hc-mvs_amd", "csrc")
SRC = os.path.join(HERE, "prior_cluster_plan_shim.cpp")
HDRS = [os.path.join(CSRC, h) for h in ("prior_gen_plan.h", "knn_layout.h", "carve.h")] + [os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libprior_cluster_plan_shim.so")
F32, F64 = C.c_float, C.c_double


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.pcp_check.argtypes = [C.POINTER(binding.PlanePriorParams), C.c_char_p, C.c_int]
    L.pcp_cell.argtypes = [F64, F32]; L.pcp_cell.restype = F32
    L.pcp_cell_usable.argtypes = [F32]
    L.pcp_constants.argtypes = [C.POINTER(C.c_longlong)]; L.pcp_constants.restype = None
    return L


def params(**kw):
    p = binding.PlanePriorParams(255, 0.18, 0.3, 10, 0.01, 80.0, 2.0, 0.25, 256, 1)  # the documented defaults, without the library: cluster_mul is 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check(lib, **kw):
    buf = C.create_string_buffer(256)
    p = params(**kw)
    n = lib.pcp_check(C.byref(p), buf, 256)
    assert n == len(buf.value)
    return buf.value.decode()


def test_cluster_mul_is_refused_unless_finite_and_not_negative(lib):
    assert params().cluster_mul == 0.0 and check(lib) == ""
    for v in (0.0, 1e-45, 2.0, 7.0, 10.0, 3e38):
        assert check(lib, cluster_mul=v) == ""
    for v in (-1.0, -1e-45, float("nan"), float("inf"), float("-inf")):
        assert "cluster_mul" in check(lib, cluster_mul=v), v
    assert "probability" in check(lib, cluster_mul=-1.0, probability=0.0)          # the earlier refusals keep their order


def test_the_cell_edge_against_numpy(lib):
    rng = np.random.RandomState(5)
    for avg, mul in list(zip(rng.uniform(1e-3, 0.5, 200), rng.uniform(0.1, 20, 200))) + [(0.0921947, 7.0), (0.05, 1e-45), (0.4, 1e-45), (1e30, 1e30), (1e-300, 2.0), (0.07, 1e-9)]:
        got = lib.pcp_cell(avg, mul)
        with np.errstate(all="ignore"):
            want = np.float32(np.float64(avg) * np.float64(np.float32(mul)))
        assert np.float32(got).tobytes() == want.tobytes(), (avg, mul)
        assert float(np.float32(got)) == cref.cluster_cell(avg, mul)
        assert lib.pcp_cell_usable(got) == int(want > 0 and np.isfinite(want))
    assert lib.pcp_cell(0.05, 1e-45) == 0.0 and lib.pcp_cell_usable(0.0) == 0        # the product underflowed: nothing is clustered
    assert np.isinf(lib.pcp_cell(1e30, 1e30)) and lib.pcp_cell_usable(float("inf")) == 0 and lib.pcp_cell_usable(float("nan")) == 0
    assert lib.pcp_cell_usable(-1.0) == 0 and lib.pcp_cell_usable(1e-45) == 1


def test_constants_and_struct_layout_against_the_binding(lib):
    k = (C.c_longlong * 7)()
    lib.pcp_constants(k)
    assert k[0] == 1 << 30 == cref.CELL_CAP
    P, S = binding.PlanePriorParams, binding.PlanePriorStats
    assert k[1] == C.sizeof(P) and k[2] == C.sizeof(S)
    assert k[3] == P.cluster_mul.offset and P._fields_[-1][0] == "cluster_mul"           # the new last field
    assert [k[4], k[5], k[6]] == [S.cluster_eps.offset, S.cluster_rejects.offset, S.cluster_left.offset]
    assert [f for f, _ in S._fields_][-4:] == ["device_bytes", "cluster_eps", "cluster_rejects", "cluster_left"]


def test_the_plan_runs_clean_under_the_host_sanitizers(tmp_path):
    """the same file with its own main, built with -fsanitize=address,undefined, run once: host code, no library, no device"""
    exe = tmp_path / "prior_cluster_plan_main"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-DPCP_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "prior_cluster_plan ok" in out.stdout, out.stdout + out.stderr

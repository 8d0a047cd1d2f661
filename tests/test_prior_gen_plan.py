"""The host half of hcmvs_generate_plane_prior_device (hc-mvs_amd/csrc/prior_gen_plan.h) on the CPU: every refusal, Kinv against numpy, the
level table, min_points, the stop rule, the decoding of the fixed-point sums, frame and quad bit for bit against the numpy statement of the
rule (tests/plane_prior_ref.py), the scratch layout, and what the inlier clustering adds: the refusals of
cluster_mul, the cell edge against numpy (a product that underflows to 0 included), the cap, the sizes and offsets of the two structs
against the binding, and the arrays it borrows from the layout during S4.  tests/prior_gen_plan_shim.cpp is compiled with g++ alone, with -ffp-contract=off as
the library is: no HIP, no library; the same file is also built as a stand-alone program under the address and undefined-behaviour
sanitizers and run once."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import plane_prior_ref as ref

binding = importlib.import_module("hc-mvs_amd.binding")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hc-mvs_amd", "csrc")
SRC = os.path.join(HERE, "prior_gen_plan_shim.cpp")
HDRS = [os.path.join(CSRC, h) for h in ("prior_gen_plan.h", "knn_layout.h", "carve.h")] + [os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libprior_gen_plan_shim.so")
U64, I32, F32, F64 = C.c_uint64, C.c_int32, C.c_float, C.c_double
K0 = np.array([[90.0, 0, 47.5], [0, 90.0, 39.5], [0, 0, 1]])
PX = 96 * 80


def stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [SRC] + HDRS)


@pytest.fixture(scope="module")
def lib():
    if stale(LIB_PATH):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    dp, fp = C.POINTER(F64), C.POINTER(F32)
    L.pgp_check.argtypes = [C.POINTER(U64), C.c_int, C.c_int, dp, C.POINTER(binding.PlanePriorParams), C.c_char_p, C.c_int]
    L.pgp_kinv.argtypes = [dp, dp]
    L.pgp_ray.argtypes = [dp, C.c_int, C.c_int, fp]; L.pgp_ray.restype = None
    L.pgp_levels.argtypes = [C.c_int, C.c_int, C.POINTER(I32)]
    L.pgp_min_points.argtypes = [C.c_ulonglong, F32]; L.pgp_min_points.restype = C.c_longlong
    L.pgp_fail_limit.argtypes = [F32, C.c_longlong, C.c_ulonglong, C.c_int]
    L.pgp_eps.argtypes = [F64, F32]; L.pgp_eps.restype = F32
    L.pgp_mean.argtypes = [C.c_longlong, C.c_ulonglong, C.c_ulonglong, C.c_int]; L.pgp_mean.restype = F64
    L.pgp_frame.argtypes = [fp, dp, dp]; L.pgp_frame.restype = None
    L.pgp_quad.argtypes = [dp, dp, dp, dp, dp, C.POINTER(I32), dp]
    L.pgp_layout.argtypes = [C.c_ulonglong] * 3 + [C.POINTER(C.c_ulonglong)]
    L.pgp_cell.argtypes = [F64, F32]; L.pgp_cell.restype = F32
    L.pgp_cell_usable.argtypes = [F32]
    L.pgp_cluster_scratch.argtypes = [C.c_ulonglong] * 4 + [C.POINTER(C.c_ulonglong)]
    L.pgp_live_in_s4.argtypes = [C.c_ulonglong] * 3 + [C.POINTER(C.c_ulonglong)]
    L.pgp_constants.argtypes = [C.POINTER(C.c_longlong)]; L.pgp_constants.restype = None
    return L


def dptr(a):
    return a.ctypes.data_as(C.POINTER(F64))


def params(**kw):
    p = binding.PlanePriorParams(255, 0.18, 0.3, 10, 0.01, 80.0, 2.0, 0.25, 256, 1)  # the documented defaults, without the library: cluster_mul is 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def check(lib, addr=None, w=96, h=80, K=K0, p=None, null_K=False, null_p=False):
    base = 0x100000
    a = dict(depth=base, normal=base + PX * 4, conf=base + PX * 16, prior=base + PX * 20, pn=base + PX * 24)
    a.update(addr or {})
    arr = (U64 * 5)(a["depth"], a["normal"], a["conf"], a["prior"], a["pn"])
    Kc = np.ascontiguousarray(K, np.float64)
    buf = C.create_string_buffer(256)
    pp = p if p is not None else params()
    n = lib.pgp_check(arr, w, h, None if null_K else dptr(Kc), None if null_p else C.byref(pp), buf, 256)
    assert n == len(buf.value)
    return buf.value.decode()


def constants(lib):
    k = (C.c_longlong * 15)()
    lib.pgp_constants(k)
    return list(k)


def test_constants_and_struct_sizes(lib):
    k = constants(lib)
    assert list(k[:6]) == [ref.M, 16, 4096, ref.SPACING_SHIFT, ref.COORD_SHIFT, ref.MAX_PLANES] and ref.MAX_PLANES == binding.MAX_PRIOR_PLANES
    assert k[6] % 8 == 0 and k[7] == C.sizeof(binding.PriorPlane) and k[8] == C.sizeof(binding.PlanePriorParams) and k[9] == C.sizeof(binding.PlanePriorStats)


def test_a_good_call_passes(lib):
    assert check(lib) == ""
    assert check(lib, dict(pn=0)) == ""          # the prior normal map is optional


def test_every_refusal(lib):
    for k in ("depth", "normal", "conf", "prior"):
        assert "null" in check(lib, {k: 0})
    assert "null" in check(lib, null_K=True) and "null" in check(lib, null_p=True)
    assert "size" in check(lib, w=0) and "size" in check(lib, h=-3) and "size" in check(lib, w=1 << 15, h=1 << 14)
    for K in (np.array([[90.0, 0, 47.5], [0, 90, 39.5], [0, 1e-9, 1]]), np.array([[90.0, 0, 47.5], [0, 90, 39.5], [0, 0, 2]]),
              np.array([[90.0, 0, 47.5], [0, 0, 39.5], [0, 0, 1]]), np.array([[np.nan, 0, 47.5], [0, 90, 39.5], [0, 0, 1]]),
              np.array([[1.0, 2, 3], [2, 4, 5], [0, 0, 1]])):
        assert "K" in check(lib, K=K)
    for v in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert "probability" in check(lib, p=params(probability=v))
    for v in (0.0, -1.0, float("inf"), float("nan")):
        assert "min_points_div" in check(lib, p=params(min_points_div=v))
        assert "epsilon_mul" in check(lib, p=params(epsilon_mul=v))
    for v in (2, 32, -1):
        assert "n_neighbors" in check(lib, p=params(n_neighbors=v))
    assert check(lib, p=params(n_neighbors=3)) == "" and check(lib, p=params(n_neighbors=31)) == ""
    for v in (0, -1, 4097):
        assert "max_rounds" in check(lib, p=params(max_rounds=v))
    assert check(lib, p=params(max_rounds=4096)) == ""
    for name in ("conf_max", "planarity_min", "normal_threshold"):
        assert "NaN" in check(lib, p=params(**{name: float("nan")}))
    base = 0x100000
    assert "prior map overlaps the depth" in check(lib, dict(prior=base + 4 * (PX - 1)))
    assert "prior map overlaps the normal" in check(lib, dict(prior=base + PX * 4 - 4 + 4, pn=0))
    assert "prior map overlaps the conf" in check(lib, dict(prior=base + PX * 16 - 4 * PX + 4, normal=base + PX * 100))
    assert "prior normal map overlaps the depth" in check(lib, dict(pn=base - 12 * PX + 4))
    assert "prior normal map overlaps the prior map" in check(lib, dict(pn=base + PX * 20 + 4 * PX - 4))
    assert check(lib, dict(pn=base + PX * 24)) == "" and check(lib, dict(prior=base - 4 * PX)) == ""  # touching is not overlapping


def test_kinv_and_rays_against_numpy(lib):
    rng = np.random.RandomState(3)
    for K in (K0, np.array([[1234.5, 0.7, 959.5], [0, 1230.25, 539.5], [0, 0, 1]]), np.array([[800.0, -3.0, 310.0], [1.5, 790.0, 255.0], [0, 0, 1]])):
        inv = np.zeros(6)
        assert lib.pgp_kinv(dptr(np.ascontiguousarray(K)), dptr(inv)) == 1
        want = np.linalg.inv(K)
        assert np.allclose(inv.reshape(2, 3), want[:2], rtol=1e-12, atol=1e-15) and np.allclose(want[2], [0, 0, 1], atol=1e-15)
        assert np.array_equal(inv, ref.kinv(K))
        w, h = 64, 48
        r = ref.rays(K, w, h)
        for x, y in zip(rng.randint(0, w, 50), rng.randint(0, h, 50)):
            got = np.zeros(3, np.float32)
            lib.pgp_ray(dptr(inv), int(x), int(y), got.ctypes.data_as(C.POINTER(F32)))
            assert np.array_equal(got, r[y, x])
            assert np.allclose(K @ got.astype(np.float64), [x, y, 1], rtol=1e-5, atol=1e-3)


def test_level_table(lib):
    lv = (I32 * 16)()
    assert lib.pgp_levels(96, 80, lv) == 5 and list(lv[:5]) == [2, 4, 8, 16, 32] == ref.levels(96, 80)
    assert lib.pgp_levels(1920, 1080, lv) == 9 and list(lv[:9]) == [2, 4, 8, 16, 32, 64, 128, 256, 512] == ref.levels(1920, 1080)
    assert lib.pgp_levels(80, 96, lv) == 5 and lib.pgp_levels(3, 3, lv) == 1 and lv[0] == 2 and lib.pgp_levels(8, 4, lv) == 2
    assert lib.pgp_levels(32768, 32768, lv) == 14 and lv[13] == 16384


def test_min_points_and_stop_rule(lib):
    for n0, div in ((4597, 80.0), (7003, 80.0), (100, 80.0), (239, 80.0), (240, 80.0), (11, 0.5), (1000, 3.0)):
        assert lib.pgp_min_points(n0, div) == ref.min_points(n0, div) == max(3, int(n0 // div))
    # the defaults: 0.01 and 1 / 80 -- a few hundred candidates, two rounds of 256
    for n0 in (800, 4597, 80000, 2000000):
        m = ref.min_points(n0, 80.0)
        assert lib.pgp_fail_limit(0.01, m, n0, 256) == 2 == ref.fail_limit(0.01, m, n0, 256)
    assert lib.pgp_fail_limit(0.01, 10, 100, 256) == 1 and lib.pgp_fail_limit(0.01, 3, 10 ** 6, 256) == 256   # capped by max_rounds
    assert lib.pgp_fail_limit(0.01, 3, 10 ** 5, 4096) == ref.fail_limit(0.01, 3, 10 ** 5, 4096) == int(np.ceil(np.ceil(np.log(np.float32(0.01)) / np.log(1 - 3e-5)) / 256))
    assert lib.pgp_fail_limit(0.01, 50, 40, 256) == 1 == ref.fail_limit(0.01, 50, 40, 256)                     # min_points above n0
    assert lib.pgp_eps(0.0921947, 2.0) == np.float32(0.0921947 * 2.0)


def test_fixed_point_means(lib):
    rng = np.random.RandomState(11)
    for shift, limit, vals in ((40, 8388608.0, rng.uniform(0, 0.3, 5000)), (32, 1073741824.0, rng.normal(0, 40, 5000)), (32, 1073741824.0, np.array([-3.25, 1e12, -1e12])),
                               (40, 8388608.0, np.array([1e9, 0.5]))):
        v = np.where(vals < limit, np.where(vals > -limit, vals, -(limit - 1.0)), limit - 1.0)
        q = np.rint(v * 2.0 ** shift).astype(np.int64)
        hi, lo = int((q >> 32).sum()), int((q & 0xffffffff).sum())
        got = lib.pgp_mean(hi, lo, len(vals), shift)
        assert got == ref.fixed_mean(vals, len(vals), shift, limit)
        assert abs(got - v.mean()) <= 2.0 ** -shift + 1e-12 * abs(v).max()
    # the order of the addends is immaterial by construction: integers


def test_frame_and_quad_equal_the_numpy_statement(lib):
    rng = np.random.RandomState(7)
    K = np.ascontiguousarray(np.array([[90.0, 0.3, 47.5], [0, 88.0, 39.5], [0, 0, 1]]))
    fallbacks = 0
    normals = [np.array(v, np.float32) for v in ([0, 0, 1], [1, 0, 0], [0, -1, 0], [0.5, 0.5, np.sqrt(0.5)], [0.5, -0.5, np.sqrt(0.5)])]
    for i in range(200):
        n = normals[i] if i < len(normals) else rng.normal(size=3)
        n = (n / np.linalg.norm(n)).astype(np.float32)
        b1, b2 = np.zeros(3), np.zeros(3)
        lib.pgp_frame(n.ctypes.data_as(C.POINTER(F32)), dptr(b1), dptr(b2))
        e1, e2 = ref.frame(n)
        assert np.array_equal(b1, e1) and np.array_equal(b2, e2)
        n64 = n.astype(np.float64)
        assert abs(b1 @ n64) < 1e-7 and abs(b2 @ n64) < 1e-7 and abs(b1 @ b2) < 1e-7 and abs(np.linalg.norm(b1) - 1) < 1e-12
        c = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 6)])
        ext = rng.uniform(0.1, 8.0 if i % 2 else 1.0, 4)
        uv = np.array([-ext[0], ext[1], -ext[2], ext[3]])
        box = np.array([3, 40, 5, 60], np.int32)
        q = np.zeros(8)
        fb = lib.pgp_quad(dptr(K), dptr(c), dptr(b1), dptr(b2), dptr(uv), box.ctypes.data_as(C.POINTER(I32)), dptr(q))
        eq, efb = ref.quad(K, c, e1, e2, uv, box)
        assert fb == efb and np.array_equal(q.reshape(4, 2), eq)
        fallbacks += fb
        if fb:
            assert np.array_equal(q, [2.5, 4.5, 40.5, 4.5, 40.5, 60.5, 2.5, 60.5])
    assert 10 < fallbacks < 190          # both branches are walked


def test_scratch_layout_is_monotone_and_aligned(lib):
    out = (C.c_ulonglong * 40)()
    for px, scan, sort in ((PX, 1000, 3000), (1920 * 1080, 70000, 9000000), (16 * 16, 1, 1), (160 * 120, 0, 0)):
        n = lib.pgp_layout(px, scan, sort, out)
        v = list(out[:n])
        assert n == 29 and v[0] == 0 and all(x % 256 == 0 for x in v)
        steps = [b - a for a, b in zip(v, v[1:])]
        assert all(s >= 0 for s in steps) and all(s > 0 for i, s in enumerate(steps) if not (scan == 0 and i == 2) and not (sort == 0 and i == 27))
        # the pieces hold what the kernels index: flags and scan px + 1 words, the sets 12 + 12 + 4 bytes a sample, the frames of 64 planes
        assert steps[0] >= (px + 1) * 4 and steps[1] >= (px + 1) * 4 and steps[2] >= scan and steps[3] >= 12 * px and steps[5] >= 4 * px
        assert steps[9] >= max(8 * px, 64 * 72) and steps[12] >= px and steps[13] >= 256 * 16 and steps[14] >= 256 * 16 and steps[15] >= 48
        assert steps[16] >= 64 * 16 * 8 and steps[17] >= 64 * k_plane_dev(lib) and steps[19] >= 64 and steps[24] >= 16 * px and steps[27] >= sort
    assert v[-1] < 160 * 120 * 200


def k_plane_dev(lib):
    return constants(lib)[6]


def test_cluster_mul_is_refused_unless_finite_and_not_negative(lib):
    assert params().cluster_mul == 0.0 and check(lib) == ""
    for v in (0.0, 1e-45, 2.0, 7.0, 10.0, 3e38):
        assert check(lib, p=params(cluster_mul=v)) == ""
    for v in (-1.0, -1e-45, float("nan"), float("inf"), float("-inf")):
        assert "cluster_mul" in check(lib, p=params(cluster_mul=v)), v
    assert "probability" in check(lib, p=params(cluster_mul=-1.0, probability=0.0))          # the earlier refusals keep their order


def test_the_cell_edge_against_numpy(lib):
    rng = np.random.RandomState(5)
    for avg, mul in list(zip(rng.uniform(1e-3, 0.5, 200), rng.uniform(0.1, 20, 200))) + [(0.0921947, 7.0), (0.05, 1e-45), (0.4, 1e-45), (1e30, 1e30), (1e-300, 2.0), (0.07, 1e-9)]:
        got = lib.pgp_cell(avg, mul)
        with np.errstate(all="ignore"):
            want = np.float32(np.float64(avg) * np.float64(np.float32(mul)))
        assert np.float32(got).tobytes() == want.tobytes(), (avg, mul)
        assert float(np.float32(got)) == ref.cluster_cell(avg, mul)
        assert lib.pgp_cell_usable(got) == int(want > 0 and np.isfinite(want))
    assert lib.pgp_cell(0.05, 1e-45) == 0.0 and lib.pgp_cell_usable(0.0) == 0        # the product underflowed: nothing is clustered
    assert np.isinf(lib.pgp_cell(1e30, 1e30)) and lib.pgp_cell_usable(float("inf")) == 0 and lib.pgp_cell_usable(float("nan")) == 0
    assert lib.pgp_cell_usable(-1.0) == 0 and lib.pgp_cell_usable(1e-45) == 1


def test_constants_and_struct_layout_against_the_binding(lib):
    k = constants(lib)
    assert k[10] == 1 << 30 == ref.CELL_CAP
    P, S = binding.PlanePriorParams, binding.PlanePriorStats
    assert k[8] == C.sizeof(P) and k[9] == C.sizeof(S)
    assert k[11] == P.cluster_mul.offset and P._fields_[-1][0] == "cluster_mul"           # the new last field
    assert [k[12], k[13], k[14]] == [S.cluster_eps.offset, S.cluster_rejects.offset, S.cluster_left.offset]
    assert [f for f, _ in S._fields_][-4:] == ["device_bytes", "cluster_eps", "cluster_rejects", "cluster_left"]


# pgp_layout's order, and pgp_cluster_scratch's
PIECES = ("flags", "scan", "scanTmp", "xyzA", "nrmA", "pixA", "xyzB", "nrmB", "pixB", "spacing", "sampleAt", "assigned", "stage", "cand", "counts", "winner", "acc", "planes",
          "words", "levels", "knn.keys", "knn.keys2", "knn.idx", "knn.idx2", "knn.sorted", "knn.pos", "knn.box", "knn.sort", "bytes")
CLUSTER_ARRAYS = ("keys", "keys2", "idx", "idx2", "cells", "start", "parent", "sizes", "marks", "scan", "scanTmp", "sortTmp", "rec")
LIVE_IN_S4 = ("xyzA", "nrmA", "pixA", "sampleAt", "assigned", "stage", "cand", "counts", "winner", "levels")


@pytest.mark.parametrize("px", [1, 255, 96 * 80, 1920 * 1080, 2 ** 29 - 1])
def test_the_cluster_scratch_stays_inside_idle_pieces(lib, px):
    """S4c at n0 = px, the most samples a call can have: every array ends inside the piece it borrows, no two overlap, none touches a
    piece S4 keeps live, and the offsets are the expressions generate_plane_prior_device had inline before the plan stated them"""
    out, cl, lv = (C.c_ulonglong * 40)(), (C.c_ulonglong * 26)(), (C.c_ulonglong * 16)()
    for scan, sort in ((0, 0), (1, 1), (1000, 3000), (70000, 9000000), (767, 4 * px + 12345)):
        assert lib.pgp_layout(px, scan, sort, out) == len(PIECES)
        lay = dict(zip(PIECES, out))
        after = dict(zip(PIECES, list(out)[1:]))                                  # where the next piece starts
        assert lib.pgp_cluster_scratch(px, scan, sort, px, cl) == len(CLUSTER_ARRAYS)
        got = {name: (cl[2 * i], cl[2 * i + 1]) for i, name in enumerate(CLUSTER_ARRAYS)}
        srt = lay["knn.sorted"]
        want = dict(keys=(lay["knn.keys"], px * 8), keys2=(lay["knn.keys2"], px * 8), idx=(lay["knn.idx"], px * 4), idx2=(lay["knn.idx2"], px * 4), cells=(srt, px * 8),
                    start=(lay["knn.pos"], px * 4), parent=(srt + px * 8, px * 4), sizes=(srt + px * 12, px * 4), marks=(lay["flags"], (px + 1) * 4),
                    scan=(lay["scan"], (px + 1) * 4), scanTmp=(lay["scanTmp"], scan), sortTmp=(lay["knn.sort"], sort), rec=(lay["words"], 128))
        assert got == want
        borrowed = dict(keys="knn.keys", keys2="knn.keys2", idx="knn.idx", idx2="knn.idx2", cells="knn.sorted", start="knn.pos", parent="knn.sorted", sizes="knn.sorted",
                        marks="flags", scan="scan", scanTmp="scanTmp", sortTmp="knn.sort", rec="words")
        for name, (off, size) in got.items():
            assert lay[borrowed[name]] <= off and off + size <= after[borrowed[name]], name
        spans = sorted(v for v in got.values() if v[1])
        assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        assert lib.pgp_live_in_s4(px, scan, sort, lv) == len(LIVE_IN_S4) and list(lv[:len(LIVE_IN_S4)]) == [lay[name] for name in LIVE_IN_S4]
        assert not set(LIVE_IN_S4) & set(borrowed.values())
        for name in LIVE_IN_S4:
            assert all(off + size <= lay[name] or after[name] <= off for off, size in got.values()), name
        # fewer samples need no more
        assert lib.pgp_cluster_scratch(px, scan, sort, px // 2, cl) == len(CLUSTER_ARRAYS)
        assert all(cl[2 * i] == got[name][0] and cl[2 * i + 1] <= got[name][1] for i, name in enumerate(CLUSTER_ARRAYS))


@pytest.fixture(scope="module")
def sanitizer_run(tmp_path_factory):
    """the same file with its own main, built with -fsanitize=address,undefined, run once: host code, no library, no device"""
    exe = tmp_path_factory.mktemp("pgp") / "prior_gen_plan_main"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-DPGP_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)


def test_the_plan_runs_clean_under_the_host_sanitizers(sanitizer_run):
    out = sanitizer_run
    assert out.returncode == 0 and "prior_gen_plan ok" in out.stdout, out.stdout + out.stderr


def test_the_cluster_entries_run_clean_under_the_host_sanitizers(sanitizer_run):
    """the one main walks the refusals of cluster_mul, the cell edge, the cap and the S4c scratch after the rest"""
    out = sanitizer_run
    assert out.returncode == 0 and "prior_cluster_plan ok" in out.stdout, out.stdout + out.stderr

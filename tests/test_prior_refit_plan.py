"""The refit of a round's winner as hc-mvs_amd/csrc/prior_gen_plan.h has it, on the CPU, against its statement
(tests/plane_prior_refit_ref.py): the solver bit for bit on every step of the golden cases and on degenerate covariances (diagonal, two equal
eigenvalues, rank 1, zeros), the scale E on both sides of a power of two, the decision sequence on records made from the statement, the
refusals of refit_iters, the sizes and offsets of the two structs against the binding, and the scratch: inside the layout, disjoint from what
the clustering borrows and from the pieces S4 keeps live.  tests/prior_refit_plan_shim.cpp is compiled with g++ alone with
-ffp-contract=off, as the library is; the same file is also built as a stand-alone program under the address and undefined-behaviour
sanitizers and run once."""
import ctypes as C
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

import plane_prior_ref as ref
import plane_prior_refit_ref as refit

binding = importlib.import_module("hc-mvs_amd.binding")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "hc-mvs_amd", "csrc")
SRC = os.path.join(HERE, "prior_refit_plan_shim.cpp")
HDRS = [os.path.join(CSRC, h) for h in ("prior_gen_plan.h", "knn_layout.h", "carve.h")] + [os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libprior_refit_plan_shim.so")
U64, I32, F32, F64 = C.c_uint64, C.c_int32, C.c_float, C.c_double
ULL = C.c_ulonglong
K0 = np.array([[90.0, 0, 47.5], [0, 90.0, 39.5], [0, 0, 1]])
PX = 96 * 80
WORDS = 24
STOP_CODES = dict(iters=0, band=1, degenerate=2, fixed=3, count=4)

with open(os.path.join(HERE, "golden", "plane_prior_refit_statement.json")) as f:
    GOLDEN = json.load(f)


def stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in [SRC] + HDRS)


@pytest.fixture(scope="module")
def lib():
    if stale(LIB_PATH):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    dp, fp, up, ip = C.POINTER(F64), C.POINTER(F32), C.POINTER(ULL), C.POINTER(I32)
    L.prp_check.argtypes = [C.POINTER(U64), C.c_int, C.c_int, dp, C.POINTER(binding.PlanePriorParams), C.c_char_p, C.c_int]
    L.prp_scale.argtypes = [F32]
    L.prp_eigvec.argtypes = [dp, dp]
    L.prp_cov.argtypes = [up, ULL, dp, dp]; L.prp_cov.restype = None
    L.prp_solve.argtypes = [up, ULL, dp, C.c_int, fp, fp]
    L.prp_round.argtypes = [C.c_int, C.c_longlong, dp, C.c_int, fp, ip, up, C.c_int, ip, fp, fp]; L.prp_round.restype = None
    L.prp_scratch.argtypes = [ULL] * 4 + [up, up, up]
    L.prp_constants.argtypes = [C.POINTER(C.c_longlong)]; L.prp_constants.restype = None
    return L


def dptr(a):
    return a.ctypes.data_as(C.POINTER(F64))


def words_of(sums):
    """the 18 words of nine integer sums, as the device returns them (two's complement for a negative high part)"""
    out = (ULL * 18)()
    for i, t in enumerate(sums):
        hi, lo = refit.split_words(int(t))
        out[2 * i] = hi & ref.MASK; out[2 * i + 1] = lo
    return out


def solve(lib, sums, m, O, E, prev):
    out = np.zeros(4, np.float32)
    O = np.array(O, np.float64); prev = np.array(prev, np.float32)
    ok = lib.prp_solve(words_of(sums), m, dptr(O), E, prev.ctypes.data_as(C.POINTER(F32)), out.ctypes.data_as(C.POINTER(F32)))
    return out if ok else None


def eigvec(lib, Cm):
    Cm = np.array(Cm, np.float64); v = np.zeros(3)
    sweeps = lib.prp_eigvec(dptr(Cm), dptr(v))
    return v, sweeps


def unhex(v):
    return [float.fromhex(x) for x in v]


def test_the_solver_equals_the_statement_on_every_step_of_the_golden_cases(lib):
    steps = [s for r in GOLDEN for s in r["steps"]]
    assert len(steps) > 60 and {s["E"] for s in steps} >= {-2, -20}
    for s in steps:
        O, prev = unhex(s["O"]), np.array(unhex(s["prev"]), np.float32)
        want = refit.refit_solve(s["sums"], s["m"], O, s["E"], prev)
        got = solve(lib, s["sums"], s["m"], O, s["E"], prev)
        assert got is not None and got.tobytes() == np.array(want, np.float32).tobytes() == np.array(unhex(s["plane"]), np.float32).tobytes()
        # and the pieces: the mean, the covariance and the eigenvector, as doubles
        mu, Cm = np.zeros(3), np.zeros(6)
        lib.prp_cov(words_of(s["sums"]), s["m"], dptr(mu), dptr(Cm))
        emu, eC = refit.covariance(s["sums"], s["m"])
        assert mu.tolist() == emu and Cm.tolist() == eC
        v, sweeps = eigvec(lib, Cm)
        ev, esweeps = refit.jacobi_smallest(eC)
        assert v.tolist() == ev and sweeps == esweeps and 1 <= sweeps <= 16
        # the statement's solver agrees with numpy's: the same direction up to rounding, and the smallest eigenvalue
        w, V = np.linalg.eigh(np.array([[eC[0], eC[1], eC[2]], [eC[1], eC[3], eC[4]], [eC[2], eC[4], eC[5]]]))
        if w[1] - w[0] > 1e-6 * w[2]:
            assert abs(abs(V[:, 0] @ v) - 1) < 1e-9


DEGENERATE = [
    ("diagonal", [3.0, 0, 0, 1.0, 0, 2.0], [0, 1, 0], 0),
    ("diagonal, a tie: the lowest index", [1.0, 0, 0, 1.0, 0, 2.0], [1, 0, 0], 0),
    ("zeros", [0.0] * 6, [1, 0, 0], 0),
    ("two equal eigenvalues", [2.0, 0, 0, 2.0, 0, 0.5], [0, 0, 1], 0),
    ("two equal eigenvalues, rotated", [1.25, 0.75, 0, 1.25, 0, 2.0], None, None),
    ("rank 1", [1.0, 2.0, 3.0, 4.0, 6.0, 9.0], None, None),
    ("rank 1, negative entries", [4.0, -2.0, 0.0, 1.0, 0.0, 0.0], None, None),
    ("a tiny off-diagonal: theta overflows", [1.0, 1e-320, 0, 2.0, 0, 3.0], None, None),
    ("huge entries", [1e300, 5e299, -2e299, 3e300, 1e299, 2e300], None, None),
]


@pytest.mark.parametrize("what,Cm,vec,sweeps", DEGENERATE, ids=[d[0] for d in DEGENERATE])
def test_the_eigenvector_of_degenerate_matrices(lib, what, Cm, vec, sweeps):
    v, n = eigvec(lib, Cm)
    ev, en = refit.jacobi_smallest(Cm)
    assert v.tobytes() == np.array(ev).tobytes() and n == en
    if vec is not None:
        assert v.tolist() == vec and n == sweeps
    A = np.array([[Cm[0], Cm[1], Cm[2]], [Cm[1], Cm[3], Cm[4]], [Cm[2], Cm[4], Cm[5]]])
    scale = np.abs(A).max() or 1.0
    lam = v @ (A / scale) @ v
    assert np.isfinite(v).all() and abs(np.linalg.norm(v) - 1) < 1e-12 and np.abs((A / scale) @ v - lam * v).max() < 1e-12       # an eigenvector
    assert lam <= np.linalg.eigvalsh(A / scale)[0] + 1e-12                                                                     # of the smallest eigenvalue


def test_random_covariances_equal_the_statement(lib):
    rng = np.random.RandomState(4)
    for i in range(300):
        B = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-6, 3)
        A = B @ B.T
        if i % 3 == 0:
            A[2] *= 1e-9; A[:, 2] *= 1e-9          # a thin band
        Cm = [A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]]
        v, n = eigvec(lib, Cm)
        ev, en = refit.jacobi_smallest(Cm)
        assert v.tobytes() == np.array(ev).tobytes() and n == en


def test_a_degenerate_solution_is_refused(lib):
    zero = [0] * 9
    prev = [0.0, 0.0, 1.0, 1.0]
    # zeros: the eigenvector is (1, 0, 0), a plane through the anchor
    got = solve(lib, zero, 5, [1.0, 2.0, 3.0], 0, prev)
    assert got.tolist() == [1.0, 0.0, 0.0, 1.0] and refit.refit_solve(zero, 5, [1.0, 2.0, 3.0], 0, prev) == (1.0, 0.0, 0.0, 1.0)
    # an anchor whose offset is not finite in float32
    assert solve(lib, zero, 5, [1e39, 0.0, 0.0], 0, prev) is None and refit.refit_solve(zero, 5, [1e39, 0.0, 0.0], 0, prev) is None
    # the normal turns to the side of the previous one
    got = solve(lib, zero, 5, [1.0, 2.0, 3.0], 0, [-1.0, 0.0, 0.0, 0.0])
    assert got.tolist() == [-1.0, -0.0, -0.0, -1.0] and got.tobytes() == np.array(refit.refit_solve(zero, 5, [1.0, 2.0, 3.0], 0, [-1.0, 0.0, 0.0, 0.0]), np.float32).tobytes()


def test_the_scale_on_both_sides_of_a_power_of_two(lib):
    for eps, E in ((0.25, -1), (np.nextafter(np.float32(0.25), np.float32(0)), -2), (np.nextafter(np.float32(0.25), np.float32(1)), -1), (1.0, 1), (0.99999994, 0), (0.5, 0),
                   (0.18438941, -2), (8.745256e-07, -20), (3e38, 128), (1e-45, -148), (0.0, 0), (-1.0, 0), (float("inf"), 0), (float("nan"), 0)):
        assert lib.prp_scale(eps) == E == refit.refit_scale(eps), eps
        if E and np.isfinite(eps):
            assert 0.5 <= float(np.float32(eps)) * 2.0 ** -E < 1.0


def run_round(lib, R, minp, O, E, winner, counts, recs):
    """prp_round on the records (counts, nine sums): (solved, kept, stop, records read, cnt_0 .. cnt_3), the final plane, the planes asked for"""
    flat = (ULL * (WORDS * len(recs)))()
    for i, (cnt, sums) in enumerate(recs):
        flat[WORDS * i:WORDS * i + 4] = cnt
        flat[WORDS * i + 4:WORDS * i + 22] = list(words_of(sums))
    out = (I32 * 8)(); plane = np.zeros(4, np.float32); asked = np.zeros((len(recs) + 1, 4), np.float32)
    O = np.array(O, np.float64); winner = np.array(winner, np.float32); counts = (I32 * 4)(*[int(v) for v in counts])
    fp = C.POINTER(F32)
    lib.prp_round(R, minp, dptr(O), E, winner.ctypes.data_as(fp), counts, flat, len(recs), out, plane.ctypes.data_as(fp), asked.ctypes.data_as(fp))
    return list(out), plane, asked


# the first round of these golden calls ends for these reasons (in the first round every sample is free and the winner is that of the call
# without steps, so the records a launch would return can be made from the fitting set alone)
REPLAYED = ((1, "iters"), (9, "fixed"), (19, "count"), (18, "fixed"), (0, "iters"))


@pytest.mark.parametrize("index,stop", REPLAYED)
def test_the_decision_sequence_equals_the_statement(lib, index, stop):
    """the header is walked launch by launch: the record of every plane it asks for -- the four counts and the band's nine sums -- is made
    from the statement's fitting set, and it must end where the statement ends, at most refit_iters + 1 launches later"""
    import test_plane_prior_ref as TR
    rec = GOLDEN[index]
    p = dict(rec["params"])
    c, state = TR.stages(rec["case"])
    res = refit.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **p)
    base = refit.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **dict(p, refit_iters=0))
    assert res["refit_stops"][0] == stop and np.array_equal(base["rounds"][0], res["rounds"][0])
    pix, P, N = state["fit"]
    thr, eps = np.float32(ref.DEFAULTS["normal_threshold"]), res["stats"]["eps"]
    bands = [eps, eps * np.float32(0.5), eps * np.float32(0.25), eps * np.float32(0.125)]
    E = refit.refit_scale(eps)
    rnd, winner = res["rounds"][0], base["refit_planes"][0]
    ia = ref.draw_below(ref.mix64((p["seed"] & ref.MASK) ^ ref.mix64(int(rnd[0]))), 0, len(pix))
    O = [float(v) for v in P[ia]]

    def record(pl):
        with np.errstate(invalid="ignore"):
            facing = np.abs(ref.dot3(pl[0], pl[1], pl[2], N[:, 0], N[:, 1], N[:, 2])) >= thr
            dist = np.abs(ref.dot3(pl[0], pl[1], pl[2], P[:, 0], P[:, 1], P[:, 2]) - pl[3])
            return [int((facing & (dist <= e)).sum()) for e in bands], refit.moment_sums(P[facing & (dist <= bands[2])], O, E)

    recs, launch = [], winner
    while True:
        recs.append(record(launch))
        out, plane, asked = run_round(lib, p["refit_iters"], res["stats"]["min_points"], O, E, winner, rnd[1:5], recs)
        assert out[3] == len(recs) and np.array_equal(asked[0], winner)
        if out[2] >= 0:
            break
        launch = asked[len(recs)]
    assert len(recs) <= p["refit_iters"] + 1
    assert out[:2] == res["refits"][0, :2].tolist() and out[2] == STOP_CODES[stop] and out[4:] == res["refits"][0, 2:].tolist()
    assert plane.tobytes() == res["refit_planes"][0].tobytes()


def test_a_band_of_fewer_than_three_samples_ends_the_steps(lib):
    winner, zero = [0.0, 0.0, 1.0, 1.0], [0] * 9
    out, plane, _ = run_round(lib, 4, 3, [0.0, 0.0, 1.0], 0, winner, [9, 5, 2, 1], [([9, 5, 2, 1], zero)])
    assert out[:4] == [0, 0, STOP_CODES["band"], 1] and out[4:] == [9, 5, 2, 1] and plane.tolist() == winner
    out, plane, _ = run_round(lib, 4, 3, [0.0, 0.0, 1.0], 0, winner, [9, 5, 3, 1], [([9, 5, 3, 1], zero)])
    assert out[:4] == [1, 0, -1, 1]                      # three samples are a band: a step is solved, its plane waits for its counts


def test_refit_iters_is_refused_outside_its_range(lib):
    def check(**kw):
        p = binding.PlanePriorParams(255, 0.18, 0.3, 10, 0.01, 80.0, 2.0, 0.25, 256, 1)
        for k, v in kw.items():
            setattr(p, k, v)
        base = 0x100000
        arr = (U64 * 5)(base, base + PX * 4, base + PX * 16, base + PX * 20, base + PX * 24)
        buf = C.create_string_buffer(256)
        n = lib.prp_check(arr, 96, 80, dptr(np.ascontiguousarray(K0)), C.byref(p), buf, 256)
        assert n == len(buf.value)
        return buf.value.decode()

    assert binding.PlanePriorParams(255, 0.18, 0.3, 10, 0.01, 80.0, 2.0, 0.25, 256, 1).refit_iters == 0 and check() == ""
    for v in range(0, 17):
        assert check(refit_iters=v) == ""
    for v in (-1, 17, 100, -2 ** 31, 2 ** 31 - 1):
        assert "refit_iters" in check(refit_iters=v), v
    assert "cluster_mul" in check(refit_iters=17, cluster_mul=-1.0)          # the earlier refusals keep their order
    assert refit.MAX_REFIT_ITERS == 16


def test_constants_and_struct_layout_against_the_binding(lib):
    """refit_iters is appended to the C struct into its tail padding (the size stays) and the binding reaches it as a property over those
    bytes; the refit's counters are a struct of their own, so hcmvs_plane_prior_stats keeps its size and its last field"""
    k = (C.c_longlong * 10)()
    lib.prp_constants(k)
    P, S, R = binding.PlanePriorParams, binding.PlanePriorStats, binding.PlanePriorRefitStats
    assert list(k[:4]) == [refit.MAX_REFIT_ITERS, refit.FIRST_SHIFT, refit.SECOND_SHIFT, WORDS]
    assert k[4] == C.sizeof(P) and k[5] == C.sizeof(S)
    assert k[6] == P.REFIT_ITERS_OFFSET == P.cluster_mul.offset + C.sizeof(C.c_float) and k[6] + 4 == C.sizeof(P)
    assert k[7] == C.sizeof(R) and [k[8], k[9]] == [R.refit_rounds.offset, R.refit_steps.offset]
    lib.prp_read_refit_iters.argtypes = [C.POINTER(P)]
    for v in (0, 1, 16, -1, 2 ** 31 - 1):
        p = P(255, 0.18, 0.3, 10, 0.01, 80.0, 2.0, 0.25, 256, 1, 7.0)
        assert p.refit_iters == 0 and lib.prp_read_refit_iters(C.byref(p)) == 0
        p.refit_iters = v
        assert p.refit_iters == v == lib.prp_read_refit_iters(C.byref(p)) and p.cluster_mul == 7.0 and p.seed == 1       # C reads what the property wrote, and nothing else moved
        q = P.from_buffer_copy(p)
        assert q.refit_iters == v                                                                                      # a copy of the struct carries it


@pytest.mark.parametrize("px", [1, 255, 96 * 80, 1920 * 1080, 2 ** 29 - 1])
def test_the_refit_scratch_stays_inside_an_idle_piece(lib, px):
    pairs, live, lay = (ULL * 28)(), (ULL * 32)(), (ULL * 4)()
    for scan, sort in ((0, 0), (1000, 3000), (70000, 9000000), (767, 4 * px + 12345)):
        assert lib.prp_scratch(px, scan, sort, px, pairs, live, lay) == 14
        rec = (pairs[0], pairs[1])
        acc, planes, total, n_live = lay[0], lay[1], lay[2], lay[3]
        assert rec == (acc, WORDS * 8) and acc + WORDS * 8 <= planes <= total          # inside `acc`, which S5 initialises before it reads it
        assert n_live == 10
        for i in range(1, 14):                                                       # disjoint from what S4c borrows
            off, size = pairs[2 * i], pairs[2 * i + 1]
            assert off + size <= rec[0] or rec[0] + rec[1] <= off, i
        for i in range(n_live):                                                      # and from the pieces S4 keeps live
            assert live[2 * i + 1] <= rec[0] or rec[0] + rec[1] <= live[2 * i], i


@pytest.fixture(scope="module")
def sanitizer_run(tmp_path_factory):
    """the same file with its own main, built with -fsanitize=address,undefined, run once: host code, no library, no device"""
    exe = tmp_path_factory.mktemp("prp") / "prior_refit_plan_main"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-DPRP_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)


def test_the_refit_entries_run_clean_under_the_host_sanitizers(sanitizer_run):
    out = sanitizer_run
    assert out.returncode == 0 and "prior_refit_plan ok" in out.stdout, out.stdout + out.stderr

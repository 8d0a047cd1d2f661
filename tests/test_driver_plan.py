"""The host-side plan of a DensifyPointCloud run (hc-mvs_amd/host/driver_plan.h, and working_size of host/scene_io.h) on the CPU: the option
table, the view selection, how the images are dealt to the devices, the memory budget, the batches, the schedule of the outer iterations
and the size of the cloud's buffers.  tests/driver_plan_shim.cpp is compiled with g++ alone: no HIP, no library, no device.

The expected values are a Python transcription of the statements the driver's main() had before the plan existed (cited as "main:" with
what the statement did), never a call into the code under test; the view selection is compared with oracle/select_views.py."""
import ctypes as C
import importlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "driver_plan_shim.cpp")
HOST = os.path.join(ROOT, "hc-mvs_amd", "host")
HDRS = [os.path.join(HOST, "driver_plan.h"), os.path.join(HOST, "scene_io.h"), os.path.join(ROOT, "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libdriver_plan_shim.so")
U64 = C.c_ulonglong
U32 = C.c_uint32
GIB = 1 << 30
OK, USAGE, ERROR = 0, 1, 2   # ParseResult

# main: kKnown, the option table
KNOWN = ["-i", "--input-file", "-o", "--output-file", "-w", "--working-folder", "-c", "--config-file", "--dense-config-file", "--archive-type",
         "--process-priority", "--max-threads", "-v", "--verbosity", "--resolution-level", "--max-resolution", "--min-resolution",
         "--number-views", "--number-views-fuse", "--ignore-mask-label", "--use-semantic", "--estimate-colors", "--estimate-normals",
         "--sample-mesh", "--filter-point-cloud", "--fusion-mode", "--depthweight", "--normalweight", "--semantic-multiplier",
         "--sigma-texture", "--sigma-prior", "--ransac-epsilon", "--n-nOptimize", "--ransac-cluster", "--ransac-min-points",
         "--project-labels", "--ransac-probability", "--n-EstimationIters", "--n-EstimationIters-external", "--n-photo2geo",
         "--n-txthreshold", "--n-maxgeo_proportion", "--n-para_part", "--n-para_part2", "--n-txthreshold2", "--n-para_tapa",
         "--n-para_tapa2", "--n-para_prior", "--n-para_prior2", "--n-photometric_flow", "--n-usepartconsistency",
         "--n-usegeoconsistency", "--n-initTriangulate", "--n-viewspread", "--n-opticalflow", "--n-adapthalfwin",
         "--n-propagatehalfwin", "--n-propagatestep",
         "--min-views-trust-point", "--fuse-order", "--fuse-count", "--device", "--devices", "--batch", "--seed", "--restore-hypothesis", "--n-postfilter",
         "--n-postfilter-interleave", "--resume", "--n-filter"]

# the initialisers of struct Options as main() had them; postFilter -1 is resolved from --n-nOptimize 2 to 1 by the parse
DEFAULTS = dict(ignoreMaskLabel="", resolutionLevel=1, numberViews=5, numberViewsFuse=2, fusionMode=0, verbosity=2, estimationIters=1, estimationItersExternal=4,
                adaptHalfWin=5, propagateHalfWin=1, propagateStep=4, photometricFlow=0.5, depthweight=1.0, normalweight=1.0, initTriangulate=1, minViewsTrustPoint=2,
                fuseCount=-1, fuseOrder=0, estimateColors=2, estimateNormals=2, maxResolution=3200, minResolution=640, nOptimize=2, postFilter=1, viewspread=0,
                postFilterInterleave=0, nFilter=0, resume=1, restoreHypothesis=0, device=0, batch=32, devices=[0], seed=1234, thFilterPointCloud=0, sampleMesh=0.0,
                sampleSeed=1234, notes=[])


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    P = C.POINTER
    scene = [C.c_int, P(C.c_int), P(C.c_int), P(C.c_int), P(C.c_int), P(U32), P(C.c_int), P(U32)]
    L.dp_max_batch.restype = C.c_int
    L.dp_known_options.argtypes = [C.c_int, P(C.c_char_p)]
    L.dp_parse.argtypes = [C.c_int, P(C.c_char_p)]
    L.dp_parse.restype = C.c_char_p
    L.dp_iteration.argtypes = [C.c_int] * 7
    L.dp_deal.argtypes = scene + [P(U32), C.c_int, C.c_int, P(U32), P(C.c_int), P(C.c_int)]
    L.dp_deal.restype = None
    L.dp_registered_neighbors.argtypes = scene + [U32, P(U32), C.c_int, P(U32)]
    L.dp_budget.argtypes = scene + [P(U32), C.c_int, C.c_int, C.c_int, U64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(U64)]
    L.dp_budget.restype = None
    L.dp_batches.argtypes = scene + [C.c_int, P(C.c_int), P(U32), C.c_int]
    L.dp_batches.restype = C.c_char_p
    L.dp_cloud_worst_case.argtypes = scene + [P(U32), C.c_int, C.c_int, P(U64)]
    L.dp_cloud_worst_case.restype = None
    L.dp_fusion_counts_first.argtypes = [U64, U64, C.c_int]
    L.dp_budget_counts_first.argtypes = [U64, C.c_int]
    L.dp_budget_cloud_bytes.argtypes = [U64, C.c_int]
    L.dp_budget_cloud_bytes.restype = U64
    L.dp_working_size.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_uint, P(C.c_int), P(C.c_int)]
    L.dp_working_size.restype = None
    L.dp_select_views.argtypes = [C.c_int, C.c_int, C.c_int, P(C.c_double), P(C.c_double), P(C.c_double), C.c_int, C.c_int, C.c_int, P(C.c_float), P(C.c_int), P(U32),
                                  C.c_int, C.c_int]
    L.dp_select_views.restype = C.c_char_p
    return L


# ---- options ----------------------------------------------------------------------------------------------------------
INTS = set(k for k, v in DEFAULTS.items() if isinstance(v, int))
FLOATS = set(k for k, v in DEFAULTS.items() if isinstance(v, float))


def parse(lib, *args):
    argv = [b"DensifyPointCloud"] + [a.encode() for a in args]
    text = lib.dp_parse(len(argv), (C.c_char_p * len(argv))(*argv)).decode()
    o = dict(notes=[])
    for line in text.splitlines():
        k, v = line.split("=", 1)
        if k == "note":
            o["notes"].append(v)
        elif k == "devices":
            o[k] = [int(x) for x in v.split()]
        elif k in INTS or k in ("result", "nNotes"):
            o[k] = int(v)
        elif k in FLOATS:
            o[k] = float(v)
        else:
            o[k] = v
    assert o.pop("nNotes") == len(o["notes"])
    return o


def test_option_defaults(lib):
    o = parse(lib, "-i", "a/b/scene.mvs")
    assert o["result"] == OK and o["err"] == ""
    assert (o["input"], o["workdir"], o["output"]) == ("a/b/scene.mvs", "a/b", "a/b/scene_dense.mvs")     # main: dirname of the input; <input base>_dense.mvs
    for k, v in DEFAULTS.items():
        assert o[k] == v, k
    assert parse(lib, "-i", "scene.mvs")["workdir"] == "."


def test_option_forms_and_errors(lib):
    a = parse(lib, "--input-file=x.mvs", "--number-views=7", "-o", "out/y.mvs", "-w", "wd", "--depthweight=0.25", "--ignore-mask-label", "3,7")
    b = parse(lib, "--input-file", "x.mvs", "--number-views", "7", "--output-file=out/y.mvs", "--working-folder=wd", "--depthweight", "0.25", "--ignore-mask-label=3,7")
    assert a == b and a["result"] == OK
    assert (a["numberViews"], a["output"], a["workdir"], a["depthweight"], a["ignoreMaskLabel"]) == (7, "out/y.mvs", "wd", 0.25, "3,7")
    # the value is the next argument whatever it starts with; the SGM modes are refused afterwards
    o = parse(lib, "-i", "x.mvs", "--fusion-mode", "-1")
    assert o["fusionMode"] == -1 and o["result"] == ERROR and o["err"] == "SGM fusion modes are not available"
    assert parse(lib, "-i", "x.mvs", "--fusion-mode", "1")["result"] == OK
    o = parse(lib, "-i", "x.mvs", "--no-such-option", "1")
    assert o["result"] == ERROR and o["err"] == "unrecognised option '--no-such-option'"
    o = parse(lib, "-i", "x.mvs", "--no-such-option=1")
    assert o["result"] == ERROR and o["err"] == "unrecognised option '--no-such-option'"
    o = parse(lib, "-i", "x.mvs", "--number-views")
    assert o["result"] == ERROR and o["err"] == "the required argument for option '--number-views' is missing"
    for v in ("-1", "3"):
        o = parse(lib, "-i", "x.mvs", "--n-filter", v)
        assert o["result"] == ERROR and o["err"] == "--n-filter expects 0 (off), 1 (adjust) or 2 (strict)"
    for v in (0, 1, 2):
        assert parse(lib, "-i", "x.mvs", "--n-filter", str(v))["nFilter"] == v
    # usage: -h, --help, no input file
    assert parse(lib, "-h")["result"] == USAGE and parse(lib, "-i", "x.mvs", "--help")["result"] == USAGE and parse(lib)["result"] == USAGE
    assert parse(lib, "--number-views", "3")["result"] == USAGE
    # the other modes read neither --fusion-mode nor --n-filter; the seed of --sample-mesh keeps its 64 bits
    o = parse(lib, "-i", "m.ply", "--sample-mesh", "-1000", "--seed", str(2 ** 40 + 5), "--fusion-mode", "-1", "--n-filter", "9", "--batch", "0")
    assert o["result"] == OK and o["sampleMesh"] == -1000.0 and o["sampleSeed"] == 2 ** 40 + 5 and o["seed"] == 5 and o["output"] == "m_dense.mvs" and o["batch"] == 0
    o = parse(lib, "-i", "d.mvs", "--filter-point-cloud", "-2", "--fusion-mode", "-1")
    assert o["result"] == OK and o["thFilterPointCloud"] == -2
    assert parse(lib, "-i", "d.mvs", "--filter-point-cloud", "2", "--fusion-mode", "-1")["result"] == ERROR     # >= 0: no effect, a densify run
    assert parse(lib, "-i", "d.mvs", "--seed", "77")["sampleSeed"] == 77
    # what is accepted and ignored with a note (-v > 1)
    o = parse(lib, "-i", "x.mvs", "--n-opticalflow", "1", "--use-semantic", "0", "--n-usegeoconsistency", "2")
    assert o["result"] == OK and o["notes"] == [k + " is not available in this build (defined subset); treated as 0" for k in ("--n-opticalflow", "--n-usegeoconsistency")]
    assert parse(lib, "-i", "x.mvs", "--n-opticalflow", "1", "-v", "1")["notes"] == []
    assert parse(lib, "-i", "x.mvs", "-v", "0", "--verbosity", "3")["verbosity"] == 3


def test_option_devices(lib):
    o = parse(lib, "-i", "x.mvs", "--devices", "0,1")
    assert o["result"] == OK and o["devices"] == [0, 1] and o["device"] == 0
    assert parse(lib, "-i", "x.mvs", "--devices", "0,0")["devices"] == [0, 0]     # an ordinal may repeat: two contexts on one GPU
    o = parse(lib, "-i", "x.mvs", "--devices", "3,3", "--device", "5")
    assert o["result"] == OK and o["devices"] == [3, 3] and o["device"] == 3
    assert parse(lib, "-i", "x.mvs", "--device", "5")["devices"] == [5]
    for bad in ("0,,1", ",0", "0,a", "-1", "0, 1"):
        o = parse(lib, "-i", "x.mvs", "--devices", bad)
        assert o["result"] == ERROR and o["err"] == "--devices expects a comma-separated list of device ordinals", bad
    for bad in ("", ",".join(["0"] * 65)):
        o = parse(lib, "-i", "x.mvs", "--devices", bad)
        assert o["result"] == ERROR and o["err"] == "--devices expects 1 to 64 device ordinals", bad
    assert len(parse(lib, "-i", "x.mvs", "--devices", ",".join(["0"] * 64))["devices"]) == 64
    assert parse(lib, "-i", "x.mvs", "--devices", "0,1,")["devices"] == [0, 1]     # (getline yields no token after a trailing comma)


def test_option_derived_values(lib):
    for nopt, pf in itertools.product(range(8), (None, 0, 1)):
        args = ["-i", "x.mvs", "--n-nOptimize", str(nopt)] + ([] if pf is None else ["--n-postfilter", str(pf)])
        want = pf if pf is not None else (1 if nopt & 3 else 0)     # main: OPTIMIZE = REMOVE_SPECKLES | FILL_GAPS
        o = parse(lib, *args)
        assert o["postFilter"] == want and o["nOptimize"] == nopt
    assert lib.dp_max_batch() == 64
    assert parse(lib, "-i", "x.mvs", "--batch", "0")["batch"] == 1 and parse(lib, "-i", "x.mvs", "--batch", "-3")["batch"] == 1
    assert parse(lib, "-i", "x.mvs", "--batch", "1000")["batch"] == 64 and parse(lib, "-i", "x.mvs", "--batch", "48")["batch"] == 48
    assert parse(lib, "-i", "x.mvs", "--n-EstimationIters-external", "0")["estimationItersExternal"] == 1
    assert parse(lib, "-i", "x.mvs", "--n-EstimationIters-external", "6")["estimationItersExternal"] == 6


def test_every_known_option_is_accepted(lib):
    name = C.c_char_p()
    n = lib.dp_known_options(0, C.byref(name))
    table = []
    for k in range(n):
        lib.dp_known_options(k, C.byref(name))
        table.append(name.value.decode())
    assert table == KNOWN
    for k in KNOWN:
        if k in ("-i", "--input-file"):
            continue
        v = "0,1" if k == "--devices" else "0"
        assert parse(lib, "-i", "x.mvs", k, v)["result"] == OK, k
        assert parse(lib, "-i", "x.mvs", k + "=" + v)["result"] == OK, k
    assert parse(lib, "--input-file", "x.mvs")["input"] == "x.mvs"


# ---- schedule ---------------------------------------------------------------------------------------------------------
FIELDS = ("filtered", "serial", "meet", "snapshotSpread", "liveSpread", "workerSubmitsFinal", "mainSubmitsFinal")


def schedule_ref(pf, il, vs, nf, iters, it, any_work):
    """main(): the predicates of the worker thread, of the main thread's loop over the outer iterations and of the filter stage"""
    filter_on_last = bool((pf and (iters - 1 == 1 or iters - 1 == 2)) or (il and vs and iters - 1 >= 1))     # main: filterOnLast
    serial = bool(il and any_work and ((pf and it in (1, 2)) or (vs and it >= 1)))                            # main: serial_iteration(it)
    last = it == iters - 1
    filtered = bool(pf and it in (1, 2) and any_work)                                                         # worker and main loop alike
    snapshot = bool(not serial and vs and it >= 1)                                                            # worker: offer_spread_maps(false)
    # worker: saver_submit(batch) inside `if (!serial)`, in the loop over the device's batches -- there is none without work
    worker_submits = bool(not serial and any_work and last and not filter_on_last and not nf)
    meet = filtered or serial                                                                                 # worker: waits; main loop: does not `continue`
    live = bool(serial and vs and it >= 1)                                                                    # main loop: offer_spread_maps(true)
    main_submits = bool(meet and last and not nf)                                                             # main loop: saver_submit(work)
    return dict(filtered=filtered, serial=serial, meet=meet, snapshotSpread=snapshot, liveSpread=live, workerSubmitsFinal=worker_submits, mainSubmitsFinal=main_submits)


def test_schedule_exhaustively(lib):
    cases = 0
    for pf, il, vs, nf, iters, any_work in itertools.product((0, 1), (0, 1), (0, 1), (0, 1, 2), range(1, 6), (0, 1)):
        cases += 1
        stage = bool(nf)     # main: the filter stage submits `todo` (which holds `work`) whenever --n-filter is on
        assert lib.dp_stage_submits_final(nf) == int(stage)
        handed = 0
        for it in range(iters):
            bits = lib.dp_iteration(pf, il, vs, nf, iters, it, any_work)
            got = {f: bool(bits >> k & 1) for k, f in enumerate(FIELDS)}
            want = schedule_ref(pf, il, vs, nf, iters, it, any_work)
            assert got == want, (pf, il, vs, nf, iters, it, any_work)
            assert not (want["snapshotSpread"] and want["liveSpread"])
            if it < iters - 1:
                assert not want["workerSubmitsFinal"] and not want["mainSubmitsFinal"]
            handed += want["workerSubmitsFinal"] + want["mainSubmitsFinal"]
        # the final maps reach the saver exactly once: worker, main thread or filter stage
        if any_work:
            assert handed + stage == 1
        elif not nf:
            assert handed == 0
        else:
            assert handed == 0 and stage
    assert cases == 240


# ---- scenes for dealing, budget, batches, cloud --------------------------------------------------------------------------
class Img:
    def __init__(self, w, h, nbs=(), srcs=(), valid=True):
        self.w, self.h, self.nbs, self.srcs, self.valid = w, h, list(nbs), list(srcs), valid

    @property
    def px(self):
        return self.w * self.h


def ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def u32s(v):
    return (U32 * max(len(v), 1))(*v)


def scene_args(scene):
    nb_first, src_first = [0], [0]
    for m in scene:
        nb_first.append(nb_first[-1] + len(m.nbs)); src_first.append(src_first[-1] + len(m.srcs))
    return (len(scene), ints([m.w for m in scene]), ints([m.h for m in scene]), ints([int(m.valid) for m in scene]), ints(nb_first),
            u32s([x for m in scene for x in m.nbs]), ints(src_first), u32s([x for m in scene for x in m.srcs]))


def make_scene(sizes, n_nb):
    """images of the given sizes; image i has the n_nb images after it (cyclically; ids repeat in a small scene) as neighbours, the first three of them as
    source views; a growing neighbour count in the mixed scenes would hide the stable sort, so every second image gets one neighbour fewer.  The last image is
    uncalibrated, image 1 has not enough views: neither is in todo"""
    n = len(sizes)
    scene = []
    for i, (w, h) in enumerate(sizes):
        nbs = [(i + 1 + k) % (n - 1) for k in range(max(0, n_nb - (i % 2 if n_nb else 0)))]
        scene.append(Img(w, h, nbs, nbs[:3], valid=i != n - 1))
    todo = [i for i in range(n - 1) if i != 1 or n <= 3]
    return scene, todo


def deal_ref(scene, todo, n_dev):
    order = sorted(todo, key=lambda i: -len(scene[i].nbs))     # main: stable_sort by neighbour count, most first
    dev = [0] * len(scene)
    for k, i in enumerate(order):
        dev[i] = k % n_dev                                     # main: position k of the fusion order goes to device k mod N
    need = [[1 if n_dev == 1 else 0] * len(scene) for _ in range(n_dev)]
    if n_dev > 1:
        for i in todo:
            need[dev[i]][i] = 1
            for s in scene[i].srcs:
                need[dev[i]][s] = 1
    return order, dev, need


def deal(lib, scene, todo, n_dev):
    n = len(scene)
    order = (U32 * max(len(todo), 1))(); dev = (C.c_int * n)(); need = (C.c_int * (n * n_dev))()
    lib.dp_deal(*scene_args(scene), u32s(todo), len(todo), n_dev, order, dev, need)
    return list(order)[:len(todo)], list(dev), [list(need)[d * n:(d + 1) * n] for d in range(n_dev)]


SIZES = {"uniform": [(96, 80)] * 7, "mixed": [(96, 80), (160, 120)] * 4, "1080p": [(1920, 1080)] * 66}


@pytest.mark.parametrize("n_dev", (1, 2, 3))
def test_dealing(lib, n_dev):
    for name, n_nb in itertools.product(SIZES, (0, 8, 40)):
        scene, todo = make_scene(SIZES[name], n_nb)
        order, dev, need = deal(lib, scene, todo, n_dev)
        assert (order, dev, need) == deal_ref(scene, todo, n_dev)
        assert [dev[i] for i in order] == [k % n_dev for k in range(len(order))]
        if n_dev == 1:
            assert need == [[1] * len(scene)]
        else:
            for d in range(n_dev):
                own = set(i for i in todo if dev[i] == d)
                assert set(i for i, g in enumerate(need[d]) if g) == own | set(s for i in own for s in scene[i].srcs)


def test_registered_neighbours(lib):
    n = 45
    scene = [Img(96, 80, [(i + 1 + k) % n for k in range(40)]) for i in range(n)]
    scene[3].nbs = [7, 5]
    todo = [i for i in range(n) if i % 6 != 5]
    out = (U32 * 64)()
    for i in (0, 3, 10, 44):
        k = lib.dp_registered_neighbors(*scene_args(scene), i, u32s(todo), len(todo), out)
        want = [x for x in scene[i].nbs if x in todo][:31]     # main: register_maps -- neighbours that are in todo, in their order, 31 at the most
        assert list(out)[:k] == want
    assert len([x for x in scene[0].nbs if x in todo]) > 31


# ---- budget -----------------------------------------------------------------------------------------------------------
def budget_ref(scene, todo, dev, need, d, free, restore, n_filter, fusion_mode, fuse_count, batch):
    """main: the block "What has to fit into a device" """
    n_dev = len(need)
    max_px = max(scene[i].px for i in todo); all_px = sum(scene[i].px for i in todo)
    own_px = sum(scene[i].px for i in todo if dev[i] == d)
    gray_px = sum(m.px for i, m in enumerate(scene) if m.valid and need[d][i])
    resident = own_px * (20 + (16 if restore else 0)) + gray_px * (8 + 16) + (1 << 30)
    if d == 0:
        max_nb = max([1] + [min(len(scene[i].nbs), 31) for i in todo])
        resident += all_px * 4 + (all_px * 20 if n_dev > 1 else 0) + max_px * (12 * max_nb + 40)
        if n_filter:
            resident += all_px * 8 + max_px * 8 * 8
        if fusion_mode != 1:
            resident += all_px // 5 * (31 + 3 * 8) if (all_px * 39 > 4 * GIB and fuse_count != 0) else all_px // 2 * 31 + all_px * 8
    per_image = max_px * 24
    b = batch
    while b > 1 and resident + b * per_image > free:
        b //= 2
    return dict(resident=resident, perImage=per_image, batch=b, fits=resident + b * per_image <= free, ownImages=sum(1 for i in todo if dev[i] == d))


@pytest.mark.parametrize("n_dev", (1, 2, 3))
@pytest.mark.parametrize("name", list(SIZES))
def test_budget(lib, n_dev, name):
    out = (U64 * 6)()
    batches_seen = set()
    for n_nb in (0, 8, 40):
        scene, todo = make_scene(SIZES[name], n_nb)
        args = scene_args(scene)
        order, dev, need = deal_ref(scene, todo, n_dev)
        for restore, n_filter, fusion_mode, fuse_count, d in itertools.product((0, 1), (0, 1), (0, 1), (-1, 0, 1), range(n_dev)):
            base = budget_ref(scene, todo, dev, need, d, 1 << 62, restore, n_filter, fusion_mode, fuse_count, 32)
            res, per = base["resident"], base["perImage"]
            # free memory at which the batch comes out as 32, as 16 (exactly, and one byte short of 32), as 1, and at which nothing fits
            for free, batch in ((res + 32 * per, 32), (res + 32 * per - 1, 16), (res + 16 * per, 16), (res + 2 * per - 1, 1), (res + per, 1), (res + per - 1, 0)):
                want = budget_ref(scene, todo, dev, need, d, free, restore, n_filter, fusion_mode, fuse_count, 32)
                assert want["fits"] == (batch != 0) and (not batch or want["batch"] == batch)
                lib.dp_budget(*args, u32s(todo), len(todo), n_dev, d, free, restore, n_filter, fusion_mode, fuse_count, 32, out)
                got = dict(resident=out[0], perImage=out[1], batch=out[2], fits=bool(out[3]), ownImages=out[4])
                assert got == want, (n_nb, restore, n_filter, fusion_mode, fuse_count, d, free)
                assert out[5] == want["resident"] + want["batch"] * want["perImage"]
                batches_seen.add(batch)
            # a batch the command line asks for is never raised
            lib.dp_budget(*args, u32s(todo), len(todo), n_dev, d, 1 << 62, restore, n_filter, fusion_mode, fuse_count, 5, out)
            assert out[2] == 5 and out[3] == 1
    assert batches_seen == {32, 16, 1, 0}


def test_budget_design_numbers(lib):
    """64 images of 1920x1080 on one device: the scene is past the budget's count-first threshold, so the cloud is reserved as 0.2 points per pixel"""
    scene, todo = make_scene(SIZES["1080p"], 8)
    assert len(todo) == 64 and sum(scene[i].px for i in todo) * 39 > 4 * GIB
    order, dev, need = deal_ref(scene, todo, 1)
    want = budget_ref(scene, todo, dev, need, 0, 288 * GIB, 0, 0, 0, -1, 32)
    out = (U64 * 6)()
    lib.dp_budget(*scene_args(scene), u32s(todo), len(todo), 1, 0, 288 * GIB, 0, 0, 0, -1, 32, out)
    assert (out[0], out[2], out[3]) == (want["resident"], 32, 1) and want["batch"] == 32


# ---- batches ----------------------------------------------------------------------------------------------------------
def batches_ref(scene, work, batch):
    """main: the block "batches" """
    per_dev = []
    for d, ids in enumerate(work):
        by_class = {8: [], 16: []}
        for i in ids:
            by_class[8 if len(scene[i].srcs) <= 8 else 16].append(i)
        per_dev.append([(d, g[b0:b0 + batch]) for c, g in sorted(by_class.items()) for b0 in range(0, len(g), batch)])
    out = []
    for k in range(max([len(p) for p in per_dev] + [0])):
        out += [p[k] for p in per_dev if k < len(p)]
    return out


def test_batches(lib):
    n = 40
    scene = [Img(96, 80, [], list(range(9 + i % 4)) if i % 3 == 0 else list(range(1 + i % 8))) for i in range(n)]
    assert {len(m.srcs) for m in scene} >= {8, 9}
    for n_dev, batch in itertools.product((1, 2, 3), (1, 3, 4, 32)):
        work = [[i for i in range(n) if i % 5 != 4 and (i // 2) % n_dev == d] for d in range(n_dev)]
        if n_dev == 3:
            work[2] = work[2][:2]     # a device with fewer batches drops out of the rotation
        first = [0]
        for ids in work:
            first.append(first[-1] + len(ids))
        text = lib.dp_batches(*scene_args(scene), n_dev, ints(first), u32s([i for ids in work for i in ids]), batch).decode()
        got = [(int(l.split(":")[0]), [int(x) for x in l.split(":")[1].split()]) for l in text.splitlines()]
        assert got == batches_ref(scene, work, batch)
        for d, ids in got:
            assert 1 <= len(ids) <= batch and all(i in work[d] for i in ids)
            assert len({len(scene[i].srcs) <= 8 for i in ids}) == 1                               # the two lane layouts never share a launch
        assert sorted(i for _, ids in got for i in ids) == sorted(i for ids in work for i in ids)  # every image once
        rounds = [d for d, _ in got]
        for d in range(n_dev):                                                                     # round-robin: the k-th batches of all devices before any (k + 1)-th
            pos = [k for k, x in enumerate(rounds) if x == d]
            for e in range(n_dev):
                pe = [k for k, x in enumerate(rounds) if x == e]
                assert all(pos[k] < pe[k + 1] for k in range(min(len(pos), len(pe) - 1)))
        if batch == 3 and n_dev == 1:
            assert any(len(ids) < batch for _, ids in got)                                         # the last, short batch of a class
    assert lib.dp_batches(*scene_args(scene), 2, ints([0, 0, 0]), u32s([]), 4) == b""


# ---- cloud ------------------------------------------------------------------------------------------------------------
def test_cloud_sizes(lib):
    out = (U64 * 2)()
    for name in SIZES:
        scene, todo = make_scene(SIZES[name], 8)
        scene[0].w += 1     # an odd pixel count: n / 2 rounds down per image
        for nvf in (1, 2, 3):
            lib.dp_cloud_worst_case(*scene_args(scene), u32s(todo), len(todo), nvf, out)
            # main: capacity += numberViewsFuse >= 2 ? n / 2 : n; viewCapacity += n
            assert out[0] == sum(scene[i].px // 2 if nvf >= 2 else scene[i].px for i in todo) and out[1] == sum(scene[i].px for i in todo)
    # main: (capacity * 31 + viewCapacity * 8) > 4 GiB || fuseCount == 1, and then only if fuseCount != 0
    edge = (4 * GIB - 31 * 1000) // 8     # 31 * 1000 + 8 * edge == 4 GiB exactly (4 GiB - 31000 is a multiple of 8)
    assert 31 * 1000 + 8 * edge == 4 * GIB
    for view_cap, fuse_count in itertools.product((edge - 1, edge, edge + 1, 0), (-1, 0, 1)):
        want = (31 * 1000 + 8 * view_cap > 4 * GIB or fuse_count == 1) and fuse_count != 0
        assert lib.dp_fusion_counts_first(1000, view_cap, fuse_count) == int(want)
    assert lib.dp_fusion_counts_first(1000, edge, -1) == 0 and lib.dp_fusion_counts_first(1000, edge + 1, -1) == 1
    # the budget's own estimate (39 B per pixel of the scene; --fuse-count 1 does not enter): a different formula, side by side with the one above
    for all_px, fuse_count in itertools.product((4 * GIB // 39 - 1, 4 * GIB // 39, 4 * GIB // 39 + 1, 12345), (-1, 0, 1)):
        first = all_px * 39 > 4 * GIB and fuse_count != 0
        assert lib.dp_budget_counts_first(all_px, fuse_count) == int(first)
        assert lib.dp_budget_cloud_bytes(all_px, fuse_count) == (all_px // 5 * (31 + 3 * 8) if first else all_px // 2 * 31 + all_px * 8)
    assert lib.dp_budget_counts_first(4 * GIB // 39, -1) == 0 and lib.dp_budget_counts_first(4 * GIB // 39 + 1, -1) == 1
    assert lib.dp_budget_counts_first(12345, 1) == 0 and lib.dp_fusion_counts_first(1, 1, 1) == 1     # where the two differ


# ---- working size -----------------------------------------------------------------------------------------------------
def working_size_ref(w, h, level, min_size, max_size):
    """main's working_size: TImage::computeMaxResolution + Image::ResizeImage"""
    image_size = max(w, h)
    if level == 0:
        size = min(image_size, max_size)
    else:
        size = image_size >> level
        if size < min_size:
            level = 0
            while (image_size >> (level + 1)) >= min_size:
                level += 1
            size = image_size >> level
        size = min(size, max_size)
    if size == 0 or image_size <= size:
        return w, h
    return (size, h * size // w) if w > h else (w * size // h, size)


def test_working_size(lib):
    nw, nh = C.c_int(), C.c_int()
    for (w, h), level, (lo, hi) in itertools.product(((1920, 1080), (1080, 1920), (4000, 3000), (640, 480), (641, 479), (500, 500), (3, 5)), range(4),
                                                     ((640, 3200), (1, 3200), (640, 800), (1, 100), (2000, 3200), (700, 600))):
        lib.dp_working_size(w, h, level, lo, hi, C.byref(nw), C.byref(nh))
        assert (nw.value, nh.value) == working_size_ref(w, h, level, lo, hi), (w, h, level, lo, hi)
    lib.dp_working_size(1920, 1080, 1, 640, 3200, C.byref(nw), C.byref(nh))
    assert (nw.value, nh.value) == (960, 540)
    lib.dp_working_size(1080, 1920, 2, 640, 3200, C.byref(nw), C.byref(nh))
    assert (nw.value, nh.value) == (540, 960)     # level 2 would be 480 < 640: level 1 is the last one not below the minimum


# ---- view selection against the oracle -------------------------------------------------------------------------------------
def test_view_selection_matches_the_oracle(lib):
    """the scene of test_densify_driver_rescales_mismatched_neighbours (tests/test_gpu_driver.py): four 320x240 views, one at 1.7x the distance"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import select_views as SV
    import scene_files as SF
    synth = importlib.import_module("hc-mvs_amd.synth")
    w, h, f = 320, 240, 380.0
    px = 10.0 / f
    scene = synth.Scene(7, min_wavelength=3.5 * px, max_wavelength=150 * px)
    base = synth.make_views(w, h, f, 4, seed=7, baseline=(0.05, 0.1), scene=scene)
    far = 2
    Cf = np.array([base[far]["C"][0], base[far]["C"][1], -0.7 * scene.depth0])
    Rf = synth.look_at(Cf, np.array([0.0, 0.0, scene.depth0]))
    g, d, n = scene.render(base[far]["K"], Rf, Cf, w, h)
    base[far] = dict(K=base[far]["K"], R=Rf, C=Cf, gray=g, depth=d, normal=n, width=w, height=h)
    verts = SF.sparse_vertices(base, 250, seed=3)
    # what the driver reads from the scene file SF.write_scene writes: one camera (K of view 0 at w x h, R = I, C = 0), one pose per image
    K = np.ascontiguousarray(base[0]["K"], np.float64)
    R = np.ascontiguousarray(np.stack([v["R"] for v in base]), np.float64); Cs = np.ascontiguousarray(np.stack([v["C"] for v in base]), np.float64)
    X = np.ascontiguousarray(np.stack([x["X"] for x in verts]), np.float32)
    first = [0]
    for x in verts:
        first.append(first[-1] + len(x["views"]))
    ids = [j for x in verts for j, _ in x["views"]]
    PD, PF = C.POINTER(C.c_double), C.POINTER(C.c_float)
    text = lib.dp_select_views(len(base), w, h, K.ctypes.data_as(PD), R.ctypes.data_as(PD), Cs.ctypes.data_as(PD), w, h, len(verts), X.ctypes.data_as(PF), ints(first),
                               u32s(ids), 12, 4).decode()     # (12: nMaxViews of the driver, 4: --number-views of the GPU test)
    got = {}
    for line in text.splitlines():
        head, srcs, scales, nb_ids, nb_scales = [p.split() for p in line.split("|")]
        got[int(head[0])] = dict(ok=int(head[1]), points=int(head[2]), srcs=[int(x) for x in srcs], scales=[float(x) for x in scales], nb=[int(x) for x in nb_ids],
                                 nb_scales=[float(x) for x in nb_scales])
    cams = [dict(K=v["K"], R=v["R"], C=v["C"]) for v in base]
    vlist = [(x["X"], [j for j, _ in x["views"]]) for x in verts]
    n_scaled = 0
    for i in range(len(base)):
        sel = SV.select(cams, [(w, h)] * len(base), vlist, i, number_views=4)
        m = got[i]
        assert sel is not None and m["ok"] == 1
        assert m["srcs"] == [s[0] for s in sel["srcs"]]                      # the same source views in the same order
        assert m["nb"] == [q["id"] for q in sel["neighbors"]]                # the same neighbours
        assert m["points"] == len(sel["points"])
        for q, scale in zip(sel["neighbors"], m["nb_scales"]):
            assert abs(q["scale"] - scale) < 0.006
        for (sid, sscale), scale in zip(sel["srcs"], m["scales"]):
            assert abs(sscale - scale) < 0.006 and (sscale != 1.0) == (scale != 1.0)
            n_scaled += scale != 1.0
    assert n_scaled >= 4     # the far view as a neighbour of the others, and the others as neighbours of the far view

"""The host half of an estimate call (hc-mvs_amd/csrc/est_plan.h) on the CPU: the constants of an item bit for bit against what the
oracle's ctx_init derives on its own (oracle/hcmvs_oracle.c, hcor_estimate_consts), the 4 GiB image window and its slab layout, the
aliasing rule of view spread, the argument checks, and the environment knobs (sweep_plan.h).  tests/est_plan_shim.cpp is compiled with
g++ alone, with -ffp-contract=off as the library is: no HIP, no library."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

synth = importlib.import_module("hc-mvs_amd.synth")
Params = importlib.import_module("hc-mvs_amd.binding").Params

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hc-mvs_amd", "csrc")
SRC = os.path.join(HERE, "est_plan_shim.cpp")
HDRS = [os.path.join(CSRC, h) for h in ("est_plan.h", "pm_types.h", "sweep_plan.h", "carve.h")] + \
       [os.path.join(os.path.dirname(HERE), "include", "hcmvs_hip.h")]
LIB_PATH = os.path.join(HERE, "libest_plan_shim.so")
V_MAX = 16
LIMIT = 0xFFFF0000
U64 = C.c_uint64
REASONS = ("ok", "batch_size", "half_window", "iter_counts", "src_count", "src_class", "null", "depth_range", "border")


class Cam(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("R", C.c_double * 9), ("C", C.c_double * 3), ("w", C.c_int32), ("h", C.c_int32)]


class Item(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("W", "H", "V", "border", "adapthalfwin", "nRandomIters", "itExternal", "propHalfwin", "propStep", "hintIter")] + \
               [("seed", C.c_uint32), ("pointersSet", C.c_int32), ("Hr", C.c_float * 9)] + \
               [(n, C.c_float) for n in ("dMin", "dMax", "dMinSqr", "dMaxSqr", "smoothBonusDepth", "smoothBonusNormal", "smoothSigmaDepth",
                                         "smoothSigmaNormal", "angle1Range", "angle2Range", "thConfSmall", "thConfBig", "thConfRand", "thRobust",
                                         "thKeep", "depthRatio", "pfScale")] + \
               [(n, C.c_double) for n in ("cx", "cy", "ifx", "ify")] + \
               [("A", C.c_float * 9 * V_MAX), ("Hm", C.c_float * 3 * V_MAX), ("vw", C.c_int32 * V_MAX), ("vh", C.c_int32 * V_MAX)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB_PATH) or any(os.path.getmtime(d) > os.path.getmtime(LIB_PATH) for d in [SRC] + HDRS):
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-o", LIB_PATH, SRC])
    L = C.CDLL(LIB_PATH)
    L.ep_item.argtypes = [C.POINTER(Cam), C.POINTER(Cam), C.c_int, C.POINTER(Params), C.c_float, C.c_float, C.c_uint32, C.c_int, C.POINTER(Item)]
    L.ep_item.restype = None
    L.ep_spread.argtypes = [C.POINTER(Cam), C.POINTER(Cam), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    L.ep_spread.restype = None
    L.ep_window.argtypes = [C.POINTER(U64), C.POINTER(U64), C.c_int, C.POINTER(C.c_uint32), C.POINTER(U64)]
    L.ep_carve.argtypes = [C.POINTER(U64), C.c_int, C.POINTER(U64)]
    L.ep_carve.restype = U64
    L.ep_overlap.argtypes = [C.POINTER(U64), C.POINTER(U64), C.c_int, C.POINTER(C.c_int)]
    L.ep_overlap.restype = None
    L.ep_check_call.argtypes = [C.c_int, C.POINTER(Params)]
    L.ep_check_items.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.ep_check_image.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.POINTER(C.c_int)]
    L.ep_uses_hint.argtypes = [C.POINTER(Params), C.c_int]
    L.ep_view_spreads.argtypes = [C.c_int, C.POINTER(Params), C.c_int, C.c_int]
    L.ep_sweep_item.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    L.ep_sweep_item.restype = None
    L.ep_knobs.argtypes = [C.c_char_p] * 5 + [C.POINTER(C.c_int)]
    L.ep_knobs.restype = None
    return L


@pytest.fixture(scope="module")
def reason(lib):
    sizes = (C.c_int * 3)(); codes = (C.c_int * len(REASONS))()
    lib.ep_layout(sizes, codes)
    assert len(set(codes)) == len(REASONS) and codes[0] == 0
    return dict(zip(REASONS, codes))


# ---- the constants against the oracle ----

# what the library's hcmvs_default_params fills (include/hcmvs_hip.h)
DEFAULTS = dict(adapthalfwin=5, n_estimation_iters=1, it_external=0, n_external_iters=1, propagate_halfwin=1, propagate_step=4, n_random_iters=6,
                ncc_threshold_keep=0.55, random_depth_ratio=0.003, random_angle1_deg=16.0, random_angle2_deg=10.0, random_smooth_depth=0.02,
                random_smooth_normal_deg=13.0, random_smooth_bonus=0.93, photometric_flow=0.0, seed=1234, median_blur=1)
PARAM_CASES = {
    "defaults": {},
    "halfwin10": dict(adapthalfwin=10),
    "halfwin7_iters": dict(adapthalfwin=7, n_estimation_iters=4, it_external=1, n_external_iters=3, propagate_halfwin=3, propagate_step=2, n_random_iters=11),
    "thresholds": dict(ncc_threshold_keep=0.61, random_smooth_depth=0.031, random_smooth_normal_deg=17.5, random_smooth_bonus=0.88,
                       random_angle1_deg=21.0, random_angle2_deg=7.5, photometric_flow=0.15, random_depth_ratio=0.0047),
}


def params_pair(**kw):
    d = dict(DEFAULTS); d.update(kw)
    p = Params()
    for k, v in d.items():
        setattr(p, k, v)
    po = O.default_params()
    for k, v in d.items():
        setattr(po, k, v)
    return p, po


_views = {}


def cameras(kind, V):
    """views[0] the reference, views[1:] V source views: synth's at the smoke size, or the same with non-square pixels and an off-centre
    principal point that differ from view to view"""
    if V not in _views:
        _views[V] = synth.make_views(96, 80, 90.0, V, seed=3)
    views = _views[V]
    if kind == "skewed":
        out = []
        for i, v in enumerate(views):
            K = v["K"].copy()
            K[0, 0] = 90.0 + 1.7 * i; K[1, 1] = 97.3 - 0.9 * i; K[0, 2] = 51.3 - 0.6 * i; K[1, 2] = 33.7 + 0.4 * i
            v = dict(v); v["K"] = K
            out.append(v)
        views = out
    return views


def cam_of(v):
    c = Cam()
    c.K[:] = list(np.asarray(v["K"], np.float64).ravel()); c.R[:] = list(np.asarray(v["R"], np.float64).ravel())
    c.C[:] = list(np.asarray(v["C"], np.float64).ravel())
    c.h, c.w = v["gray"].shape
    return c


def plan_item(lib, views, p, d_min, d_max, seed_offset=0, hint=False):
    ref = cam_of(views[0])
    srcs = (Cam * (len(views) - 1))(*[cam_of(v) for v in views[1:]])
    out = Item()
    lib.ep_item(C.byref(ref), srcs, len(views) - 1, C.byref(p), d_min, d_max, seed_offset, int(hint), C.byref(out))
    return out


def bits(x):
    a = np.ascontiguousarray(np.array(x))
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b, what):
    a, b = np.array(a), np.array(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %r != %r" % (what, a, b)


F32_FIELDS = ("dMin", "dMax", "dMinSqr", "dMaxSqr", "smoothBonusDepth", "smoothBonusNormal", "smoothSigmaDepth", "smoothSigmaNormal", "angle1Range",
              "angle2Range", "thConfSmall", "thConfBig", "thConfRand", "thRobust")


def check_against_oracle(lib, views, kw, d_min, d_max, seed_offset=0):
    p, po = params_pair(**kw)
    V = len(views) - 1
    k = plan_item(lib, views, p, d_min, d_max, seed_offset)
    o = O.estimate_consts(views, po, d_min, d_max)
    # the numbers the oracle derives on its own
    same_bits(np.array(k.Hr, np.float32), np.array(o.Hrf, np.float32), "Hr")
    same_bits(np.array(k.A, np.float32)[:V], np.array(o.Af, np.float32)[:V], "A")
    same_bits(np.array(k.Hm, np.float32)[:V], np.array(o.Hmf, np.float32)[:V], "Hm")
    same_bits(np.float64(k.ifx), np.float64(o.ifx), "ifx"); same_bits(np.float64(k.ify), np.float64(o.ify), "ify")
    for f in F32_FIELDS:
        same_bits(np.float32(getattr(k, f)), np.float32(getattr(o, f)), f)
    # the members the oracle reads straight from its arguments
    K = np.asarray(views[0]["K"], np.float64)
    same_bits(np.float64(k.cx), K[0, 2], "cx"); same_bits(np.float64(k.cy), K[1, 2], "cy")
    same_bits(np.float32(k.thKeep), np.float32(p.ncc_threshold_keep), "thKeep")
    same_bits(np.float32(k.depthRatio), np.float32(p.random_depth_ratio), "depthRatio")
    same_bits(np.float32(k.pfScale), np.float32(1) - np.float32(p.photometric_flow), "pfScale")
    h, w = views[0]["gray"].shape
    assert (k.W, k.H, k.V) == (w, h, V)
    assert k.border == max(7, p.adapthalfwin)
    assert (k.adapthalfwin, k.nRandomIters, k.itExternal, k.propHalfwin, k.propStep) == \
           (p.adapthalfwin, p.n_random_iters, p.it_external, p.propagate_halfwin, p.propagate_step)
    assert k.seed == (p.seed + seed_offset) % 2 ** 32
    assert k.hintIter == -1 and k.pointersSet == 0
    for v in range(V_MAX):
        hh, ww = views[1 + v]["gray"].shape if v < V else (0, 0)
        assert (k.vw[v], k.vh[v]) == (ww, hh)
        if v >= V:
            assert not np.any(np.array(k.A[v])) and not np.any(np.array(k.Hm[v]))
    # view spread, every source view
    ref = cam_of(views[0])
    for v in range(V):
        out = (C.c_double * 8)(); wh = (C.c_int * 2)()
        s = cam_of(views[1 + v])
        lib.ep_spread(C.byref(ref), C.byref(s), out, wh)
        Kj = np.asarray(views[1 + v]["K"], np.float64)
        same_bits(np.array(out[0:2]), np.array([Kj[0, 2], Kj[1, 2]]), "spread cx, cy of view %d" % v)
        same_bits(np.array(out[2:4]), np.array([o.jifx[v], o.jify[v]]), "spread ifx, ify of view %d" % v)
        same_bits(np.array(out[4:7]), np.array(o.spT[v][6:9]), "spread Tz of view %d" % v)
        same_bits(np.float64(out[7]), np.float64(o.spt[v][2]), "spread tz of view %d" % v)
        assert (wh[0], wh[1]) == (s.w, s.h)


@pytest.mark.parametrize("V", [1, 8, 9, 16])
@pytest.mark.parametrize("kind", ["synth", "skewed"])
@pytest.mark.parametrize("case", sorted(PARAM_CASES))
def test_constants_match_the_oracle_bit_for_bit(lib, kind, V, case):
    check_against_oracle(lib, cameras(kind, V), PARAM_CASES[case], 7.25, 13.5)


@pytest.mark.parametrize("kind", ["synth", "skewed"])
def test_constants_with_a_zero_near_depth_and_a_seed_offset(lib, kind):
    check_against_oracle(lib, cameras(kind, 8), {}, 0.0, 13.5)                                 # the `restore` variant's range
    check_against_oracle(lib, cameras(kind, 9), PARAM_CASES["thresholds"], 0.0, 0.37, seed_offset=77)
    check_against_oracle(lib, cameras(kind, 1), dict(seed=0xFFFFFFF0), 2.0, 3.0, seed_offset=0x20)  # the sum wraps like uint32


def test_the_structures_keep_the_layout_the_kernels_read(lib):
    sizes = (C.c_int * 3)(); codes = (C.c_int * len(REASONS))()
    lib.ep_layout(sizes, codes)
    # EstConst: 9 i32 (+4) | 4 pointers | 9 f32 (+4) | 4 f64 | 17 f32, u32 | 5 pointers | i32 (+4) | 2 pointers; DevView: u32, 2 i32, 12 f32;
    # SpreadView: 3 pointers, 2 i32, 8 f64
    assert list(sizes) == [280, 60, 96]


def test_the_hint_belongs_to_the_last_sweep_of_the_last_outer_iteration(lib):
    views = cameras("synth", 1)
    for it_ext, n_ext, offered, want in ((0, 1, True, True), (0, 1, False, False), (1, 3, True, False), (2, 3, True, True), (2, 3, False, False)):
        p, _ = params_pair(it_external=it_ext, n_external_iters=n_ext, n_estimation_iters=5)
        assert bool(lib.ep_uses_hint(C.byref(p), int(offered))) == want
        assert plan_item(lib, views, p, 1.0, 2.0, hint=offered).hintIter == (4 if want else -1)


def test_a_view_spreads_from_outer_iteration_one_when_it_offers_maps_of_its_size(lib):
    for on in (0, 1):
        for it_ext in (0, 1, 2):
            for maps in (0, 1):
                for rescaled in (0, 1):
                    p, _ = params_pair(it_external=it_ext, n_external_iters=3)
                    want = bool(on and it_ext >= 1 and maps and not rescaled)
                    assert bool(lib.ep_view_spreads(on, C.byref(p), maps, rescaled)) == want


def test_the_sweep_item_restates_the_constants(lib):
    def item(W, H, border, V, hint, hint_iter, keep, spread, n_sweeps):
        out = (C.c_int * 6)()
        lib.ep_sweep_item((C.c_int * 8)(W, H, border, V, hint, hint_iter, keep, spread), n_sweeps, out)
        return list(out)
    assert item(96, 80, 7, 3, 0, -1, 0, 0, 2) == [66, 82, 3, 0, 0, 0]
    assert item(96, 80, 10, 16, 1, 1, 1, 1, 2) == [60, 76, 16, 1, 1, 1]
    assert item(96, 80, 7, 3, 1, 1, 0, 0, 3) == [66, 82, 3, 0, 0, 0]      # the hint's sweep is not the call's last
    assert item(96, 80, 7, 3, 0, 1, 0, 1, 2) == [66, 82, 3, 0, 0, 1]      # hintIter without the maps is no hint


# ---- the image window ----

def window(lib, addr, sizes):
    n = len(addr)
    off = (C.c_uint32 * n)(); bs = (U64 * 2)()
    kind = lib.ep_window((U64 * n)(*addr), (U64 * n)(*sizes), n, off, bs)
    return ("direct", "slab", "refused")[kind], list(off), bs[0], bs[1]


def carve(lib, sizes):
    off = (U64 * len(sizes))()
    total = lib.ep_carve((U64 * len(sizes))(*sizes), len(sizes), off)
    return list(off), total


def test_images_within_the_window_are_addressed_from_the_lowest(lib):
    base = 0x7F0000001000
    sizes = [96 * 80 * 16, 1000, 640 * 480 * 16]
    hi = base + LIMIT - 1                                     # span 0xFFFF0000 - 1: the last view ends there
    addr = [base + 0x40000000, base, hi - sizes[2]]
    kind, off, b, _ = window(lib, addr, sizes)
    assert kind == "direct" and b == base and off == [a - base for a in addr]
    kind, off, b, _ = window(lib, [addr[2], addr[0], addr[1]], [sizes[2], sizes[0], sizes[1]])   # the order does not matter
    assert kind == "direct" and b == base and off == [addr[2] - base, addr[0] - base, 0]


def test_a_span_of_the_limit_takes_the_slab_in_carve_order(lib):
    base = 0x7F0000001000
    sizes = [96 * 80 * 16, 1000, 640 * 480 * 16]
    addr = [base + 0x40000000, base, base + LIMIT - sizes[2]]   # span 0xFFFF0000 exactly
    kind, off, _, total = window(lib, addr, sizes)
    want_off, want_total = carve(lib, sizes)
    assert kind == "slab" and off == want_off and total == want_total
    assert want_off == [0, 122880, 122880 + 1024] and want_total == 122880 + 1024 + 640 * 480 * 16   # each piece rounded up to 256 bytes
    kind, off, _, total = window(lib, addr[::-1], sizes[::-1])                                       # in the order of the views
    assert kind == "slab" and (off, total) == carve(lib, sizes[::-1])


def test_a_slab_that_reaches_the_limit_is_refused(lib):
    far = [0x100000000000, 0x200000000000]
    half = LIMIT // 2                                                   # a multiple of 256
    assert window(lib, far, [half, half - 256])[0] == "slab"
    assert window(lib, far, [half, half])[0] == "refused"               # total == 0xFFFF0000
    assert window(lib, far, [half, half + 256])[0] == "refused"
    assert window(lib, far, [half, half - 256 + 1])[0] == "refused"     # the rounding of the last piece counts


def test_the_window_of_a_single_view(lib):
    assert window(lib, [0x7F0012345600], [96 * 80 * 16]) == ("direct", [0], 0x7F0012345600, 0)
    assert window(lib, [0x7F0012345600], [LIMIT - 1])[0] == "direct"
    kind, off, _, total = window(lib, [0x7F0012345600], [LIMIT])          # one image of the limit: not addressable, whatever is done
    assert kind == "refused" and off == [0] and total == LIMIT


# ---- view spread: the aliasing rule ----

FAR = 0x100000000   # apart enough for any two maps below


def batch(n):
    """n items of 40 x 30 with 3 source views each, every map far from every other; no item spreads, no view offers maps"""
    items = []
    for i in range(n):
        a = (1 + i) * 64 * FAR
        items.append(dict(W=40, H=30, depth=a, normal=a + FAR, conf=a + 2 * FAR, n_src=3, spread=0, views={}))
    return items


def offer(items, i, v, depth, normal=None, conf=None, w=40, h=30):
    a = (1 + i) * 64 * FAR + (8 + 3 * v) * FAR
    items[i]["views"][v] = (depth if depth is not None else a, normal if normal is not None else a + FAR, conf if conf is not None else a + 2 * FAR, w, h)
    items[i]["spread"] = 1


def overlap(lib, items):
    n = len(items)
    it = (U64 * (7 * n))(); vs = (U64 * (5 * V_MAX * n))()
    for i, d in enumerate(items):
        it[7 * i:7 * i + 7] = [d["W"], d["H"], d["depth"], d["normal"], d["conf"], d["n_src"], d["spread"]]
        for v, m in d["views"].items():
            vs[5 * (V_MAX * i + v):5 * (V_MAX * i + v) + 5] = list(m)
    out = (C.c_int * 3)()
    lib.ep_overlap(it, vs, n, out)
    return tuple(out)


NONE = (-1, -1, -1)
PX = 40 * 30


def test_ranges_that_touch_are_accepted_and_one_shared_byte_is_refused(lib):
    for field, width in (("depth", 4), ("normal", 12), ("conf", 4)):
        items = batch(1)
        offer(items, 0, 1, depth=items[0][field] + PX * width)           # begins where the item's map ends
        assert overlap(lib, items) == NONE, field
        offer(items, 0, 1, depth=items[0][field] + PX * width - 1)
        assert overlap(lib, items) == (0, 0, 1), field
        offer(items, 0, 1, depth=items[0][field] - PX * 4)               # ends where the item's map begins
        assert overlap(lib, items) == NONE, field
        offer(items, 0, 1, depth=items[0][field] - PX * 4 + 1)
        assert overlap(lib, items) == (0, 0, 1), field


def test_a_normal_map_is_twelve_bytes_a_pixel(lib):
    items = batch(1)
    offer(items, 0, 2, depth=None, conf=items[0]["normal"] + PX * 4)     # clears n * 4 of the item's normals, not n * 12
    assert overlap(lib, items) == (0, 0, 2)
    offer(items, 0, 2, depth=None, conf=items[0]["normal"] + PX * 12)
    assert overlap(lib, items) == NONE
    items = batch(1)
    offer(items, 0, 0, depth=None, normal=items[0]["conf"] - PX * 4)     # the view's normals reach into the item's conf
    assert overlap(lib, items) == (0, 0, 0)
    offer(items, 0, 0, depth=None, normal=items[0]["conf"] - PX * 12)
    assert overlap(lib, items) == NONE
    items = batch(1)
    offer(items, 0, 0, depth=items[0]["depth"] - 70 * 50 * 4 + 1, w=70, h=50)   # a view of another size: its own extent counts
    assert overlap(lib, items) == (0, 0, 0)
    offer(items, 0, 0, depth=items[0]["depth"] - 70 * 50 * 4, w=70, h=50)
    assert overlap(lib, items) == NONE


def test_a_spread_view_of_another_item_is_found_first_in_loop_order(lib):
    items = batch(3)
    offer(items, 2, 1, depth=items[0]["conf"])                           # item 0 writes what a source view of item 2 offers
    assert overlap(lib, items) == (0, 2, 1)
    offer(items, 1, 2, depth=None, conf=items[0]["depth"] + 8)
    assert overlap(lib, items) == (0, 1, 2)                              # the other item counts before the view
    offer(items, 1, 0, depth=None, normal=items[1]["normal"])
    assert overlap(lib, items) == (0, 1, 2)                              # the item counts before the other item
    offer(items, 0, 2, depth=items[0]["normal"] + 100)
    assert overlap(lib, items) == (0, 0, 2)
    offer(items, 0, 0, depth=items[0]["depth"])
    assert overlap(lib, items) == (0, 0, 0)


def test_items_that_do_not_spread_and_views_beyond_the_count_are_passed_over(lib):
    items = batch(2)
    offer(items, 1, 1, depth=items[0]["depth"])
    assert overlap(lib, items) == (0, 1, 1)
    items[1]["spread"] = 0                                               # EstConst::spread null: the item's table is not read by the launch
    assert overlap(lib, items) == NONE
    items = batch(2)
    offer(items, 1, 3, depth=items[0]["depth"])                          # n_src is 3: entry 3 is not a view of the item
    assert overlap(lib, items) == NONE
    items[1]["n_src"] = 4
    assert overlap(lib, items) == (0, 1, 3)


# ---- the argument checks ----

def check_items(lib, n_src, d_min=None, d_max=None, null=None):
    n = len(n_src)
    at = C.c_int()
    r = lib.ep_check_items((C.c_int * n)(*n_src), (C.c_float * n)(*(d_min or [1.0] * n)), (C.c_float * n)(*(d_max or [2.0] * n)),
                           (C.c_int * n)(*(null or [0] * n)), n, C.byref(at))
    return r, at.value


def test_the_call_as_a_whole(lib, reason):
    def call(n, **kw):
        p, _ = params_pair(**kw)
        return lib.ep_check_call(n, C.byref(p))
    assert call(1) == call(64) == reason["ok"]
    assert call(0) == call(65) == call(-1) == reason["batch_size"]
    assert call(1, adapthalfwin=1) == call(1, adapthalfwin=10) == reason["ok"]
    assert call(1, adapthalfwin=0) == call(1, adapthalfwin=11) == reason["half_window"]
    assert call(1, n_random_iters=20) == call(1, n_random_iters=0) == call(1, n_estimation_iters=0) == reason["ok"]
    assert call(1, n_random_iters=21) == call(1, n_random_iters=-1) == call(1, n_estimation_iters=-1) == reason["iter_counts"]
    assert call(0, adapthalfwin=0, n_random_iters=21) == reason["batch_size"]      # in this order
    assert call(1, adapthalfwin=0, n_random_iters=21) == reason["half_window"]


def test_the_items_of_a_batch(lib, reason):
    ok = (reason["ok"], -1)
    assert check_items(lib, [1]) == check_items(lib, [16]) == check_items(lib, [8, 1, 5]) == ok
    assert check_items(lib, [9, 16]) == check_items(lib, [16, 9, 12]) == ok
    assert check_items(lib, [0]) == (reason["src_count"], 0)
    assert check_items(lib, [3, 17]) == (reason["src_count"], 1)
    assert check_items(lib, [8, 9]) == (reason["src_class"], 1)
    assert check_items(lib, [9, 10, 8]) == (reason["src_class"], 2)
    assert check_items(lib, [2, 2], null=[0, 1]) == (reason["null"], 1)
    assert check_items(lib, [2], d_min=[0.0], d_max=[1e-30]) == ok                 # d_min == 0: the `restore` variant's range
    assert check_items(lib, [2], d_min=[-0.0], d_max=[1.0]) == ok
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (-1e-30, 1.0), (float("nan"), 1.0), (1.0, float("nan"))):
        assert check_items(lib, [2, 2], d_min=[1.0, lo], d_max=[2.0, hi]) == (reason["depth_range"], 1), (lo, hi)
    # one item after the other, and within an item in this order
    assert check_items(lib, [2, 0], d_min=[3.0, 1.0], d_max=[2.0, 2.0]) == (reason["depth_range"], 0)
    assert check_items(lib, [8, 9], d_min=[1.0, 3.0], null=[0, 1]) == (reason["src_class"], 1)
    assert check_items(lib, [8, 8], d_min=[1.0, 3.0], null=[0, 1]) == (reason["null"], 1)


def test_the_image_against_the_border(lib, reason):
    def image(w, h, i=0, **kw):
        p, _ = params_pair(**kw)
        at = C.c_int()
        return lib.ep_check_image(i, w, h, C.byref(p), C.byref(at)), at.value
    ok = (reason["ok"], -1)
    assert image(16, 16) == image(16, 200) == ok                                   # 2 * 7 + 2: one pixel inside the border
    assert image(15, 16) == (reason["border"], 0) and image(16, 15, i=5) == (reason["border"], 5)
    assert image(16, 16, adapthalfwin=7) == ok and image(16, 16, adapthalfwin=8) == (reason["border"], 0)
    assert image(22, 22, adapthalfwin=10) == ok
    assert image(21, 22, adapthalfwin=10) == (reason["border"], 0) and image(22, 21, adapthalfwin=10) == (reason["border"], 0)


# ---- the knobs of the environment ----

KNOB_DEFAULTS = [1, 1, 0, -1, 0]   # HCMVS_SWEEP_LAG, HCMVS_XCD_AFFINITY, HCMVS_SWEEP_LAUNCHES, HCMVS_SWEEP_SEGMENT, HCMVS_WAVES_PER_ROW


def knobs(lib, *texts):
    out = (C.c_int * 5)()
    lib.ep_knobs(*[None if t is None else t.encode() for t in texts], out)
    return list(out)


def one_knob(lib, i, text):
    t = [None] * 5
    t[i] = text
    got = knobs(lib, *t)
    assert got[:i] + got[i + 1:] == KNOB_DEFAULTS[:i] + KNOB_DEFAULTS[i + 1:]      # a knob changes nothing but itself
    return got[i]


def test_knobs_unset_valid_and_ignored(lib):
    assert knobs(lib, None, None, None, None, None) == KNOB_DEFAULTS
    assert knobs(lib, "3", "0", "one", "128", "4") == [3, 0, 2, 128, 4]
    # HCMVS_SWEEP_LAG: a number >= 1
    assert [one_knob(lib, 0, t) for t in ("1", "2", "17")] == [1, 2, 17]
    assert [one_knob(lib, 0, t) for t in ("0", "-2", "", "x")] == [1] * 4
    # HCMVS_XCD_AFFINITY: any number, 0 turns it off (and so does a text that is no number)
    assert [one_knob(lib, 1, t) for t in ("1", "7", "-1")] == [1] * 3
    assert [one_knob(lib, 1, t) for t in ("0", "", "off")] == [0] * 3
    # HCMVS_SWEEP_LAUNCHES: the two words, exactly
    assert [one_knob(lib, 2, t) for t in ("per-sweep", "one")] == [1, 2]
    assert [one_knob(lib, 2, t) for t in ("both", "One", "per_sweep", "", "1", "one ")] == [0] * 6
    # HCMVS_SWEEP_SEGMENT: a number >= 0 (0 = whole rows)
    assert [one_knob(lib, 3, t) for t in ("0", "32", "256")] == [0, 32, 256]
    assert [one_knob(lib, 3, t) for t in ("-1", "-64")] == [-1] * 2
    # HCMVS_WAVES_PER_ROW: 1 .. 4
    assert [one_knob(lib, 4, t) for t in ("1", "2", "3", "4")] == [1, 2, 3, 4]
    assert [one_knob(lib, 4, t) for t in ("5", "0", "-1", "", "two")] == [0] * 5

"""View spread (--n-viewspread, DepthMap.cpp:1504-1608) on the CPU: the oracle's estimate with spread maps (oracle/hcmvs_spread.inc) against the plain one, against
itself in both visiting orders, against hand-derived known answers, its two arithmetic modes against each other (the bridge), the two
schedules of the scene-level harness against each other, and the three entry points of the C-ABI (exported and bound)."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O  # noqa: E402
import scene_oracle as SO  # noqa: E402
import test_oracle_bridge as BR  # noqa: E402
import test_oracle_schedule as SCH  # noqa: E402

synth = importlib.import_module("hc-mvs_amd.synth")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def gt_maps(views, conf=0.1):
    """the source views' analytic maps (depth, normal in their own camera frame) with a score below the keep threshold"""
    return [(v["depth"], v["normal"], np.full(v["depth"].shape, conf, np.float32)) for v in views[1:]]


def prepared(views, mode, **kw):
    """outer iteration 0 of the plain estimate: the maps outer iteration 1 starts from"""
    pts = synth.sparse_points(views, 80)
    d0, n0, dmin, dmax = SO.splat(views[0], pts)
    p0 = O.default_params(arith_mode=mode, order=O.ORDER_ROWS, n_threads=4, it_external=0, n_external_iters=3, **kw)
    d, n, c, _ = O.estimate(views, p0, dmin, dmax, d0, n0)
    return d, n, dmin, dmax


# ---- spread off / no maps == hcor_estimate; zig-zag == rows ------------------------------------------------------------------

@pytest.mark.parametrize("mode", [O.ARITH_REFERENCE, O.ARITH_DEVICE])
@pytest.mark.parametrize("order,threads", [(O.ORDER_ZIGZAG, 1), (O.ORDER_ROWS, 1), (O.ORDER_ROWS, 3), (O.ORDER_ROWS, 8)])
def test_spread_off_or_without_maps_is_hcor_estimate(mode, order, threads):
    views = synth.make_views(96, 80, 90.0, 3, seed=3)
    kw = dict(adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4)
    d, n, dmin, dmax = prepared(views, mode, **kw)
    p = O.default_params(arith_mode=mode, order=order, n_threads=threads, it_external=1, n_external_iters=3, **kw)
    want = O.estimate(views, p, dmin, dmax, d, n)
    assert same(O.estimate(views, p, dmin, dmax, d, n, maps=gt_maps(views), on=False), want)    # switched off, maps there
    assert same(O.estimate(views, p, dmin, dmax, d, n, maps=None, on=True), want)               # switched on, no maps
    assert same(O.estimate(views, p, dmin, dmax, d, n, maps=[None] * 3, on=True), want)
    small = [(m[0][:-2], m[1][:-2], m[2][:-2]) for m in gt_maps(views)]                         # maps of another size: the view does not spread
    assert same(O.estimate(views, p, dmin, dmax, d, n, maps=small, on=True), want)
    p0 = O.default_params(arith_mode=mode, order=order, n_threads=threads, it_external=0, n_external_iters=3, **kw)   # outer iteration 0
    pts = synth.sparse_points(views, 80)
    d0, n0, lo, hi = SO.splat(views[0], pts)
    assert same(O.estimate(views, p0, lo, hi, d0, n0, maps=gt_maps(views), on=True), O.estimate(views, p0, lo, hi, d0, n0))
    assert not same(O.estimate(views, p, dmin, dmax, d, n, maps=gt_maps(views), on=True), want)  # and with everything there it does something


@pytest.mark.parametrize("mode", [O.ARITH_REFERENCE, O.ARITH_DEVICE])
def test_zigzag_equals_rows_with_spread(mode):
    views = synth.make_views(96, 80, 90.0, 3, seed=5)
    kw = dict(adapthalfwin=5, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4)
    d, n, dmin, dmax = prepared(views, mode, **kw)
    maps = gt_maps(views)
    maps[1] = None      # a mixed estimate: view 1 offers nothing
    res = []
    for order, threads in [(O.ORDER_ZIGZAG, 1), (O.ORDER_ROWS, 1), (O.ORDER_ROWS, 3), (O.ORDER_ROWS, 8)]:
        p = O.default_params(arith_mode=mode, order=order, n_threads=threads, it_external=1, n_external_iters=3, **kw)
        O.stats(reset=True)
        res.append(O.estimate(views, p, dmin, dmax, d, n, maps=maps, on=True) + (O.stats(),))
    assert res[0][4][0] > 0 and res[0][4][1] > 0    # slots were scored and some accepted
    for r in res[1:]:
        assert same(r, res[0]) and r[4] == res[0][4]


# ---- known answers, each derived by hand from DepthMap.cpp:1504-1608 ---------------------------------------------------------------

W, H, F = 96, 80, 90.0


def plane_scene(C1=(0.8, 0.5, 0.1)):
    """a fronto-parallel plane z = 10 (in the reference camera's frame) seen by the reference camera at the origin and one source camera
    at C1 that looks at (0, 0, 10): rotated against the reference, so the transform of DepthMap.cpp:1590-1592 is not the identity"""
    scene = synth.Scene(7, depth0=10.0, slope=(0.0, 0.0), sphere=(0., 0., -100., 0.1), min_wavelength=3.5 * 10 / F, max_wavelength=150 * 10 / F)
    K = np.array([[F, 0, (W - 1) / 2], [0, F, (H - 1) / 2], [0, 0, 1.]])

    def cam(Cc):
        Cc = np.asarray(Cc, float)
        R = synth.look_at(Cc, np.array([0., 0., 10.])) if np.any(Cc) else np.eye(3)
        g, d, n = scene.render(K, R, Cc, W, H)
        return dict(K=K.copy(), R=R, C=Cc, gray=g, depth=d, normal=n)

    return [cam((0, 0, 0)), cam(C1)]


def project(v, x, y, depth, ref):
    X = np.array([(x - ref["K"][0, 2]) / ref["K"][0, 0] * depth, (y - ref["K"][1, 2]) / ref["K"][1, 1] * depth, depth])
    xc = v["R"] @ (ref["R"].T @ X + ref["C"] - v["C"])
    return (v["K"] @ xc)[:2] / xc[2]


def run_traced(views, x, y, mode, wrong=12.0, maps=None, on=True, hint=None, it=1, n_ext=3, a=6):
    """one forward sweep from a map that holds `wrong` everywhere (normal facing the camera), single-threaded zig-zag, pixel (x, y) traced"""
    d0 = np.full((H, W), wrong, np.float32)
    n0 = np.zeros((H, W, 3), np.float32); n0[..., 2] = -1
    kw = {}
    if hint is not None:
        kw = dict(hint_depth=O.fptr(hint[0]), hint_normal=O.fptr(hint[1]))
    p = O.default_params(adapthalfwin=a, n_estimation_iters=1, arith_mode=mode, order=O.ORDER_ZIGZAG, n_threads=1, it_external=it, n_external_iters=n_ext,
                         median_blur=0, **kw)
    O.trace(x, y); O.stats(reset=True)
    d, n, c, ev = O.estimate(views, p, 5.0, 40.0, d0, n0, maps=maps, on=on)
    tr = O.trace_rows()
    O.trace(-1, -1)
    return d, n, c, tr, O.stats()


MODES = [O.ARITH_REFERENCE, O.ARITH_DEVICE]


@pytest.mark.parametrize("mode", MODES)
def test_transformed_depth_is_the_analytic_one(mode):
    """every pixel of the source view's analytic map is a point of the plane z = 10 of the reference camera: DepthMap.cpp:1590-1592 must
    give 10, up to the float32 roundings of the stored depth and of the cast(s) (2^-23 * 10 = 1.2e-6 each; a handful of them)"""
    views = plane_scene()
    for nx, ny in [(9, 8), (40, 40), (88, 70), (0, 0)]:
        z = O.transform_depth(views[0], views[1], nx, ny, float(views[1]["depth"][ny, nx]), mode)
        assert abs(z - 10.0) < 2e-5, (nx, ny, z)
    # and for a pure translation along the axis by hand: a point at depth 7 of a camera 2 units behind the reference is at depth 5
    back = dict(views[0]); back["C"] = np.array([0., 0., 2.])
    assert O.transform_depth(back, views[0], 30, 20, 7.0, mode) == 5.0


@pytest.mark.parametrize("mode", MODES)
def test_wrong_depth_is_replaced_by_the_source_views_true_one_in_candidate_order(mode):
    """Pixel (7, 7) is the first the forward sweep visits: its neighbours hold the wrong depth 12 like itself, so propagation and the
    refinement trials (+-0.3 %) leave it near 12 with a score below thConfRand.  It projects to x1 = (10.17, 9.43) in the source view
    (computed below from the cameras), so the candidates are (10, 8), (10, 10), (9, 9), (11, 9) in that order (DepthMap.cpp:1533-1536);
    all hold the plane's true depth, which transforms to 10 in the reference camera, all below the keep threshold, so four slots are
    scored.  The first is accepted (the true plane matches almost perfectly); the other three propose the same depth with a normal that
    is at best equally good and are not accepted by `conf > nconf`... unless better -- so at least the first, and the pixel ends at 10."""
    views = plane_scene()
    x1 = project(views[1], 7, 7, 12.0, views[0])
    ix, iy = int(x1[0]), int(x1[1])
    assert (ix, iy) == (10, 9)
    d, n, c, tr, st = run_traced(views, 7, 7, mode, maps=gt_maps(views))
    pix = tr[tr[:, 0] == 0]; view = tr[tr[:, 0] == 1]; slots = tr[tr[:, 0] == 2]
    assert len(pix) == 1 and pix[0, 2] == 0 and pix[0, 3] < 0.55 * 0.9       # not through the full-random return
    assert len(view) == 1 and tuple(view[0, 1:6]) == (0, ix, iy, 4, 4)
    assert [tuple(r[2:4]) for r in slots] == [(ix, iy - 1), (ix, iy + 1), (ix - 1, iy), (ix + 1, iy)]     # the four-candidate order
    assert (slots[:, 4] == 2).all() and np.abs(slots[:, 5] - 10.0).max() < 2e-5                            # all scored, at the analytic depth
    assert slots[0, 7] == 1 and slots[0, 6] < 0.01                                                         # the first is accepted, nearly perfect
    last = slots[slots[:, 7] == 1][-1]
    assert d[7, 7] == last[5] and abs(d[7, 7] - 10.0) < 2e-5 and c[7, 7] == last[6]
    src_n = views[1]["normal"][int(last[3]), int(last[2])]
    assert np.array_equal(n[7, 7], src_n)        # view j's stored normal, in view j's frame, NOT rotated (it faces the camera: CorrectNormal leaves it)
    assert st[0] > 0 and st[2] == 0 and st[3] == 0
    off = run_traced(views, 7, 7, mode, maps=gt_maps(views), on=False)
    assert abs(off[0][7, 7] - 12.0) < 0.1        # without spread the pixel stays where it was


@pytest.mark.parametrize("mode", MODES)
def test_pixel_that_returns_through_the_full_random_branch_is_not_spread(mode):
    """with the source camera on the other side, pixel (7, 7)'s patch leaves the source image under every depth tried: its score stays at
    thRobust >= thConfRand, the six random trials do not bring it below, and ProcessPixel returns at DepthMap.cpp:1464 before the block"""
    views = plane_scene(C1=(-0.8, -0.5, 0.1))
    d, n, c, tr, st = run_traced(views, 7, 7, mode, maps=gt_maps(views))
    pix = tr[tr[:, 0] == 0]
    assert len(pix) == 1 and pix[0, 2] == 1 and pix[0, 3] >= np.float32(0.55) * np.float32(0.9)
    assert len(tr) == 1          # no view, no slot
    assert c[7, 7] == pix[0, 3]


@pytest.mark.parametrize("mode", MODES)
def test_source_pixel_at_or_above_the_keep_threshold_is_not_offered(mode):
    views = plane_scene()
    d, n, c, tr, st = run_traced(views, 7, 7, mode, maps=gt_maps(views, conf=0.55))
    slots = tr[tr[:, 0] == 2]
    assert len(slots) == 4 and (slots[:, 4] == 0).all()      # four slots, all skipped by DepthMap.cpp:1585
    assert st == (0, 0, 0, 0)
    assert abs(d[7, 7] - 12.0) < 0.1
    just_below = run_traced(views, 7, 7, mode, maps=gt_maps(views, conf=np.nextafter(np.float32(0.55), np.float32(0))))
    assert (just_below[3][just_below[3][:, 0] == 2][:, 4] == 2).all()


@pytest.mark.parametrize("mode", MODES)
def test_x1_on_the_rim_yields_no_candidates(mode):
    """7 < x1.x < W - 7 (DepthMap.cpp:1532).  The reference map holds the TRUE depth 10, so the estimate stays there; the source camera sits
    on the side that shifts the projection to the left: pixel (9, 40) projects to x = 7.54 in the source view -- (int) gives 7, on the rim,
    no candidates; its right neighbour (10, 40) projects to 8.61 -- 8, the first column inside it, four candidates.  (A 7 x 7 patch, half
    window 3: wider ones leave the source image this close to its edge, and the pixel would return through the full-random branch.)"""
    views = plane_scene(C1=(-0.8, -0.5, 0.1))
    assert int(project(views[1], 9, 40, 10.0, views[0])[0]) == 7 and int(project(views[1], 10, 40, 10.0, views[0])[0]) == 8
    for x, ncand in [(9, 0), (10, 4)]:
        d, n, c, tr, st = run_traced(views, x, 40, mode, wrong=10.0, maps=gt_maps(views), a=3)
        pix = tr[tr[:, 0] == 0]; view = tr[tr[:, 0] == 1]
        assert len(pix) == 1 and pix[0, 2] == 0 and len(view) == 1
        assert int(view[0, 2]) == int(project(views[1], x, 40, 10.0, views[0])[0])
        assert view[0, 4] == ncand and len(tr[tr[:, 0] == 2]) == ncand


@pytest.mark.parametrize("mode", MODES)
def test_smoothness_set_after_a_view_without_valid_candidates_is_empty(mode):
    """neighborsClose.Empty() runs for every spreading view (DepthMap.cpp:1523-1527), also when none of its candidates holds a depth: the
    `restore` hint scored afterwards (the last sweep of the last outer iteration) then sees an empty set, factor 1.  Without spread it sees
    the pixel's own neighbours."""
    views = plane_scene()
    hint = (np.full((H, W), 10.0, np.float32), np.tile(np.array([0, 0, -1], np.float32), (H, W, 1)).copy())
    empty = [(np.zeros((H, W), np.float32), views[1]["normal"], np.full((H, W), 0.1, np.float32))]
    d, n, c, tr, st = run_traced(views, 7, 7, mode, maps=empty, hint=hint, it=2, n_ext=3)
    view = tr[tr[:, 0] == 1]; hrow = tr[tr[:, 0] == 3]
    assert len(view) == 1 and tuple(view[0, 4:6]) == (4, 0)     # four candidates, no slot
    assert len(hrow) == 1 and hrow[0, 2] == 0                   # the hint's smoothness set is empty
    assert st == (0, 0, 0, 0)
    full = run_traced(views, 7, 7, mode, maps=gt_maps(views), hint=hint, it=2, n_ext=3)
    assert full[3][full[3][:, 0] == 3][0, 2] == 4               # ... the last view's four slots otherwise
    off = run_traced(views, 7, 7, mode, maps=empty, on=False, hint=hint, it=2, n_ext=3)
    assert len(off[3]) == 1 and off[3][0, 0] == 3 and off[3][0, 2] == 2   # spread off: the pixel's own neighbours (the two inside the 7-pixel border)


def test_candidates_outside_a_smaller_source_map_are_counted_not_read():
    """D10: candidates must lie inside view j's map.  A source view of 64 x 48 under a 96 x 80 reference image: x1 beyond its size is
    inside the reference image's rim test, so the reference would read past the map; here the candidates are counted and skipped."""
    views = plane_scene()
    small = dict(views[1])
    Ks = views[1]["K"].copy(); Ks[0, 2] = (64 - 1) / 2; Ks[1, 2] = (48 - 1) / 2
    scene = synth.Scene(7, depth0=10.0, slope=(0.0, 0.0), sphere=(0., 0., -100., 0.1), min_wavelength=3.5 * 10 / F, max_wavelength=150 * 10 / F)
    g, dd, nn = scene.render(Ks, small["R"], small["C"], 64, 48)
    small.update(K=Ks, gray=g, depth=dd, normal=nn)
    vs = [views[0], views[1], small]     # (a pixel that leaves the small view is still scored through the full-size one, so it reaches the block)
    d, n, dmin, dmax = prepared(vs, O.ARITH_DEVICE, adapthalfwin=5, n_estimation_iters=1)
    p = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=4, it_external=1, n_external_iters=3, adapthalfwin=5, n_estimation_iters=1)
    O.stats(reset=True)
    O.estimate(vs, p, dmin, dmax, d, n, maps=gt_maps(vs), on=True)
    st = O.stats()
    print("ragged: scored %d accepted %d dropped %d outside %d" % st)
    assert st[3] > 0 and st[0] > 0


# ---- the bridge: reference arithmetic against device association ----------------------------------------------------------------

BRIDGE = [
    dict(name="V3 a6 it1", n_src=3, seed=31, it=1, kw=dict(adapthalfwin=6, n_estimation_iters=3, propagate_halfwin=5, propagate_step=4)),
    dict(name="V3 a6 it2", n_src=3, seed=31, it=2, kw=dict(adapthalfwin=6, n_estimation_iters=3, propagate_halfwin=5, propagate_step=4)),
    dict(name="V10 a7 pf0.26 it1", n_src=10, seed=32, it=1, kw=dict(adapthalfwin=7, n_estimation_iters=3, photometric_flow=0.26, propagate_halfwin=5, propagate_step=4)),
    dict(name="V10 a7 pf0.26 it2", n_src=10, seed=32, it=2, kw=dict(adapthalfwin=7, n_estimation_iters=3, photometric_flow=0.26, propagate_halfwin=5, propagate_step=4)),
]


@pytest.mark.parametrize("sc", BRIDGE, ids=[s["name"] for s in BRIDGE])
def test_bridge_reference_and_device_arithmetic_agree_with_spread(sc):
    """the estimate with view spread in both arithmetic modes through outer iterations 0 .. it (spread from 1 on, the source views offering their analytic
    maps), held to the rows of tests/test_oracle_bridge.py::TOL for whole estimates"""
    views = synth.make_views(128, 96, 110.0, sc["n_src"], seed=sc["seed"])
    pts = synth.sparse_points(views, 150)
    d0, n0, dmin, dmax = SO.splat(views[0], pts)
    out = []
    for mode in MODES:
        d, n = d0, n0
        for it in range(sc["it"] + 1):
            p = O.default_params(arith_mode=mode, order=O.ORDER_ROWS, n_threads=8, it_external=it, n_external_iters=sc["it"] + 1, **sc["kw"])
            O.stats(reset=True)
            d, n, c, ev = O.estimate(views, p, dmin, dmax, d, n, maps=gt_maps(views), on=True)
        assert O.stats()[0] > 0
        out.append((d, n, c))
    m = BR.compare(out[0], out[1], views[0]["depth"], views[0]["normal"])
    print("spread bridge %-20s" % sc["name"], {k: round(x, 4) for k, x in m.items()})
    for k in ("valid_agree", "within_1pct"):
        assert m[k] >= BR.TOL[k], (k, m[k])
    for k in ("l1_mean", "l1_median", "valid_count", "accuracy"):
        assert m[k] <= BR.TOL[k], (k, m[k])
    assert m["normal_deg_median"] < 2.0


# ---- the two schedules of the scene-level harness ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SCH.CASES, ids=[c["id"] for c in SCH.CASES])
def test_batch_and_interleaved_schedules_agree_within_tolerance_with_spread(case):
    """D6's comparison with view spread on (D10): batch = every estimate of an outer iteration reads its source views' maps as the
    previous iteration left them (Jacobi), interleaved = the reference's order (live maps).  Held to D6's own TOL table; the measured
    row is in BASELINE.md section 3."""
    views, srcs, neighbors, order, init = SO.ring_scene(**case["scene"])
    kw = dict(n_external_iters=3, postfilter=True, mode=case["mode"], seed=900, adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4)
    batch = SO.densify(views, srcs, neighbors, order, init, viewspread=True, interleave=False, **kw)
    inter = SO.densify(views, srcs, neighbors, order, init, viewspread=True, interleave=True, **kw)
    m = SCH.compare(inter, batch, views)
    print("spread schedule (interleaved = a, batch = b):", {k: round(v, 4) if isinstance(v, float) else v for k, v in m.items()},
          "filled:", sum(inter["filled"]), sum(batch["filled"]), "spread:", inter["spread"], batch["spread"])
    assert inter["spread"][0] > 0 and batch["spread"][0] > 0
    assert not all(np.array_equal(inter["maps"][i][0], batch["maps"][i][0]) for i in inter["maps"])
    assert m["worst_valid_agree"] >= SCH.TOL["valid_agree"] and m["worst_within_1pct"] >= SCH.TOL["within_1pct"]
    assert abs(m["points_a"] - m["points_b"]) <= SCH.TOL[case["points"]] * m["points_a"]
    assert abs(m["acc_a"] - m["acc_b"]) <= SCH.TOL["accuracy"]


def test_scene_harness_without_spread_is_the_plain_harness():
    views, srcs, neighbors, order, init = SO.ring_scene(n=4, w=96, h=80, f=90.0, n_src=2, n_points=60)
    kw = dict(n_external_iters=2, postfilter=True, seed=5, adapthalfwin=5, n_estimation_iters=1, propagate_halfwin=5, propagate_step=4)
    a = SO.densify(views, srcs, neighbors, order, init, **kw)
    b = SO.densify(views, srcs, neighbors, order, init, viewspread=False, **kw)
    assert all(np.array_equal(x, y) for i in a["maps"] for x, y in zip(a["maps"][i], b["maps"][i])) and a["evals"] == b["evals"]


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["hcmvs_set_viewspread", "hcmvs_set_spread_maps_device", "hcmvs_get_spread_stats"]


def test_library_exports_and_binding_declares_the_view_spread_entry_points():
    binding = importlib.import_module("hc-mvs_amd.binding")
    out = subprocess.check_output(["nm", "-D", "--defined-only", binding.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "hcmvs_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in exported, s
        assert s in binding.SYMBOLS, s
        assert s + "(" in header, s
    assert C.sizeof(binding.SpreadStats) == 32
    for m in ("set_viewspread", "set_spread_maps_device", "spread_stats"):
        assert callable(getattr(binding.Context, m))
    import inspect
    dist = importlib.import_module("hc-mvs_amd.distributed")
    assert inspect.signature(dist.densify_scene).parameters["viewspread"].default is False

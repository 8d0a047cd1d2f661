"""The geometric-consistency term on the CPU: the oracle variant's term-level function (tests/oracle_geo.c)
against an independent numpy statement in double on hand-built pairs -- a fronto-parallel plane with the neighbour's analytic depth, a
neighbour depth off by a known factor, every neutral cause, e just below and at max_px -- the weight rule, the blend, the variant's
estimate without the term against the oracle itself, and what the term does to a low-contrast region (measured, then pinned: the oracle
is deterministic)."""
import importlib

import numpy as np
import pytest

import geo_cases as GC
import oracle_geo_lib as G
import oracle_lib as O
import scene_oracle as SO
import scene_oracle_geo as SG

synth = importlib.import_module("hc-mvs_amd.synth")
f32 = np.float32
Z = 10.0            # the plane z = Z of the reference camera (R = I, C = 0)
NORMAL = np.array([0.0, 0.0, -1.0])


@pytest.fixture(scope="module")
def cams():
    views = synth.make_views(96, 80, 90.0, 2, seed=4)
    return views[0], views[1]


def plane_maps(src, h=80, w=96, factor=1.0):
    """view j's analytic depth and normal maps of the plane z = Z (world = the reference camera's frame), depth times `factor`"""
    K, R, C = (np.asarray(src[k], np.float64) for k in ("K", "R", "C"))
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ray = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1) @ R      # R^T ray, world
    z = (Z - C[2]) / ray[..., 2]
    n = np.broadcast_to(R @ NORMAL, (h, w, 3))
    return (z * factor).astype(np.float32), np.ascontiguousarray(n, np.float32), np.zeros((h, w), np.float32)


def by_hand(ref, src, maps, x, y, depth=Z, normal=NORMAL):
    """steps 1-4 of D14 in numpy, in double, from the two cameras: x1, (u, v), e, c"""
    Ki, Ri, Ci = (np.asarray(ref[k], np.float64) for k in ("K", "R", "C"))
    Kj, Rj, Cj = (np.asarray(src[k], np.float64) for k in ("K", "R", "C"))
    # the pixel's point on the hypothesis' plane (depth at the pixel itself), into view j
    X = Ri.T @ (np.linalg.inv(Ki) @ np.array([x, y, 1.0]) * depth) + Ci
    q = Kj @ Rj @ (X - Cj)
    x1 = q[:2] / q[2]
    u, v = int(np.floor(x1[0] + 0.5)), int(np.floor(x1[1] + 0.5))
    z = float(maps[0][v, u])
    Xc = np.array([(x1[0] - Kj[0, 2]) * z / Kj[0, 0], (x1[1] - Kj[1, 2]) * z / Kj[1, 1], z])
    p = Ki @ Ri @ (Rj.T @ Xc + Cj - Ci)
    e = float(np.hypot(x - p[0] / p[2], y - p[1] / p[2]))
    m = Ri @ Rj.T @ maps[1][v, u].astype(np.float64)
    c = min(1.0, abs(float(normal @ m)) / float(np.sqrt((normal @ normal) * (m @ m))))
    return x1, (u, v), e, c


def test_a_fronto_parallel_plane_with_the_neighbours_analytic_depth_is_consistent(cams):
    ref, src = cams
    maps = plane_maps(src)
    for x, y in ((48, 40), (20, 15), (80, 60), (33, 61)):
        r = G.pair(ref, src, maps, x, y, Z, NORMAL)
        x1, _, e, c = by_hand(ref, src, maps, x, y)
        assert r["cls"] == "consistent"
        assert abs(r["x1"][0] - x1[0]) < 1e-3 and abs(r["x1"][1] - x1[1]) < 1e-3
        assert r["e"] < 5e-3 and abs(r["e"] - e) < 5e-3           # e ~ 0: what is left is the float arithmetic at |X| ~ 10
        assert abs(r["c"] - 1.0) < 1e-6 and abs(c - 1.0) < 1e-9
        assert r["geo"] < 5e-3 / 3.0 + 1e-6 and r["geo"] == float(f32(f32(r["e"]) / f32(3.0)) + (f32(1.0) - f32(r["c"])))


def test_a_neighbour_depth_off_by_a_known_factor_gives_the_error_computed_by_hand(cams):
    ref, src = cams
    for factor in (1.05, 0.9, 1.2):
        maps = plane_maps(src, factor=factor)
        for x, y in ((48, 40), (25, 55)):
            r = G.pair(ref, src, maps, x, y, Z, NORMAL, max_px=100.0)
            _, _, e, c = by_hand(ref, src, maps, x, y)
            assert r["cls"] == "consistent" and e > 0.05
            assert abs(r["e"] - e) < 2e-3 and abs(r["c"] - c) < 1e-5
            assert abs(r["geo"] - (e / 100.0 + 1.0 - c)) < 1e-4
    # a tilted neighbour normal: the cosine term
    maps = plane_maps(src)
    t = np.deg2rad(30.0)
    tilted = np.asarray(src["R"], np.float64) @ np.array([np.sin(t), 0.0, -np.cos(t)])
    maps = (maps[0], np.ascontiguousarray(np.broadcast_to(tilted, (80, 96, 3)), np.float32), maps[2])
    r = G.pair(ref, src, maps, 48, 40, Z, NORMAL)
    assert abs(r["c"] - np.cos(t)) < 1e-5 and abs(r["geo"] - (r["e"] / 3.0 + 1.0 - np.cos(t))) < 1e-5


def test_e_just_below_and_at_max_px(cams):
    ref, src = cams
    maps = plane_maps(src, factor=1.2)
    e = f32(G.pair(ref, src, maps, 48, 40, Z, NORMAL, max_px=100.0)["e"])
    assert e > 0.5
    at = G.pair(ref, src, maps, 48, 40, Z, NORMAL, max_px=float(e))
    assert at["cls"] == "worst" and at["geo"] == 2.0                                    # e == max_px: at and beyond it a pair is worst
    above = float(np.nextafter(e, f32(np.inf)))
    below = G.pair(ref, src, maps, 48, 40, Z, NORMAL, max_px=above)
    assert below["cls"] == "consistent" and below["geo"] == float(f32(e / f32(above)) + (f32(1.0) - f32(below["c"]))) and 0.99 < below["geo"] < 1.01
    assert G.pair(ref, src, maps, 48, 40, Z, NORMAL, max_px=float(np.nextafter(e, f32(0))))["cls"] == "worst"


def test_every_neutral_cause(cams):
    ref, src = cams
    maps = plane_maps(src)
    assert G.pair(ref, src, None, 48, 40, Z, NORMAL) == dict(geo=1.0, cls="nomaps", e=0.0, c=0.0, x1=G.pair(ref, src, maps, 48, 40, Z, NORMAL)["x1"])
    # outside view j's map: a hypothesis so close to the camera that the parallax carries the pixel out of the image
    r = G.pair(ref, src, maps, 48, 40, Z / 40.0, NORMAL)
    assert r["cls"] == "outside" and r["geo"] == 1.0 and not (0 <= r["x1"][0] < 96 and 0 <= r["x1"][1] < 80)
    # view j's depth there is not finite and > 0 (D11's validity rule)
    _, (u, v), _, _ = by_hand(ref, src, maps, 48, 40)
    for bad in (0.0, -3.0, np.nan, np.inf, -np.inf):
        d = maps[0].copy(); d[v, u] = bad
        r = G.pair(ref, src, (d, maps[1], maps[2]), 48, 40, Z, NORMAL)
        assert r["cls"] == "nodepth" and r["geo"] == 1.0
    # degenerate normals: view j's is zero, the hypothesis' is zero
    n = maps[1].copy(); n[v, u] = 0
    assert G.pair(ref, src, (maps[0], n, maps[2]), 48, 40, Z, NORMAL)["cls"] == "behind"
    assert G.pair(ref, src, maps, 48, 40, Z, np.zeros(3))["geo"] == 1.0
    # behind the reference camera: view j stands at (0, 0, 2 Z) and looks back; a depth of 3 Z in its map is a point at z = -Z
    back = dict(src, R=np.diag([-1.0, 1.0, -1.0]), C=np.array([0.0, 0.0, 2 * Z]))
    bm = plane_maps(back)
    ok = G.pair(ref, back, bm, 40, 36, Z, NORMAL)
    assert ok["cls"] == "consistent" and ok["e"] < 5e-3
    far = (bm[0] * f32(3.0), bm[1], bm[2])
    r = G.pair(ref, back, far, 40, 36, Z, NORMAL)
    assert r["cls"] == "behind" and r["geo"] == 1.0


def test_the_weight_rule_and_the_blend():
    kw = dict(para_tapa=0.25, para_tapa2=0.15, txthreshold=150.0, txthreshold2=160.0)
    assert [G.weight(g, **kw) for g in (0, 149, 150, 159, 160, 255)] == [0.25, 0.25, float(f32(0.15)), float(f32(0.15)), 0.0, 0.0]
    assert G.weight(10, para_tapa=0.3, para_tapa2=0.2, txthreshold=-1.0, txthreshold2=-0.5) == 0.0
    rng = np.random.default_rng(3)
    for _ in range(200):
        s, w, geo = f32(rng.uniform(0, 1.2)), f32(rng.uniform(0, 1)), f32(rng.uniform(0, 2))
        assert G.blend(s, w, geo) == float(f32(s * f32(f32(1) - w)) + f32(w * geo))     # 1 - w rounded once, nothing fused
    assert G.blend(0.5, 0.0, 2.0) == 0.5


@pytest.fixture(scope="module")
def small():
    views = GC.make_views(96, 80, 3, 13)
    d, n, dmin, dmax = GC.start(views, 13)
    maps = [GC.neighbour_maps(v, 13 + i) for i, v in enumerate(views[1:])]
    return views, d, n, dmin, dmax, maps


def test_without_the_term_the_variant_is_the_oracle(small):
    """the bodies the variant restates are the oracle's: off, w = 0 everywhere, it_external < photo2geo and no maps each give the
    oracle's own estimate bit for bit, with its evaluation count"""
    views, d, n, dmin, dmax, maps = small
    tx = GC.thresholds(views[0]["gray"])
    for it_external in (0, 1, 2):
        po = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, adapthalfwin=6, n_estimation_iters=2, it_external=it_external,
                              n_external_iters=3, seed=43, **GC.KW)
        want = O.estimate(views, po, dmin, dmax, d, n)
        for geo, m in ((None, maps), (dict(on=0, photo2geo=0), maps), (dict(on=1, photo2geo=0, txthreshold=-1.0, txthreshold2=-0.5), maps),
                       (dict(on=1, photo2geo=it_external + 1), maps), (dict(on=1, photo2geo=0), None)):
            got = G.estimate(views, po, dmin, dmax, d, n, maps=m, geo=geo)
            assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3]["evals"] == want[3]
            assert got[3]["evals_geo"] == 0 and got[3]["pixels_geo"] == 0
    # ... and with it, the cases' conditions hold and the counters add up
    po = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3,
                          seed=43, **GC.KW)
    got = G.estimate(views, po, dmin, dmax, d, n, maps=maps, geo=dict(on=1, photo2geo=1, max_px=1.0, txthreshold=tx[0], txthreshold2=tx[1]))
    plain = O.estimate(views, po, dmin, dmax, d, n)
    n_est = (96 - 14) * (80 - 14)
    GC.conditions(got[3], n_est, int((got[0] != plain[0]).sum()))
    assert got[3]["pixels_geo"] == got[3]["pixels_w"][0] + got[3]["pixels_w"][1] and 0 < got[3]["evals_geo"] < got[3]["evals"]


# Measured on the CPU oracle variant: a ring of three 96 x 80 views, every one a reference image, three outer iterations of two sweeps;
# image 0 has the contrast of one region scaled to 5 %.  The share of the region's pixels within 1 % of the analytic depth:
#   without the term 0.2550, with the defaults (0.25 / 0.15, photo2geo 2: one outer iteration blends) 0.3161, with the authors'
#   0.26 / 0.26 and photo2geo 1 (two outer iterations blend) 0.3835.  Over all estimated pixels of the three images: 0.7439, 0.7498, 0.7577.
QUALITY = {"off": (0.2550, 0.7439), "defaults": (0.3161, 0.7498), "authors": (0.3835, 0.7577)}


def test_the_term_pulls_a_low_contrast_region_towards_the_agreed_depth():
    views, srcs, _, _, init = SO.ring_scene(n=3, w=96, h=80, f=90.0, n_points=80)
    views = {i: dict(v) for i, v in views.items()}
    g = views[0]["gray"].copy(); reg = (slice(24, 56), slice(28, 72))
    g[reg] = g[reg].mean() + (g[reg] - g[reg].mean()) * 0.05
    views[0]["gray"] = g.astype(np.float32)
    kw = dict(adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4)
    got = {}
    for name, geo in (("off", None), ("defaults", dict()), ("authors", dict(para_tapa=0.26, para_tapa2=0.26, photo2geo=1))):
        r = SG.densify(views, srcs, init, geo, n_external_iters=3, seed=900, **kw)
        ok = {i: (r["maps"][i][0] > 0) & (np.abs(r["maps"][i][0] - views[i]["depth"]) < 0.01 * views[i]["depth"]) for i in views}
        got[name] = (float(ok[0][reg].mean()), float(np.mean([ok[i][7:-7, 7:-7].mean() for i in views])))
        print("%-8s within 1 %%: region %.4f, all images %.4f" % (name, got[name][0], got[name][1]))
    for name, want in QUALITY.items():
        assert abs(got[name][0] - want[0]) < 1e-4 and abs(got[name][1] - want[1]) < 1e-4, (name, got[name], want)

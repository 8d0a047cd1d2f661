"""The scenes of tests/view_select_scenes.py, on the CPU and with the oracle alone: the oracle reaches every branch of the view selection
on them, and they meet the conditions under which a float32 device result can be compared with numpy (tests/test_gpu_view_select.py
does that): per-point viewing angles >= 2 degrees, <= 512 shared points per pair, projections >= 1e-3 px from image edges and cell lines,
every threshold comparison with a relative margin >= 4e-3 -- four times the score tolerance of the device test.  This test guards the
inputs, not the feature."""
import numpy as np
import pytest

import view_select_scenes as VS

SV = VS.SV
F32 = np.float32
MARGIN = 4e-3


def rel_margin(x, t):
    return abs(x - t) / abs(t)


def pair_terms(scene):
    """(A, B, angle, footprint ratio) of every scored (point, A, B), with the oracle's formulas"""
    out = []
    for X, views in scene.verts:
        for a in views:
            A = scene.cams[a]
            fp1 = F32(A["K"][0, 0] / SV._w2c(A, X)[2])
            for b in views:
                if b != a:
                    B = scene.cams[b]
                    out.append((a, b, VS.point_angle(scene.cams, X, a, b), float(fp1 / F32(B["K"][0, 0] / SV._w2c(B, X)[2]))))
    return out


@pytest.mark.parametrize("name", sorted(VS.SCENES))
def test_scene_is_comparable_in_float32(name):
    scene = VS.SCENES[name]()
    assert 6 <= len(scene.cams) <= 16 and 200 <= len(scene.verts) <= 3000
    for X, views in scene.verts:
        assert views == sorted(set(views)) and all(scene.cams[v] is not None for v in views)
        assert VS.point_ok(scene.cams, scene.sizes, X, views)           # angles >= 2 degrees, projections off the edges and cell lines
    lo, hi = float(F32(np.deg2rad(F32(3.0)))), float(F32(np.deg2rad(F32(65.0))))
    for i, sel in enumerate(VS.oracle_scene(name)):
        cand = sel["candidates"]
        assert all(n["points"] <= 512 for n in cand)
        for n in cand:                                                   # FilterNeighborViews' comparisons
            assert min(rel_margin(n["angle"], lo), rel_margin(n["angle"], hi)) >= MARGIN, (i, n)
            assert min(rel_margin(n["scale"], 0.2), rel_margin(n["scale"], 3.2)) >= MARGIN, (i, n)
        for a, b in zip(cand, cand[1:]):                                 # the order of the sort
            assert a["score"] > 0 and (a["score"] - b["score"]) / a["score"] >= MARGIN, (i, a, b)
        nb = sel["neighbors"]
        if nb:
            f_min = nb[0]["score"] * (0.3 * 0.1)
            for n in nb:
                assert rel_margin(n["score"], f_min) >= MARGIN, (i, n)   # the InitViews cut
                assert rel_margin(abs(n["scale"] - 1.0), 0.15) >= MARGIN, (i, n)


def test_wrapper_is_the_oracles_select():
    for name in sorted(VS.SCENES):
        scene = VS.SCENES[name]()
        for i, sel in enumerate(VS.oracle_scene(name)):
            want = None if scene.cams[i] is None else SV.select(scene.cams, scene.sizes, scene.verts, i, number_views=5)
            assert (want is None) == (sel["status"] != 0)
            if want is not None:
                assert want == dict(points=sel["points"], neighbors=sel["neighbors"], srcs=sel["srcs"])


def test_the_oracle_reaches_every_branch():
    ring, small = VS.ring(), VS.small()
    terms = pair_terms(ring) + pair_terms(small)
    r = np.array([t[3] for t in terms]); ang = np.array([t[2] for t in terms])
    assert (r > 1.6).any() and ((r >= 1) & (r <= 1.6)).any() and (r < 1).any()          # the three wScale branches
    f_optim = float(F32(np.deg2rad(F32(10.0))))
    assert (ang >= f_optim * 1.01).any() and (ang <= f_optim * 0.99).any()               # wAngle saturated and not
    assert ang.min() >= VS.MIN_POINT_ANGLE
    R, S = VS.oracle_scene("ring"), VS.oracle_scene("small")
    lo = float(F32(np.deg2rad(F32(3.0))))

    def dropped(sel):
        kept = {n["id"] for n in sel["neighbors"]}
        return [n for n in sel["candidates"] if n["id"] not in kept]

    # a neighbour resampled, and one that is not
    assert any(s != 1.0 for sel in R for _, s in sel["srcs"]) and any(s == 1.0 for sel in R for _, s in sel["srcs"])
    # dropped for the angle, for the scale bound (both bounds), for the area
    assert any(n["id"] == 12 and n["angle"] < lo for n in dropped(R[3]))
    assert any(n["id"] == 13 and n["scale"] >= 3.2 for n in dropped(R[5]))
    hi = float(F32(np.deg2rad(F32(65.0))))
    assert R[13]["status"] == 2 and R[13]["candidates"] and all(n["scale"] < 0.2 or n["angle"] >= hi for n in R[13]["candidates"])
    assert any(n["scale"] < 0.2 for n in R[13]["candidates"]) and any(n["angle"] >= hi for n in R[13]["candidates"])
    assert any(n["id"] == 3 and n["area"] < 0.01 and n["points"] >= 3 for n in dropped(S[0]))
    # more candidates than nMaxViews, and the cut itself
    passing = SV.filter_neighbor_views(R[5]["candidates"], n_max_views=64)
    assert len(R[5]["candidates"]) > 12 and len(passing) > 12 and len(R[5]["neighbors"]) == 12
    # the number-views cut and the score-ratio cut
    assert len(R[5]["srcs"]) == 5 and R[5]["neighbors"][5]["score"] >= R[5]["neighbors"][0]["score"] * 0.03
    cut = S[1]
    assert cut["status"] == 0 and len(cut["srcs"]) < min(5, len(cut["neighbors"]))
    assert cut["neighbors"][len(cut["srcs"])]["score"] < cut["neighbors"][0]["score"] * 0.03
    # an image with <= 3 points, an uncalibrated image, points seen by one view only, every status
    assert S[5]["status"] == 1 and len(S[5]["points"]) <= 3
    assert ring.cams[15] is None and R[15]["status"] == 3
    assert sum(len(v[1]) == 1 for v in ring.verts) >= 6 and sum(len(v[1]) == 1 for v in small.verts) >= 6
    assert {sel["status"] for sel in R + S} == {0, 1, 2, 3}
    # projections outside an image occur (the inside test decides something)
    out = 0
    for X, views in ring.verts:
        for v in views:
            ua, va = SV._project(ring.cams[v], X)
            out += not (0 <= ua < 160 and 0 <= va < 120)
    assert out > 0

"""The numpy reference of hcmvs_estimate_point_normals (tests/normals_ref.py) against independent answers, and the conditions the
clouds of tests/test_gpu_normals.py (tests/normals_clouds.py) have to meet for that comparison to mean something: a wrong neighbour
must move the reference normal far beyond the comparison tolerance, and (next to) no point may be excluded from the comparison."""
import numpy as np
import pytest

import normals_clouds as NC
import normals_ref as NR


def angle(a, b):
    """between two lines given by unit vectors, accurate near 0"""
    return np.arcsin(np.linalg.norm(np.cross(a, b), axis=-1).clip(0, 1))


def test_neighbours_equal_a_kd_tree():
    from scipy.spatial import cKDTree
    xyz, _ = NC.cloud("a")
    idx, dist = NC.table("a")
    X = xyz.astype(np.float64)
    d, nn = cKDTree(X).query(X, k=idx.shape[1])
    assert (np.diff(dist, axis=1) > 0).all()                 # tie-free: the order is by distance alone
    assert np.array_equal(nn, idx) and (idx[:, 0] == np.arange(len(X))).all()
    assert np.abs(np.sqrt(dist) - d).max() < 1e-12


def test_ties_go_to_the_lower_index_and_n_below_k():
    # the centre and six points at distance 1 from it: the centre's three nearest are itself and the two lowest indices
    pts = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [-1, 0, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1]], np.float32)
    idx, dist = NR.neighbour_table(pts, 3)
    assert idx[2].tolist() == [2, 0, 1, 3] and dist[2].tolist() == [0, 1, 1, 1]
    assert idx[0].tolist() == [0, 2, 1, 4] and dist[0].tolist() == [0, 1, 2, 2]
    perm = np.array([6, 5, 4, 3, 2, 1, 0])
    idx, _ = NR.neighbour_table(pts[perm], 3)
    assert idx[4].tolist() == [4, 0, 1, 2]                   # the same rule in the new numbering: other points
    r = NR.reference(pts, np.array([[0.0, 0.0, 9.0]]), np.zeros(7, np.int64), 3)
    assert not r["near_tie"].any()                           # equal distances are no near tie
    # fewer points than k: all of them, the (k + 1)-th does not exist
    idx, dist = NR.neighbour_table(pts[:3], 16)
    assert idx.shape == (3, 3) and sorted(idx[1].tolist()) == [0, 1, 2]
    r = NR.reference(pts[:3], np.array([[0.3, 0.2, 9.0]]), np.zeros(3, np.int64), 16)
    assert not r["near_tie"].any() and np.abs(np.abs(r["normal"][:, 2]) - 1).max() < 1e-7 and (r["normal"][:, 2] > 0).all()


def test_masks():
    # near tie: the closest float32 coordinates, 1 and 1 + 2^-23, give squared distances a relative 2.4e-7 apart, which is none; in a
    # table handed in, a (k + 1)-th distance a relative 1e-10 above the k-th is one, 1e-8 above is none, equal is none
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1 - 2.0 ** -23]], np.float32)
    cam, first = np.array([[5.0, 4.0, 3.0]]), np.zeros(5, np.int64)
    idx, dist = NR.neighbour_table(pts, 4)
    assert not NR.reference(pts, cam, first, 4, (idx, dist))["near_tie"].any()
    for rel, want in ((1e-10, True), (1e-8, False), (0.0, False)):
        d = dist.copy(); d[0, 4] = d[0, 3] * (1 + rel)
        assert NR.reference(pts, cam, first, 4, (idx, d))["near_tie"].tolist() == [want] + [False] * 4
    # ill-conditioned: collinear neighbours, and all neighbours in one place; grazing: the camera in the plane of the neighbours
    line = np.array([[t, 2 * t, -t] for t in range(5)], np.float32)
    assert NR.reference(line, np.array([[0.0, 0.0, 9.0]]), np.zeros(5, np.int64), 3)["ill_conditioned"].all()
    assert NR.reference(np.ones((4, 3), np.float32), np.array([[0.0, 0.0, 9.0]]), np.zeros(4, np.int64), 3)["ill_conditioned"].all()
    square = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    r = NR.reference(square, np.array([[7.0, 3.0, 0.0], [7.0, 3.0, 0.01]]), np.array([0, 0, 1, 1]), 4)
    assert r["grazing"].tolist() == [True, True, False, False] and not r["ill_conditioned"].any()
    assert (r["normal"][2:, 2] == 1).all()                   # and the flip towards the camera of the point's own view


def test_exact_plane():
    # z = 0.5 x + 0.25 y on dyadic x, y: exact in float32; the cameras above it
    rng = np.random.RandomState(0)
    xy = rng.randint(-512, 512, (800, 2)) / 256.0
    pts = np.concatenate([xy, 0.5 * xy[:, :1] + 0.25 * xy[:, 1:]], 1).astype(np.float32)
    want = np.array([-0.5, -0.25, 1.0]) / np.sqrt(1.3125)
    first = rng.randint(0, 3, 800)
    for k in (3, 16, 32):
        r = NR.reference(pts, NC.CENTRES, first, k)
        ok = ~r["ill_conditioned"]                           # three random neighbours may be collinear
        assert ok.mean() > 0.95 and not r["grazing"].any()
        assert np.abs(r["normal"][ok] - want.astype(np.float32)).max() <= 2.0 ** -24
        assert angle(r["normal64"][ok], want).max() < 1e-11
    below = NR.reference(pts, np.array([[0.0, 0.0, -30.0]]), np.zeros(800, np.int64), 16)
    assert np.abs(below["normal"] + want.astype(np.float32)).max() <= 2.0 ** -24


def test_sphere():
    """a Fibonacci lattice on the unit sphere, the camera at its centre: the normal is -p up to the tilt of a least-squares plane through
    a cap of radius r whose points lie r^2 / 2 at most under the tangent plane: below r, the distance to the k-th neighbour"""
    n, k = 3000, 16
    i = np.arange(n) + 0.5
    phi = np.pi * (1 + 5 ** 0.5) * i
    z = 1 - 2 * i / n
    pts = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1).astype(np.float32)
    idx, dist = NR.neighbour_table(pts, k)
    r = NR.reference(pts, np.zeros((1, 3)), np.zeros(n, np.int64), k, (idx, dist))
    assert not (r["near_tie"] | r["ill_conditioned"] | r["grazing"]).any()
    rk = np.sqrt(dist[:, k - 1])
    assert rk.max() < 0.2
    p = pts.astype(np.float64)
    assert ((r["normal"] * p).sum(1) < -0.9).all()           # towards the centre
    assert (angle(r["normal64"], p / np.linalg.norm(p, axis=1, keepdims=True)) < rk).all()


@pytest.mark.parametrize("name,k", [(c, k) for c, k in NC.CASES if c in NC.NOISY])
def test_a_wrong_neighbour_shows(name, k):
    """what makes the comparison on the device meaningful: with the k-th neighbour replaced by the (k + 1)-th the reference normal moves
    by more than 100 times the comparison tolerance at 99 % of the compared points at least (an exact plane would hide every neighbour
    error, which is why these clouds carry noise)"""
    xyz, _ = NC.cloud(name)
    ref = NC.reference(name, k)
    idx, _ = NC.table(name)
    wrong = np.concatenate([idx[:, :k - 1], idx[:, k:k + 1]], 1)
    _, v = NR.pca(xyz, wrong)
    ok = NC.comparable(ref)
    moved = angle(v, ref["normal64"])[ok]
    print("%s k=%d: moved by median %.3g, min %.3g; above 100 tol: %.4f" % (name, k, np.median(moved), moved.min(), (moved > 100 * NC.TOL).mean()))
    assert (moved > 100 * NC.TOL).mean() >= 0.99


@pytest.mark.parametrize("name,k", NC.CAPPED)
def test_exclusion_caps(name, k):
    """conditions on the inputs: no near tie, no grazing point, at most 2 % ill-conditioned points, on every cloud of the device tests"""
    ref = NC.reference(name, k)
    n = len(ref["normal"])
    print("%s k=%d n=%d: near ties %d, grazing %d, ill-conditioned %d (%.2f %%; gap below 1e-3: %d)" % (
        name, k, n, ref["near_tie"].sum(), ref["grazing"].sum(), ref["ill_conditioned"].sum(), 100 * ref["ill_conditioned"].mean(),
        (ref["gap"] < 1e-3).sum()))
    assert ref["near_tie"].sum() == 0 and ref["grazing"].sum() == 0
    assert ref["ill_conditioned"].sum() <= NC.CAP_ILL * n
    assert np.isfinite(ref["normal"]).all() and np.abs(np.linalg.norm(ref["normal"].astype(np.float64), axis=1) - 1).max() < 1e-6


def test_clouds_outside_the_caps_are_what_they_claim():
    # d2: the lone point is the one near tie; d, d2: the lone point is the one ill-conditioned point
    for name, near in (("d", 0), ("d2", 1)):
        xyz, first = NC.cloud(name)
        ref = NC.reference(name, 16)
        lone = np.nonzero(xyz[:, 0] > 1e6)[0]
        assert len(lone) == 1 and first[lone[0]] >= 3 and (first[xyz[:, 0] < 1e6] < 3).all()
        assert np.nonzero(ref["ill_conditioned"])[0].tolist() == lone.tolist() and not ref["grazing"].any()
        assert np.nonzero(ref["near_tie"])[0].tolist() == (lone.tolist() if near else [])
    # h: exactly collinear, ill-conditioned everywhere
    xyz, _ = NC.cloud("h")
    rel = xyz.astype(np.float64) - xyz[0].astype(np.float64)
    assert np.abs(np.cross(rel, NC.LINE_DIR)).max() == 0 or np.abs(np.cross(rel, [3.0, 2.0, 1.0])).max() == 0
    assert NC.reference("h", 8)["ill_conditioned"].all() and not NC.reference("h", 8)["near_tie"].any()
    # one or two points: nothing to tie
    for name in ("i1", "i2"):
        for k in NC.CLOUDS[name][1]:
            assert not NC.reference(name, k)["near_tie"].any()


def grid_ratio(xyz, k):
    """longest side of the box over the cell edge the k-nearest search of cloud_kernels.hip starts from (sqrt(k / 2 * area / n), area
    the largest face of the box); above 1048575 the cell is enlarged to keep 20 bits per axis"""
    ext = (xyz.max(0).astype(np.float64) - xyz.min(0).astype(np.float64))
    area = max(ext[0] * ext[1], ext[0] * ext[2], ext[1] * ext[2], 1e-30)
    return ext.max() / max(np.sqrt(0.5 * k * area / len(xyz)), 1e-12)


def test_clouds_reach_what_they_are_for():
    # a: no two equal distances among the k + 1 nearest of any point, so the order of summation is the order by distance whatever the
    # input order (the premise of the order-independence test on the device)
    assert (np.diff(NC.table("a")[1], axis=1) > 0).all() and NC.table("a")[1].shape[1] == 33
    # e: exact ties at the k-th distance for every k it runs with, and the index decides them differently from the position
    idx, dist = NC.table("e")
    for k in NC.CLOUDS["e"][1]:
        tied = dist[:, k - 1] == dist[:, k]
        assert tied.sum() >= 10, (k, tied.sum())
        assert (idx[tied, k - 1] < idx[tied, k]).all()
    xyz, _ = NC.cloud("e")
    assert np.array_equal(xyz * 4, np.round(xyz * 4)) and np.abs(xyz).max() < 32
    # f: the copies are tied at distance 0 and fill whole neighbourhoods
    xyz, _ = NC.cloud("f")
    idx, dist = NC.table("f")
    assert ((dist[:, :16] == 0).all(1)).sum() == NC.N_COPIES + 1
    assert (((dist[:, 15] == dist[:, 16]) & (dist[:, 15] > 0)).sum()) >= 5       # sheet points that take SOME of the copies: by index
    # g: flat; d: the sheet lies in one cell but the 20-bit limit is not reached; d2: it is
    assert np.ptp(NC.cloud("g")[0][:, 2]) == 0
    assert grid_ratio(NC.cloud("d")[0], 16) < 1048575 < grid_ratio(NC.cloud("d2")[0], 16)
    ext = np.ptp(NC.cloud("d")[0].astype(np.float64), axis=0)
    assert np.sqrt(8 * ext[0] * ext[1] / 2001) > 100         # the cell edge against a sheet of 2 x 2
    # every view is some point's first view; n <= 8000
    for name in NC.CLOUDS:
        xyz, first = NC.cloud(name)
        assert len(xyz) <= 8000 and (len(xyz) < 50 or len(set(first.tolist()) & {0, 1, 2}) == 3)

"""The numpy restatement of Scene::PointCloudFilter (tests/visibility_ref.py) on hand-built clouds whose visibility is worked out
here: one camera at the origin looking down +z, 640 px wide with f = 500, so the cone half-angle is 2 atan(0.64) / 640 = 1.78e-3 rad
and a point on the optical axis has t = its z exactly."""
import numpy as np

import visibility_ref as V

CAM = dict(K=np.array([[500.0, 0, 319.5], [0, 500.0, 239.5], [0, 0, 1]]), R=np.eye(3), C=np.zeros(3), width=640, height=480)


def run(points, views, cameras=(CAM,), th=-1):
    xyz = np.array(points, np.float32)
    nv = np.array([len(v) for v in views], np.uint32)
    vi = np.array([j for v in views for j in v], np.uint32)
    vis = V.visibility(xyz, nv, vi, list(cameras))
    return vis, V.removal_order(vis, th)


def test_cone_half_angle():
    Cf, cosSq = V.cone(CAM)
    angle = 2 * np.arctan(640 / 1000.0) / 640
    assert abs(float(cosSq) - np.cos(angle) ** 2) < 1e-7 and Cf.dtype == np.float32
    assert V.cone(dict(CAM, width=0)) is None and V.cone(None) is None


def test_three_points_on_one_ray():
    # A (z 5), B (z 10), S (z 20): B's cone reaches A (-1 for A); S's reaches A and B; A's own cone ends at 5.1
    vis, kept = run([[0, 0, 5], [0, 0, 10], [0, 0, 20]], [[0], [0], [0]])
    assert vis.tolist() == [-2, -1, 0]
    assert kept.tolist() == [2]
    _, kept = run([[0, 0, 5], [0, 0, 10], [0, 0, 20]], [[0], [0], [0]], th=-2)
    assert kept.tolist() == [2, 1]  # A (index 0) removed: the last point moves into its place


def test_similar_and_support():
    # X at 10; P1 0.5 % behind it (similar to X both ways: no vote); P2 1.5 % behind (inside X's cone up to 10.2: +|views(P2)| = 2);
    # from P2's pair X is 1.48 % in front: -|views(P2)| = -2 for X
    vis, _ = run([[0, 0, 10], [0, 0, 10.05], [0, 0, 10.15]], [[0], [0], [0, 1]], cameras=(CAM, None))
    assert vis.tolist() == [-2, 0, 2]


def test_floater_in_front_counts_every_view_entry():
    # the floater F loses |views(X)| = 3 (the uncalibrated image 1 and the unknown image 7 still count in the weight); the skipped pairs
    # cast no vote of their own
    vis, kept = run([[0, 0, 10], [0, 0, 6]], [[0, 1, 7], [0]], cameras=(CAM, None))
    assert vis.tolist() == [0, -3]
    assert kept.tolist() == [0]
    # just outside the cone (2.0e-3 rad off X's ray) no vote; just inside (1.6e-3 rad) the vote
    vis, _ = run([[0, 0, 10], [0.010, 0, 5], [0.008, 0, 5], [0, 0, -5]], [[0], [], [], []])
    assert vis.tolist() == [0, 0, -1, 0]


def test_duplicates_and_points_without_views():
    # two copies of X: each is depth-similar to the other (no vote); the point in front loses 1 per copy; a point without views
    # votes for nothing and gains nothing when behind (|views| = 0), but loses when in front
    vis, _ = run([[0, 0, 10], [0, 0, 10], [0, 0, 5], [0, 0, 10.15], [0, 0, 4]], [[0], [0], [0], [], []])
    assert vis.tolist() == [0, 0, -2 + 0, 0, -2 - 1]


def test_thresholds():
    pts = [[0, 0, 20], [0, 0, 10], [0, 0, 5], [0, 0, 4]]
    views = [[0, 1], [0], [0], [0]]
    cams = (CAM, None)
    # z 10: -|views(z 20)| = -2; z 5: -2 - 1; z 4: -2 - 1 - 1; the point at 20 keeps 0
    vis, _ = run(pts, views, cams)
    assert vis.tolist() == [0, -2, -3, -4]
    assert run(pts, views, cams, th=-1)[1].tolist() == [0]
    assert run(pts, views, cams, th=-3)[1].tolist() == [0, 1]
    assert run(pts, views, cams, th=-5)[1].tolist() == [0, 1, 2, 3]


def test_removal_order():
    # list [0 1 2 3 4 5]: remove 5 (the last) -> [0 1 2 3 4]; remove 2 -> [0 1 4 3]; remove 0 -> [3 1 4]
    assert V.removal_order(np.array([-5, 0, -5, 0, 0, -5]), -1).tolist() == [3, 1, 4]
    assert V.removal_order(np.array([0, 0, 0]), -1).tolist() == [0, 1, 2]
    assert V.removal_order(np.array([-1, -1]), -1).tolist() == []
    assert V.removal_order(np.array([-2, -1, 0, -3]), -2).tolist() == [2, 1]

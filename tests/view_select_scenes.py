"""Deterministic sparse scenes for the view selection (hcmvs_select_views) and what the numpy oracle (oracle/select_views.py) says about
them.  Test infrastructure: nothing here is imported by the product.

Two scenes, built so that the oracle alone reaches every branch of Scene::SelectNeighborViews / FilterNeighborViews / InitViews
(tests/test_view_select_scenes.py asserts that) and so that a float32 device result can be compared with numpy at all: every point is
redrawn until its viewing angles are >= 2 degrees and its projections keep 1e-3 px from every image edge and 1/16 cell line; the seeds
are chosen so that every threshold comparison has a relative margin >= 4e-3 (asserted by the same test).

  ring   16 images of 160 x 120: twelve on an arc 4 degrees apart (wAngle saturated and not; the footprint ratio on both sides of 1), one
         2.5 degrees above image 3 (dropped for its angle < 3 degrees), one six times as far (ratio > 1.6; dropped by the scale bound, and
         itself left with no neighbour), one 1.3 times as far (resampled: |scale - 1| >= 0.15), one uncalibrated.  Image 5 and its
         neighbours have more candidates than nMaxViews = 12 and more neighbours than number-views.
  small  6 images of different sizes and focal lengths: a trio, an image that shares with image 0 only a cluster of four points in one
         cell (dropped for its area < 0.01), an image with five points (its score is below 3 % of the best: the score-ratio cut), an image
         with three points (SelectNeighborViews fails), points seen by one view only.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import select_views as SV  # noqa: E402

F32 = np.float32
MIN_POINT_ANGLE = np.deg2rad(2.0)
PX_MARGIN = 1e-3


def look_at(C, f, w, h, target=(0.0, 0.0, 0.0)):
    C = np.asarray(C, np.float64)
    z = np.asarray(target, np.float64) - C; z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return dict(K=np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1.0]]), R=np.stack([x, y, z]), C=C)


def on_sphere(dist, az_deg, el_deg):
    az, el = np.deg2rad(az_deg), np.deg2rad(el_deg)
    return np.array([dist * np.sin(az) * np.cos(el), dist * np.sin(el), -dist * np.cos(az) * np.cos(el)])


def point_angle(cams, X, a, b):
    V1 = (cams[a]["C"] - X.astype(np.float64)).astype(F32); V2 = (cams[b]["C"] - X.astype(np.float64)).astype(F32)
    return float(np.arccos(np.clip(np.dot(V1, V2) / np.sqrt(np.dot(V1, V1) * np.dot(V2, V2)), -1, 1)))


def projection_margin(cam, size, X):
    """distance in px of the projection of X from the nearest image edge or 1/16 cell line, in u and in v (inf behind the camera)"""
    q = cam["K"] @ (cam["R"] @ (X.astype(np.float64) - cam["C"]))
    if q[2] <= 0:
        return np.inf if q[2] < -1e-6 else 0.0
    m = np.inf
    for c, n in ((q[0] / q[2], size[0]), (q[1] / q[2], size[1])):
        lines = np.arange(17) * (n / 16.0)
        m = min(m, float(np.min(np.abs(lines - c))))
    return m


def point_ok(cams, sizes, X, views):
    """the per-point conditions under which float32 on the device and numpy make the same integer decisions"""
    for i, a in enumerate(views):
        if projection_margin(cams[a], sizes[a], X) < PX_MARGIN:
            return False
        for b in views[i + 1:]:
            if point_angle(cams, X, a, b) < MIN_POINT_ANGLE:
                return False
    return True


class Scene:
    def __init__(self, name, cams, sizes, verts):
        self.name, self.cams, self.sizes, self.verts = name, cams, sizes, verts
        self._snv = {}

    def neighbor_views(self, ID, n_min_views=2, n_min_point_views=2):
        """the oracle's select_neighbor_views for image ID, computed once (it does not depend on the filter's or the cut's parameters)"""
        key = (ID, n_min_views, n_min_point_views)
        if key not in self._snv:
            self._snv[key] = SV.select_neighbor_views(self.cams, self.sizes, self.verts, ID, n_min_views=n_min_views, n_min_point_views=n_min_point_views)
        points, cand, ok = self._snv[key]
        return list(points), [dict(n) for n in cand], ok

    def csr(self):
        xyz = np.ascontiguousarray(np.stack([v[0] for v in self.verts]), np.float32)
        nv = np.array([len(v[1]) for v in self.verts], np.uint32)
        ids = np.array([j for v in self.verts for j in v[1]], np.uint32)
        return xyz, nv, ids


def _draw(rng, cams, sizes, views, box, centre=(0.0, 0.0, 0.0)):
    """a point of the box seen by `views` that meets point_ok: redrawn until it does"""
    for _ in range(1000):
        X = (np.asarray(centre) + rng.uniform(-1, 1, 3) * np.asarray(box)).astype(F32)
        if point_ok(cams, sizes, X, views):
            return X
    raise AssertionError("no admissible point for views %s" % (views,))


RING_SEED, SMALL_SEED = 3, 1


@functools.lru_cache(maxsize=None)
def ring(seed=RING_SEED):
    w, h, f = 160, 120, 380.0
    cams = [look_at(on_sphere(10.0, (i - 5.5) * 4.0, 0.0), f, w, h) for i in range(12)]
    cams.append(look_at(on_sphere(10.0, (3 - 5.5) * 4.0, 2.5), f, w, h))     # 12: 2.5 degrees above image 3
    cams.append(look_at(on_sphere(60.0, 34.0, 14.0), f, w, h))               # 13: six times as far
    cams.append(look_at(on_sphere(13.0, -34.0, -12.0), f, w, h))             # 14: 1.3 times as far
    cams.append(None)                                                        # 15: uncalibrated
    sizes = [(w, h)] * 16
    rng = np.random.RandomState(seed)
    verts = []
    for _ in range(520):
        n = rng.randint(2, 8)
        s = rng.randint(0, 13 - n)
        views = list(range(s, s + n))
        for extra, prob in ((12, 0.35), (13, 0.3), (14, 0.35)):
            if rng.uniform() < prob:
                views.append(extra)
        verts.append((_draw(rng, cams, sizes, views, (2.3, 1.8, 1.0)), sorted(views)))
    for i in (2, 9, 14):                                                     # points seen by one view only
        for _ in range(6):
            verts.append((_draw(rng, cams, sizes, [i], (1.6, 1.4, 1.0)), [i]))
    return Scene("ring", cams, sizes, verts)


@functools.lru_cache(maxsize=None)
def small(seed=SMALL_SEED):
    sizes = [(200, 90), (160, 120), (176, 144), (160, 120), (128, 96), (160, 120)]
    focal = [420.0, 460.0, 400.0, 380.0, 300.0, 380.0]
    at = [(10.0, -7.0, 0.0), (10.0, 0.0, 1.0), (11.0, 7.0, -1.0), (10.0, 15.0, 4.0), (9.5, -15.0, -5.0), (10.0, 3.0, 9.0)]
    cams = [look_at(on_sphere(*p), fo, *sz) for p, fo, sz in zip(at, focal, sizes)]
    rng = np.random.RandomState(seed)
    verts = []
    for k in range(170):                                                     # the trio
        views = [[0, 1, 2], [0, 1], [1, 2], [0, 2]][k % 4]
        verts.append((_draw(rng, cams, sizes, views, (1.2, 0.6, 0.8)), views))
    for _ in range(45):                                                      # image 3 with images 1 and 2
        verts.append((_draw(rng, cams, sizes, [1, 2, 3], (1.0, 0.6, 0.6)), [1, 2, 3]))
    for _ in range(4):                                                       # ... and with image 0 a cluster inside one cell: area 1 / 256
        verts.append((_draw(rng, cams, sizes, [0, 3], (0.02, 0.02, 0.02), centre=(0.1, 0.05, 0.0)), [0, 3]))
    for k in range(5):                                                       # image 4: five points with images 1 and 2
        verts.append((_draw(rng, cams, sizes, [1, 2, 4], (0.9, 0.5, 0.5)), [1, 2, 4]))
    for _ in range(3):                                                       # image 5: three points
        verts.append((_draw(rng, cams, sizes, [0, 1, 5], (0.9, 0.5, 0.5)), [0, 1, 5]))
    for i in (0, 2):                                                         # points seen by one view only
        for _ in range(5):
            verts.append((_draw(rng, cams, sizes, [i], (1.2, 0.6, 0.8)), [i]))
    order = rng.permutation(len(verts))                                      # the kinds interleaved, as a real cloud has them
    return Scene("small", cams, sizes, [verts[i] for i in order])


SCENES = {"ring": ring, "small": small}


def avg_depth(scene, ID):
    """Image::avgDepth (Scene.cpp:565, :575, :603): float(PointDepth) summed into a float in point order, over nPoints"""
    s, n = F32(0), 0
    for X, views in scene.verts:
        if ID in views:
            s = F32(s + F32(SV._w2c(scene.cams[ID], X)[2])); n += 1
    return n, (float(F32(s / F32(n))) if n else 0.0)


def oracle_select(scene, ID, number_views=5, n_min_views=2, n_min_point_views=2, n_max_views=12):
    """SelectViews + the InitViews cut for image ID from the oracle's three steps, with what the C-ABI reports beside them:
    dict(status, points, candidates [before the filter], neighbors, srcs, n_seen, avg_depth); status as hcmvs_view_selection.status"""
    if scene.cams[ID] is None:
        return dict(status=3, points=[], candidates=[], neighbors=[], srcs=[], n_seen=0, avg_depth=0.0)
    points, cand, ok = scene.neighbor_views(ID, n_min_views, n_min_point_views)
    n_seen, avg = avg_depth(scene, ID)
    out = dict(points=points, candidates=cand, neighbors=[], srcs=[], n_seen=n_seen, avg_depth=avg)
    if not ok:
        return dict(out, status=1)
    nb = SV.filter_neighbor_views(cand, n_max_views=n_max_views)
    srcs = SV.init_views(nb, number_views) if nb else []
    return dict(out, neighbors=nb, srcs=srcs, status=0 if srcs else 2)


@functools.lru_cache(maxsize=None)
def oracle_scene(name, number_views=5, n_max_views=12):
    """oracle_select of every image of a scene, computed once per process"""
    scene = SCENES[name]()
    return [oracle_select(scene, i, number_views=number_views, n_max_views=n_max_views) for i in range(len(scene.cams))]

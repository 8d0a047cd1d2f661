"""The visibility filter of a finished cloud on the device (hcmvs_point_cloud_filter, DensifyPointCloud --filter-point-cloud < 0)
against the numpy restatement of Scene::PointCloudFilter (tests/visibility_ref.py): visibility sums and the kept order equal, bit for bit."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import scene_files
import visibility_ref as V

pytestmark = pytest.mark.gpu

binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")
mvsio = importlib.import_module("hc-mvs_amd.mvsio")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hc-mvs_amd", "DensifyPointCloud")


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def project(cam, X):
    p = (np.asarray(X, np.float64) - cam["C"]) @ np.asarray(cam["R"]).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return cam["K"][0, 0] * p[:, 0] / p[:, 2] + cam["K"][0, 2], cam["K"][1, 1] * p[:, 1] / p[:, 2] + cam["K"][1, 2], p[:, 2]


def small_cloud(n_cams, case, seed=1):
    """about 5 k surface points with exact view lists on a synthetic scene, floaters in front of the surface, points just behind it,
    and the variation `case` asks for; returns xyz, n_views, view_ids, cameras, floater indices"""
    w, h = 160, 120
    views = synth.make_views(w, h, 150.0, n_cams - 1, seed=seed, baseline=(0.1, 0.3))
    verts = scene_files.sparse_vertices(views, 5200 // n_cams + 40, seed=seed)
    rng = np.random.RandomState(seed)
    cams = [dict(K=v["K"], R=v["R"], C=v["C"], width=w, height=h) for v in views]
    xyz = [v["X"] for v in verts]
    lists = [[j for j, _ in v["views"]] for v in verts]
    ns = len(xyz)
    floaters = []
    for k in rng.choice(ns, ns // 50, replace=False):  # floaters on the ray of one of the point's views
        j = lists[k][rng.randint(len(lists[k]))]
        floaters.append(len(xyz))
        xyz.append((views[j]["C"] + rng.uniform(0.4, 0.9) * (xyz[k] - views[j]["C"])).astype(np.float32))
        lists.append([j])
    for k in rng.choice(ns, ns // 50, replace=False):  # 1.2 - 1.9 % behind the surface along a view's ray
        j = lists[k][0]
        xyz.append((views[j]["C"] + rng.uniform(1.012, 1.019) * (xyz[k] - views[j]["C"])).astype(np.float32))
        lists.append(list(lists[k]))
    xyz = np.array(xyz, np.float32)
    if case == "margin":  # add the views in which a point falls just outside the image (inside the binned margin)
        for j, cam in enumerate(cams):
            u, v, z = project(cam, xyz)
            band = (z > 0) & (((u >= -20) & (u < -0.5)) | ((u >= w - 0.5) & (u < w + 20)) | ((v >= -20) & (v < -0.5)) | ((v >= h - 0.5) & (v < h + 20)))
            band &= (u >= -20) & (u < w + 20) & (v >= -20) & (v < h + 20)
            for k in np.nonzero(band)[0][:400]:
                if j not in lists[k]:
                    lists[k].append(j)
        assert sum(len(a) for a in lists) > 0
    elif case == "behind":  # a camera that looks away from the scene: every point is behind it (the exact path)
        C = np.array([0.3, -0.2, -1.0])
        cams.append(dict(K=views[0]["K"], R=synth.look_at(C, C + np.array([0.1, 0.05, -1.0])), C=C, width=w, height=h))
        for k in rng.choice(len(xyz), 300, replace=False):
            lists[k].append(len(cams) - 1)
    elif case == "uncalibrated":  # an image without a pose, and an id past the last image, in view lists
        cams.append(None)
        for k in rng.choice(len(xyz), 300, replace=False):
            lists[k].append(len(cams) - 1 if k % 2 else len(cams) + 3)
    elif case == "mixed":  # images of other sizes (K at that size): other cone angles and grids
        for j in range(1, len(cams), 2):
            s = 0.5 if j % 4 == 1 else 1.75
            K = cams[j]["K"].copy()
            K[0, 0] *= s; K[1, 1] *= s; K[0, 2] = (K[0, 2] + 0.5) * s - 0.5; K[1, 2] = (K[1, 2] + 0.5) * s - 0.5
            cams[j] = dict(cams[j], K=K, width=int(round(w * s)), height=int(round(h * s)))
    nv = np.array([len(a) for a in lists], np.uint32)
    vi = np.array([j for a in lists for j in a], np.uint32)
    return xyz, nv, vi, cams, np.array(floaters)


@pytest.mark.parametrize("n_cams,case", [(4, "plain"), (6, "margin"), (8, "behind"), (10, "uncalibrated"), (12, "mixed")])
def test_filter_is_bit_exact(ctx, n_cams, case):
    xyz, nv, vi, cams, floaters = small_cloud(n_cams, case)
    assert 4000 < len(xyz) < 7000
    rvis = V.visibility(xyz, nv, vi, cams)
    for th in (-1, -3):
        vis, kept = ctx.point_cloud_filter(xyz, nv, vi, cams, th_remove=th)
        st = ctx.visibility_stats
        assert np.array_equal(vis, rvis), (case, th, np.nonzero(vis != rvis)[0][:10])
        assert np.array_equal(kept, V.removal_order(rvis, th))
        assert st["pairs"] + st["skipped_pairs"] == len(vi) and st["hits"] > 0
    # the floaters are what the filter exists for: most of them go
    assert np.isin(floaters, kept, invert=True).mean() > 0.9
    if case == "behind":
        assert st["fallback_pairs"] >= 300
    if case == "uncalibrated":
        assert st["skipped_pairs"] == 300
    if case in ("plain", "mixed"):
        assert st["fallback_pairs"] == 0


def ring_cloud(n_target, n_cams=32, w=1920, h=1080, f=1500.0, seed=7):
    """a textured-scene plane seen by a ring of 1080p cameras, each looking outward and down at its own part of it: uniform surface
    points with their exact view lists (in front, inside the image; nothing occludes a plane), plus 1 % floaters placed on the ray of
    one of their point's views"""
    scene = synth.Scene(seed)
    rng = np.random.RandomState(seed)
    cams = []
    K = np.array([[f, 0, (w - 1) / 2], [0, f, (h - 1) / 2], [0, 0, 1]])
    for i in range(n_cams):
        a = 2 * np.pi * i / n_cams
        C = np.array([3.0 * np.cos(a), 3.0 * np.sin(a), 0.0])
        tgt = np.array([6.0 * np.cos(a), 6.0 * np.sin(a), 0.0])
        tgt[2] = scene.depth0 + scene.slope[0] * tgt[0] + scene.slope[1] * tgt[1]
        cams.append(dict(K=K, R=synth.look_at(C, tgt), C=C, width=w, height=h))
    r = np.sqrt(rng.uniform(1.0, 10.0 ** 2, n_target)); a = rng.uniform(0, 2 * np.pi, n_target)
    x, y = r * np.cos(a), r * np.sin(a)
    X = np.stack([x, y, scene.depth0 + scene.slope[0] * x + scene.slope[1] * y], -1).astype(np.float32)
    seen = np.zeros((n_target, n_cams), bool)
    for j, cam in enumerate(cams):
        u, v, z = project(cam, X)
        seen[:, j] = (z > 0) & (u >= 0) & (u < w - 1) & (v >= 0) & (v < h - 1)
    keep = seen.sum(1) >= 2
    X, seen = X[keep], seen[keep]
    nf = len(X) // 100
    src = rng.choice(len(X), nf, replace=False)
    F = np.empty((nf, 3), np.float32); fv = np.empty(nf, np.int64)
    for q, k in enumerate(src):
        js = np.nonzero(seen[k])[0]
        j = js[rng.randint(len(js))]
        F[q] = cams[j]["C"] + rng.uniform(0.4, 0.85) * (X[k] - cams[j]["C"]); fv[q] = j
    xyz = np.concatenate([X, F])
    nv = np.concatenate([seen.sum(1), np.ones(nf, np.int64)]).astype(np.uint32)
    rows, cols = np.nonzero(seen)
    vi = np.concatenate([cols, fv]).astype(np.uint32)  # np.nonzero is row-major: the lists come out point by point, ids ascending
    return xyz, nv, vi, cams, np.arange(len(X), len(xyz))


def test_filter_at_scale(ctx):
    xyz, nv, vi, cams, floaters = ring_cloud(2_100_000)
    assert len(xyz) >= 2_000_000 and len(cams) == 32
    vis, kept = ctx.point_cloud_filter(xyz, nv, vi, cams, th_remove=-1)
    st = ctx.visibility_stats
    print("visibility at scale: %d points, %d pairs, %.1f candidates per pair, %d votes, %d exact-path pairs, %.1f ms, %.0f MiB" %
          (len(xyz), st["pairs"], st["candidates"] / st["pairs"], st["hits"], st["fallback_pairs"], st["ms_device"], st["device_bytes"] / 2 ** 20))
    rng = np.random.RandomState(3)
    sample = np.concatenate([rng.choice(floaters, 32, replace=False), rng.choice(len(xyz) - len(floaters), 32, replace=False)])
    ref = V.visibility(xyz, nv, vi, cams, targets=sample)
    assert np.array_equal(vis[sample], ref)
    assert np.array_equal(kept, V.removal_order(vis, -1))
    # every floater lies on the ray of a surface point seen by >= 2 views and goes -- unless the float32 cone test itself misses it: at
    # 1080p 1 - cos^2(half-angle) is 6 ulp of 1, and when |dir|^2 rounds low even a point on the axis tests t^2 == cosSq |E|^2 (not
    # VISIBLE).  Those few are checked against the brute force
    left = floaters[np.isin(floaters, kept)]
    assert len(left) <= len(floaters) // 1000
    assert (V.visibility(xyz, nv, vi, cams, targets=left) > -1).all() if len(left) else True


def write_dense(path, xyz, nv, vi, cams, rng, image_names=None):
    """a dense scene: one platform, one camera + pose per image (cameras carry their resolution, so no image is needed), vertices
    with views and weights, normals, colours"""
    platforms, images = [], []
    for i, c in enumerate(cams):
        platforms.append(dict(name="p%d" % i, cameras=[dict(name="c", width=c["width"], height=c["height"], K=c["K"], R=np.eye(3), C=np.zeros(3))],
                              poses=[dict(R=c["R"], C=c["C"])]))
        images.append(dict(name=(image_names or {}).get(i, "nowhere/img%03d.ppm" % i), platformID=i, cameraID=0, poseID=0, ID=i))
    wts = rng.uniform(0.1, 3.0, len(vi)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(nv, dtype=np.int64)])
    verts = [dict(X=xyz[k], views=[(int(vi[e]), float(wts[e])) for e in range(off[k], off[k + 1])]) for k in range(len(xyz))]
    normals = rng.normal(size=(len(xyz), 3)).astype(np.float32)
    colors = rng.randint(0, 256, (len(xyz), 3)).astype(np.uint8)
    mvsio.write_mvs(path, platforms, images, verts, colors, normals)
    return wts, normals, colors


def test_driver_filter_end_to_end(tmp_path):
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path)
    xyz, nv, vi, cams, _ = small_cloud(6, "plain", seed=4)
    rng = np.random.RandomState(0)
    src = os.path.join(tmp, "dense.mvs")
    wts, normals, colors = write_dense(src, xyz, nv, vi, cams, rng)
    out = os.path.join(tmp, "out.mvs")
    r = subprocess.run([EXE, "-i", src, "-o", out, "--filter-point-cloud", "-1", "-v", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Visibility lengths" in r.stdout and "Point-cloud filtered" in r.stdout
    vis, kept = V.filter_cloud(xyz, nv, vi, cams, -1)
    assert 0 < len(kept) < len(xyz)
    off = np.concatenate([[0], np.cumsum(nv, dtype=np.int64)])
    d = mvsio.read_mvs(os.path.join(tmp, "out_filtered.mvs"))
    assert len(d["vertices"]) == len(kept) and len(d["images"]) == len(cams)
    for q, k in enumerate(kept):
        v = d["vertices"][q]
        assert np.array_equal(v["X"], xyz[k])
        assert [a for a, _ in v["views"]] == vi[off[k]:off[k + 1]].tolist()
        assert np.array_equal(np.array([b for _, b in v["views"]], np.float32), wts[off[k]:off[k + 1]])
    assert np.array_equal(d["normals"], normals[kept]) and np.array_equal(d["colors"], colors[kept])
    ply = mvsio.read_ply(os.path.join(tmp, "out_filtered.ply"))
    assert len(ply) == len(kept)
    assert np.array_equal(np.stack([ply["x"], ply["y"], ply["z"]], -1), xyz[kept])
    assert np.array_equal(np.stack([ply["nx"], ply["ny"], ply["nz"]], -1), normals[kept])
    assert np.array_equal(np.stack([ply["blue"], ply["green"], ply["red"]], -1), colors[kept])
    # -v 3: the removed points, reverse index order, with their colours, in the working folder
    removed = np.nonzero(vis <= -1)[0][::-1]
    o = mvsio.read_ply(os.path.join(tmp, "scene_dense_outliers.ply"))
    assert np.array_equal(np.stack([o["x"], o["y"], o["z"]], -1), xyz[removed])
    assert np.array_equal(np.stack([o["blue"], o["green"], o["red"]], -1), colors[removed])
    # an empty cloud is an error
    empty = os.path.join(tmp, "empty.mvs")
    write_dense(empty, xyz[:0], nv[:0], vi[:0], cams, rng)
    r = subprocess.run([EXE, "-i", empty, "--filter-point-cloud", "-1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "empty initial point-cloud" in r.stderr


def test_driver_filter_after_densify(tmp_path):
    tmp = str(tmp_path)
    views = synth.make_views(192, 144, 220.0, 4, seed=4, baseline=(0.04, 0.09))
    verts = scene_files.sparse_vertices(views, 120)
    scene = scene_files.write_scene(tmp, views, verts)
    dense = os.path.join(tmp, "scene_dense.mvs")
    r = subprocess.run([EXE, "-i", scene, "-o", dense, "--resolution-level", "0", "--number-views", "4", "--n-EstimationIters", "2",
                        "--n-EstimationIters-external", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    n_in = len(mvsio.read_mvs(dense)["vertices"])
    assert n_in > 1000
    r = subprocess.run([EXE, "-i", dense, "--filter-point-cloud", "-1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = mvsio.read_mvs(os.path.join(tmp, "scene_dense_dense_filtered.mvs"))
    assert 0 < len(out["vertices"]) <= n_in
    assert len(mvsio.read_ply(os.path.join(tmp, "scene_dense_dense_filtered.ply"))) == len(out["vertices"])

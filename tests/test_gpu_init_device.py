"""The initial maps rasterised on the device (hcmvs_triangulate_init_device, hcmvs_splat_init_device; init_kernels.hip) against the host
forms (binding.triangulate_points, hcmvs_splat_points through Context.splat_init), which are the oracle: depth, normal, d_min and d_max
bit for bit.  The device buffers start out filled with a sentinel, so equality also shows that every pixel is written.  The host forms
get zero-filled normals (the device form defines the splat's normals as 0 everywhere)."""
import importlib

import numpy as np
import pytest
import torch

import init_plan_lib as IP

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")
D = importlib.import_module("hc-mvs_amd.distributed")

SENTINEL = 7.0
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def sentinel_maps(w, h):
    d = torch.full((h * w,), SENTINEL, dtype=torch.float32, device=DEV)
    n = torch.full((h * w * 3,), SENTINEL, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize(DEV)      # the context writes on a stream of its own
    return d, n


def untouched(d, n):
    return bool((d == SENTINEL).all()) and bool((n == SENTINEL).all())


def dev_tri(ctx, vid, w, h, pts, **kw):
    d, n = sentinel_maps(w, h)
    lo, hi = ctx.triangulate_init_device(vid, pts, d.data_ptr(), n.data_ptr(), **kw)
    ctx.synchronize()
    return d.cpu().numpy().reshape(h, w), n.cpu().numpy().reshape(h, w, 3), lo, hi


def dev_splat(ctx, vid, w, h, pts):
    d, n = sentinel_maps(w, h)
    lo, hi = ctx.splat_init_device(vid, pts, d.data_ptr(), n.data_ptr())
    ctx.synchronize()
    return d.cpu().numpy().reshape(h, w), n.cpu().numpy().reshape(h, w, 3), lo, hi


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3]


def scene(w, h, f, n, seed):
    views = synth.make_views(w, h, f, 1, seed=seed)
    return views[0], synth.sparse_points(views, n, seed=seed + 3)


def upload(ctx, vid, v):
    ctx.upload_view(vid, v["gray"], v["K"], v["R"], v["C"])


def plain_camera(w, h, f):
    """a camera at the origin looking down +z: world = camera space, so a pixel position survives the float32 round trip to within 2^-20"""
    return dict(gray=np.zeros((h, w), np.float32), K=np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float64), R=np.eye(3), C=np.zeros(3))


def backproject(v, xyz_pix):
    """(x, y, z) pixel position and depth -> world point, float32"""
    p = np.asarray(xyz_pix, np.float64).reshape(-1, 3)
    K = v["K"]
    Xc = np.stack([(p[:, 0] - K[0, 2]) * p[:, 2] / K[0, 0], (p[:, 1] - K[1, 2]) * p[:, 2] / K[1, 1], p[:, 2]], -1)
    return (Xc @ v["R"] + v["C"]).astype(np.float32)


def check_tri(ctx, v, w, h, pts, **kw):
    """device == host, and the counters against the shim's table; returns (host maps, stats)"""
    upload(ctx, 0, v)
    want = binding.triangulate_points(w, h, v["K"], v["R"], v["C"], pts, **kw)
    got = dev_tri(ctx, 0, w, h, pts, **kw)
    assert same(got, want)
    st = ctx.init_stats()
    tab = IP.tri_table(w, h, v["K"], v["R"], v["C"], pts, **kw)
    assert st["n_faces"] == len(tab["faces"]) and st["n_used"] == tab["n_used"]
    assert st["covered_pixels"] == int((want[0] > 0).sum())
    assert st["cover_hits"] == IP.raster_faces(tab, w, h)[2] >= st["covered_pixels"]
    assert st["n_tile_entries"] == len(IP.bin_tiles(w, h, IP.face_boxes(tab["faces"]))[3])
    assert st["ms_device"] > 0 and st["ms_host"] > 0 and st["device_bytes"] > 0
    return want, st


@pytest.mark.parametrize("w,h,f,n,seed", [(97, 131, 120.0, 25, 3), (160, 120, 150.0, 60, 1), (320, 200, 300.0, 400, 2), (640, 480, 500.0, 2000, 4)])
@pytest.mark.parametrize("add_corners", [True, False])
def test_triangulation_of_synth_scenes(ctx, w, h, f, n, seed, add_corners):
    tw, th = IP.tile_shape()
    assert 97 % tw and 131 % th        # the odd size is no multiple of the tile in either direction
    v, pts = scene(w, h, f, n, seed)
    want, st = check_tri(ctx, v, w, h, pts, add_corners=add_corners)
    if add_corners:
        assert (want[0] > 0).all()
    else:
        assert 0 < (want[0] > 0).mean() < 1


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("add_corners", [True, False])
def test_very_few_points(ctx, n, add_corners):
    """faces that span the whole image and many tiles; without corners one point leaves no face at all: a map of zeros"""
    w, h = 160, 120
    v, pts = scene(w, h, 150.0, n, seed=7)
    want, st = check_tri(ctx, v, w, h, pts, add_corners=add_corners)
    if add_corners:
        assert (want[0] > 0).all()
    if n == 1 and not add_corners:
        assert st["n_faces"] == 0 and not want[0].any()


def lattice_points(w, h):
    pix = []
    pix += [(x, 40.0, 0) for x in range(10, 150, 14)]                  # a row
    pix += [(80.0, y, 0) for y in range(8, 112, 13)]                   # a column
    pix += [(20.0 + 7 * k, 15.0 + 7 * k, 0) for k in range(12)]        # a diagonal
    pix += [(30.5 + 9 * k, 100.5 - 6 * k, 0) for k in range(10)]       # half-integer positions, an anti-diagonal run
    pix += [(12.5, 70.0, 0), (100.0, 20.5, 0), (140.5, 60.5, 0), (55.0, 90.0, 0), (56.0, 90.0, 0), (55.0, 91.0, 0), (120.0, 100.0, 0), (33.0, 57.5, 0)]
    pix += [(0.0, 30.0, 0), (0.0, 90.5, 0), (50.0, 0.0, 0), (110.5, 0.0, 0), (float(w), 45.0, 0), (float(w), 100.0, 0), (70.0, float(h), 0), (130.0, float(h), 0),
            (0.0, 0.0, 0), (float(w), float(h), 0)]                    # on the image's border lines
    return [(x, y, 8.0 + 0.01 * x + 0.02 * y) for (x, y, _) in pix]


@pytest.mark.parametrize("add_corners", [True, False])
def test_lattice_points_top_left_rule(ctx, add_corners):
    """edges pass exactly through pixel centres: the top-left bias of the edge constants decides, on both sides alike"""
    w, h = 160, 120
    v = plain_camera(w, h, 128.0)
    pix = lattice_points(w, h)
    assert len(pix) >= 55
    pts = backproject(v, pix)
    tab = IP.tri_table(w, h, v["K"], v["R"], v["C"], pts, add_corners=add_corners)
    assert (tab["faces"]["X"] % 8 == 0).mean() > 0.8     # the vertices sit on the half-pixel lattice of the 28.4 grid
    check_tri(ctx, v, w, h, pts, add_corners=add_corners)


@pytest.mark.parametrize("add_corners", [True, False])
def test_clusters_of_nearly_coincident_points(ctx, add_corners):
    """slivers below 1/16 pixel, faces that collapse or flip under the vertex rounding: whatever they cover, the order rule holds"""
    w, h = 160, 120
    v = plain_camera(w, h, 128.0)
    rng = np.random.RandomState(21)
    pix = []
    for _ in range(20):
        cx, cy = rng.uniform(10, w - 10), rng.uniform(10, h - 10)
        for _ in range(5):
            pix.append((cx + rng.uniform(-0.05, 0.05), cy + rng.uniform(-0.05, 0.05), 9.0 + rng.uniform(-0.5, 0.5)))
    want, st = check_tri(ctx, v, w, h, backproject(v, pix), add_corners=add_corners)
    print("clusters add_corners=%d: faces %d, cover_hits - covered_pixels = %d" % (add_corners, st["n_faces"], st["cover_hits"] - st["covered_pixels"]))


@pytest.mark.parametrize("add_corners", [True, False])
def test_points_outside_the_image_and_behind_the_camera(ctx, add_corners):
    w, h = 160, 120
    v, pts = scene(w, h, 150.0, 40, seed=12)
    outside = backproject(v, [(-30.0, 20.0, 9.0), (w + 50.0, 60.0, 10.0), (40.0, -20.0, 11.0), (90.0, h + 35.0, 9.5), (-200.0, -150.0, 12.0), (w + 3.0, h + 3.0, 8.0)])
    behind = backproject(v, [(50.0, 50.0, -4.0), (100.0, 30.0, -9.0)])
    mixed = np.vstack([pts[:20], outside[:3], behind, pts[20:], outside[3:]]).astype(np.float32)
    want, st = check_tri(ctx, v, w, h, mixed, add_corners=add_corners)
    if add_corners:
        assert st["n_used"] == 40           # the points outside are dropped
    else:
        assert st["n_used"] == 46           # faces cross the border and are clamped
    d, n = sentinel_maps(w, h)
    with pytest.raises(binding.HcmvsError, match="no sparse point in front of view 0"):
        ctx.triangulate_init_device(0, np.vstack([behind, behind]), d.data_ptr(), n.data_ptr(), add_corners=add_corners)
    ctx.synchronize()
    assert untouched(d, n)


def test_duplicates_and_explicit_avg_depth(ctx):
    w, h = 160, 120
    v, pts = scene(w, h, 150.0, 30, seed=15)
    dup = np.vstack([pts, pts[4:5], pts[17:18]]).astype(np.float32)
    want, st = check_tri(ctx, v, w, h, dup)
    assert st["n_used"] <= 30
    check_tri(ctx, v, w, h, pts, avg_depth=13.5)
    check_tri(ctx, v, w, h, pts, avg_depth=13.5, add_corners=False)
    # a corner with fewer than three faces to take its depth from keeps the average depth: with one point that is every corner
    a, _ = check_tri(ctx, v, w, h, pts[:1], avg_depth=13.5)
    c, _ = check_tri(ctx, v, w, h, pts[:1])
    assert not np.array_equal(a[0], c[0])


def splat_extras(v, w, h):
    return backproject(v, [(-1.0, 5.0, 9.0), (w + 0.4, h - 1.0, 11.0), (1.0, 1.0, 8.5), (w - 2.0, 0.0, 12.0)])


def check_splat(ctx, v, w, h, pts):
    upload(ctx, 0, v)
    want = ctx.splat_init(0, pts)            # hcmvs_splat_points with the view's camera, zero-filled normals
    got = dev_splat(ctx, 0, w, h, pts)
    assert same(got, want) and not got[1].any()
    st = ctx.init_stats()
    tab = IP.splat_table(w, h, v["K"], v["R"], v["C"], pts)
    box = tab["box"].astype(np.int64)
    hits = int(((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])).sum())
    assert st["n_used"] == len(pts) and st["n_faces"] == 0
    assert st["covered_pixels"] == int((want[0] > 0).sum()) and st["cover_hits"] == hits
    assert st["ms_device"] > 0
    return want, st


@pytest.mark.parametrize("w,h,f,n,seed", [(160, 120, 150.0, 300, 1), (97, 131, 120.0, 40, 2), (640, 480, 500.0, 2000, 3)])
def test_splat_matches_host(ctx, w, h, f, n, seed):
    views = synth.make_views(w, h, f, 1, seed=seed)
    v = views[0]
    pts = np.vstack([synth.sparse_points(views, n, seed=seed + 10), splat_extras(v, w, h)]).astype(np.float32)
    want, st = check_splat(ctx, v, w, h, pts)
    assert 0 < (want[0] > 0).mean() < 1
    if n == 300:
        assert st["cover_hits"] > int((want[0] > 0).sum())       # blocks overlap: the order rule decided pixels


def test_splat_fifty_points_on_one_pixel(ctx):
    w, h = 160, 120
    v = plain_camera(w, h, 128.0)
    rng = np.random.RandomState(5)
    pix = [(70.0 + rng.uniform(-0.3, 0.3), 50.0 + rng.uniform(-0.3, 0.3), 8.0 + 0.1 * k) for k in rng.permutation(50)]
    pts = backproject(v, pix + [(20.0, 20.0, 9.0)])
    tab = IP.splat_table(w, h, v["K"], v["R"], v["C"], pts)
    assert (tab["xy"][:50] == (70, 50)).all()
    want, st = check_splat(ctx, v, w, h, pts)
    assert want[0][50, 70] == tab["d"][49]       # the last of the fifty
    assert st["cover_hits"] == 51 * 25 and st["covered_pixels"] == 2 * 25


def test_determinism_and_buffer_reuse(ctx):
    big = scene(640, 480, 500.0, 2000, 4)
    small = scene(97, 131, 120.0, 25, 3)
    other = scene(160, 120, 150.0, 60, 1)
    upload(ctx, 0, big[0]); upload(ctx, 1, small[0]); upload(ctx, 2, other[0])
    want = {0: binding.triangulate_points(640, 480, big[0]["K"], big[0]["R"], big[0]["C"], big[1]),
            1: binding.triangulate_points(97, 131, small[0]["K"], small[0]["R"], small[0]["C"], small[1]),
            2: binding.triangulate_points(160, 120, other[0]["K"], other[0]["R"], other[0]["C"], other[1])}
    size = {0: (640, 480), 1: (97, 131), 2: (160, 120)}
    pts = {0: big[1], 1: small[1], 2: other[1]}
    # the same call twice; two images alternately; large, small, large again over the grow-only buffers
    for vid in (0, 0, 1, 2, 1, 2, 0, 1, 0):
        assert same(dev_tri(ctx, vid, *size[vid], pts[vid]), want[vid])
    # several calls enqueued back to back without a synchronise in between: the staging is reused only after its copy
    bufs = [(vid, sentinel_maps(*size[vid])) for vid in (0, 1, 2, 0)]
    for vid, (d, n) in bufs:
        ctx.triangulate_init_device(vid, pts[vid], d.data_ptr(), n.data_ptr())
    ctx.synchronize()
    for vid, (d, n) in bufs:
        w, h = size[vid]
        assert np.array_equal(d.cpu().numpy().reshape(h, w), want[vid][0]) and np.array_equal(n.cpu().numpy().reshape(h, w, 3), want[vid][1])


def test_bad_input_is_refused_and_nothing_is_written(ctx):
    w, h = 160, 120
    v, pts = scene(w, h, 150.0, 30, seed=9)
    upload(ctx, 0, v)
    d, n = sentinel_maps(w, h)
    bad = pts.copy(); bad[11, 1] = np.nan
    inf = pts.copy(); inf[3, 2] = np.inf
    for call in (ctx.triangulate_init_device, ctx.splat_init_device):
        with pytest.raises(binding.HcmvsError, match="coordinate 1 of point 11 is not finite"):
            call(0, bad, d.data_ptr(), n.data_ptr())
        with pytest.raises(binding.HcmvsError, match="coordinate 2 of point 3 is not finite"):
            call(0, inf, d.data_ptr(), n.data_ptr())
        with pytest.raises(binding.HcmvsError, match="n_points < 1"):
            call(0, np.zeros((0, 3), np.float32), d.data_ptr(), n.data_ptr())
        with pytest.raises(binding.HcmvsError, match="bad arguments"):
            call(0, pts, 0, n.data_ptr())
        with pytest.raises(binding.HcmvsError, match="unknown view 4242"):
            call(4242, pts, d.data_ptr(), n.data_ptr())
    ctx.synchronize()
    assert untouched(d, n)


def test_densify_scene_takes_points_instead_of_maps(ctx):
    """densify_scene with init entries as dicts (rasterised by the context into the slab) == with the host-made tuples: maps and clouds"""
    w, h = 96, 80
    base = synth.make_views(w, h, 90.0, 2, seed=3)
    n = len(base)
    views = {i: dict(gray=u["gray"], K=u["K"], R=u["R"], C=u["C"],
                     bgr=np.stack([np.clip(np.rint(u["gray"] * 255), 0, 255).astype(np.uint8)] * 3, -1).copy()) for i, u in enumerate(base)}
    srcs = {i: [j for j in range(n) if j != i] for i in range(n)}
    order = list(range(n))
    pts = {i: synth.sparse_points([base[i]], 60, seed=40 + i) for i in range(n)}
    p = binding.default_params(adapthalfwin=6, n_estimation_iters=2, seed=900)
    for i, u in views.items():
        ctx.upload_view(i, u["gray"], u["K"], u["R"], u["C"])

    def run(init):
        cloud = D.densify_scene(ctx, views, srcs, srcs, order, init, p, device=DEV)
        maps = {i: [m.cpu().numpy().copy() for m in cloud["maps"][i]] for i in order}
        return cloud["n_points"], np.array(cloud["xyz"]).copy(), np.array(cloud["n_views"]).copy(), maps

    def equal(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and all(
            np.array_equal(x, y) for i in order for x, y in zip(a[3][i], b[3][i]))

    tuples = {i: binding.triangulate_points(w, h, base[i]["K"], base[i]["R"], base[i]["C"], pts[i]) for i in order}
    dicts = {i: dict(points=pts[i]) for i in order}
    ref = run(tuples)
    assert ref[0] > 0 and (ref[3][0][0] > 0).mean() > 0.5
    assert equal(run(dicts), ref)
    assert equal(run({0: tuples[0], 1: dicts[1], 2: tuples[2]}), ref)
    # options travel with the dict
    opt = {i: binding.triangulate_points(w, h, base[i]["K"], base[i]["R"], base[i]["C"], pts[i], avg_depth=11.0, add_corners=False) for i in order}
    assert equal(run({i: dict(points=pts[i], avg_depth=11.0, add_corners=False) for i in order}), run(opt))
    # the splat
    stuples = {i: ctx.splat_init(i, pts[i]) for i in order}
    assert equal(run({i: dict(splat=pts[i]) for i in order}), run(stuples))

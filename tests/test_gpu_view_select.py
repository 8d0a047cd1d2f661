"""hcmvs_select_views (view_kernels.hip: one record per ordered pair of a vertex's views, a stable sort, one wave per pair, one wave per
image) against the numpy oracle (oracle/select_views.py) on the scenes of tests/view_select_scenes.py -- every image of every scene.

Exact: status, the points lists, neighbour ids and their order, points shared, covered area (= cells / 256), source ids, which sources
are resampled, nPoints, the number of candidates.  Floats, under the conditions tests/test_view_select_scenes.py asserts of the scenes
(viewing angles >= 2 degrees, <= 512 shared points per pair): the two sides differ by a few float32 ulp in the cosine, which acos turns
into <= 5e-7 / sin(2 deg) ~ 1.5e-5 rad; 512 sequential float32 additions add <= 512 * 2^-24 ~ 3e-5 relative.  Hence angle 1e-4 rad
absolute, scale and avgDepth 1e-4 relative, score 1e-3 relative (1.5 x the angle's relative error at 2 degrees, plus powf, plus the sum).
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import view_select_scenes as VS

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")

ANGLE_ABS, SCALE_REL, SCORE_REL = 1e-4, 1e-4, 1e-3


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def run(ctx, scene, csr=None, **kw):
    xyz, nv, ids = csr or scene.csr()
    return ctx.select_views_raw(scene.cams, scene.sizes, xyz, nv, ids, **kw)


def check_against_oracle(r, want, scene):
    for i, o in enumerate(want):
        tag = "%s image %d" % (scene.name, i)
        assert r["status"][i] == o["status"], tag
        assert r["n_seen"][i] == o["n_seen"] and r["n_candidates"][i] == len(o["candidates"]), tag
        assert list(r["point_ids"][int(r["points_first"][i]):int(r["points_first"][i + 1])]) == o["points"], tag
        assert r["avg_depth"][i] == pytest.approx(o["avg_depth"], rel=SCALE_REL), tag
        nb = o["neighbors"]
        assert r["n_neighbors"][i] == len(nb) and r["n_srcs"][i] == len(o["srcs"]), tag
        k = len(nb)
        assert list(r["nb_id"][i, :k]) == [n["id"] for n in nb], tag
        assert list(r["nb_points"][i, :k]) == [n["points"] for n in nb], tag
        assert list(r["nb_area"][i, :k]) == [n["area"] for n in nb], tag
        for j, n in enumerate(nb):
            print("%s nb %d: angle %+.2e rad, scale %+.2e rel, score %+.2e rel" % (
                tag, n["id"], r["nb_angle"][i, j] - n["angle"], r["nb_scale"][i, j] / n["scale"] - 1, r["nb_score"][i, j] / n["score"] - 1))
            assert abs(float(r["nb_angle"][i, j]) - n["angle"]) <= ANGLE_ABS, tag
            assert r["nb_scale"][i, j] == pytest.approx(n["scale"], rel=SCALE_REL), tag
            assert r["nb_score"][i, j] == pytest.approx(n["score"], rel=SCORE_REL), tag
        for j, (sid, sc) in enumerate(o["srcs"]):
            assert r["nb_id"][i, j] == sid and (r["src_scale"][i, j] != 1.0) == (sc != 1.0), tag
            assert r["src_scale"][i, j] == (1.0 if sc == 1.0 else r["nb_scale"][i, j]), tag
        assert not r["nb_id"][i, k:].any() and not r["nb_score"][i, k:].any() and not r["src_scale"][i, len(o["srcs"]):].any(), tag


def same_bits(a, b):
    keys = [k for k in a if k != "stats"]
    assert sorted(keys) == sorted(k for k in b if k != "stats")
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", sorted(VS.SCENES))
def test_every_image_matches_the_oracle(ctx, name):
    scene = VS.SCENES[name]()
    r = run(ctx, scene)
    check_against_oracle(r, VS.oracle_scene(name), scene)
    st = r["stats"]
    assert st["pairs"] == sum(len(v[1]) * (len(v[1]) - 1) for v in scene.verts) and st["skipped"] == 0 and st["chunks"] >= 1
    assert st["device_bytes"] > 0 and st["ms_device"] > 0


@pytest.mark.parametrize("name", sorted(VS.SCENES))
def test_python_shape_is_the_oracles(ctx, name):
    scene = VS.SCENES[name]()
    got = ctx.select_views(scene.cams, scene.sizes, *scene.csr())
    for g, o in zip(got, VS.oracle_scene(name)):
        assert (g is None) == (o["status"] != 0)
        if g is not None:
            assert g["points"] == o["points"] and [n["id"] for n in g["neighbors"]] == [n["id"] for n in o["neighbors"]] and g["status"] == 0
            assert [s[0] for s in g["srcs"]] == [s[0] for s in o["srcs"]]
            assert sorted(g["neighbors"][0]) == ["angle", "area", "id", "points", "scale", "score"]
            assert g["avg_depth"] == pytest.approx(o["avg_depth"], rel=SCALE_REL)
    assert list(ctx.view_select_stats["status"]) == [o["status"] for o in VS.oracle_scene(name)]


@pytest.mark.parametrize("name", sorted(VS.SCENES))
def test_skipped_view_entries(ctx, name):
    """view entries naming an uncalibrated image or an id >= n_images, on points that keep >= 2 valid views, change nothing"""
    scene = VS.SCENES[name]()
    n = len(scene.cams)
    extra = ([n - 1] if scene.cams[n - 1] is None else []) + [n, n + 24]
    rng = np.random.RandomState(5)
    verts, added = [], 0
    for X, views in scene.verts:
        add = [e for e in extra if rng.uniform() < 0.4] if len(views) >= 2 else []
        verts.append((X, views + add)); added += len(add)
    assert added > 50
    dirty = VS.Scene(scene.name, scene.cams, scene.sizes, verts)
    clean, r = run(ctx, scene), run(ctx, dirty)
    same_bits(clean, r)
    assert r["stats"]["skipped"] == added and r["stats"]["pairs"] == clean["stats"]["pairs"]


def test_determinism_and_chunking(ctx):
    scene = VS.ring()
    a, b = run(ctx, scene), run(ctx, scene)
    same_bits(a, b)
    assert "HCMVS_SELECT_CHUNK" not in os.environ
    try:
        for size, chunks in (("1", 16), ("3", 6)):
            os.environ["HCMVS_SELECT_CHUNK"] = size
            c = run(ctx, scene)
            same_bits(a, c)
            assert c["stats"]["chunks"] == chunks > 1
    finally:
        os.environ.pop("HCMVS_SELECT_CHUNK", None)
    assert run(ctx, scene)["stats"]["chunks"] == a["stats"]["chunks"] == 1


@pytest.mark.parametrize("kw", [dict(number_views=0), dict(n_max_views=1), dict(n_max_views=64), dict(number_views=2, n_max_views=7)],
                         ids=["all_views", "max1", "max64", "views2_max7"])
def test_other_parameters(ctx, kw):
    scene = VS.ring()
    okw = dict(number_views=kw.get("number_views", 5), n_max_views=kw.get("n_max_views", 12))
    r = run(ctx, scene, **kw)
    assert r["nb_id"].shape == (16, okw["n_max_views"])
    check_against_oracle(r, VS.oracle_scene("ring", **okw), scene)


def test_no_points(ctx):
    scene = VS.ring()
    r = run(ctx, scene, csr=(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
    assert list(r["status"]) == [1] * 15 + [3]
    assert not r["n_seen"].any() and not r["n_neighbors"].any() and not r["n_srcs"].any() and not r["avg_depth"].any()
    assert len(r["point_ids"]) == 0 and not r["points_first"].any() and r["stats"]["pairs"] == 0


def test_refusals(ctx):
    scene = VS.small()
    xyz, nv, ids = scene.csr()

    def refused(match, cams=scene.cams, sizes=scene.sizes, xyz=xyz, nv=nv, ids=ids, **kw):
        with pytest.raises(binding.HcmvsError, match=match) as e:
            ctx.select_views_raw(cams, sizes, xyz, nv, ids, **kw)
        assert e.value.code == binding.ERR_INVALID

    bad = xyz.copy(); bad[7, 1] = np.nan
    refused("point 7 ", xyz=bad)
    bad = xyz.copy(); bad[3, 0] = np.inf; bad[9, 2] = np.nan
    refused("point 3 ", xyz=bad)                                            # the first offender
    cams = [dict(c) for c in scene.cams]; cams[2] = dict(cams[2], R=cams[2]["R"].copy()); cams[2]["R"][1, 1] = np.inf
    refused("image 2 ", cams=cams)
    first = np.concatenate([[0], np.cumsum(nv, dtype=np.int64)])
    p = int(np.nonzero(nv >= 2)[0][4])
    swapped = ids.copy(); swapped[first[p]], swapped[first[p] + 1] = ids[first[p] + 1], ids[first[p]]
    refused("point %d " % p, ids=swapped)
    equal = ids.copy(); equal[first[p] + 1] = ids[first[p]]
    refused("point %d " % p, ids=equal)
    refused("n_max_views", n_max_views=0)
    refused("n_max_views", n_max_views=65)
    refused("images", cams=[], sizes=[])
    refused("images", cams=[None] * 65536, sizes=[None] * 65536)
    # 2^32 view entries: refused on the counts alone, before any id is read
    many = np.full(2, 1 << 31, np.uint32)
    par = binding.default_view_select_params()
    r = run(ctx, scene)
    arrays = {k: r[k] for k, _ in binding.ViewSelection._fields_}
    sel = binding.ViewSelection()
    for k, a in arrays.items():
        setattr(sel, k, a.ctypes.data_as(dict(binding.ViewSelection._fields_)[k]))
    m = len(scene.cams)
    wh = np.array(scene.sizes, np.int32); K = np.stack([c["K"].ravel() for c in scene.cams]); R = np.stack([c["R"].ravel() for c in scene.cams])
    Cc = np.stack([c["C"] for c in scene.cams])
    dp, u32 = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    rc = binding.lib().hcmvs_select_views(ctx._h, m, wh.ctypes.data_as(C.POINTER(C.c_int32)), K.ctypes.data_as(dp), R.ctypes.data_as(dp), Cc.ctypes.data_as(dp), 2,
                                          xyz[:2].ctypes.data_as(C.POINTER(C.c_float)), many.ctypes.data_as(u32), ids.ctypes.data_as(u32), C.byref(par), C.byref(sel),
                                          None)
    assert rc == binding.ERR_INVALID and b"2^32" in binding.lib().hcmvs_last_error(ctx._h)
    # the context is as good as before
    same_bits(run(ctx, scene), r)


def test_plan_scene_end_to_end():
    """4 images of 160 x 128, one outer iteration, 2 sweeps: plan_scene -> triangulate_init on the returned points -> densify_scene gives,
    bit for bit, the cloud of the same run planned with the oracle's select()"""
    import torch
    import scene_files as SF
    synth = importlib.import_module("hc-mvs_amd.synth")
    D = importlib.import_module("hc-mvs_amd.distributed")
    base = synth.make_views(160, 128, 150.0, 3, seed=31, baseline=(0.07, 0.10))
    verts = SF.sparse_vertices(base, 150, seed=3)
    views = {i: dict(gray=v["gray"], K=v["K"], R=v["R"], C=v["C"],
                     bgr=np.stack([np.clip(np.rint(v["gray"] * 255), 0, 255).astype(np.uint8)] * 3, -1).copy()) for i, v in enumerate(base)}
    cams = [dict(K=v["K"], R=v["R"], C=v["C"]) for v in base]
    sizes = [(160, 128)] * 4
    vlist = [(x["X"], [j for j, _ in x["views"]]) for x in verts]
    xyz, nv, ids = VS.Scene("e2e", cams, sizes, vlist).csr()
    sel = [VS.SV.select(cams, sizes, vlist, i, number_views=3) for i in range(4)]
    assert all(s is not None for s in sel)
    want_plan = ({i: [s[0] for s in sel[i]["srcs"]] for i in range(4)}, {i: [n["id"] for n in sel[i]["neighbors"]] for i in range(4)},
                 sorted(range(4), key=lambda i: -len(sel[i]["neighbors"])), {i: sel[i]["points"] for i in range(4)})
    clouds = []
    for planned_by in ("device", "oracle"):
        ctx = binding.Context(0)
        try:
            if planned_by == "device":
                srcs, neighbors, order, points = D.plan_scene(ctx, cams, sizes, xyz, nv, ids, number_views=3)
                assert (srcs, neighbors, order) == want_plan[:3] and {i: list(p) for i, p in points.items()} == want_plan[3]
                assert all(s == 1.0 for g in ctx.select_views(cams, sizes, xyz, nv, ids, number_views=3) for _, s in g["srcs"])
            else:
                srcs, neighbors, order, points = want_plan
            for i, v in views.items():
                ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"])
            init = {i: ctx.triangulate_init(i, xyz[np.asarray(points[i], np.int64)]) for i in order}
            p = binding.default_params(adapthalfwin=6, n_estimation_iters=2, seed=77)
            clouds.append(D.densify_scene(ctx, views, srcs, neighbors, order, init, p, device=torch.device("cuda", 0), n_external_iters=1))
        finally:
            ctx.close()
    a, b = clouds
    assert a["n_points"] == b["n_points"] > 1000
    for k in ("xyz", "normal", "bgr", "n_views"):
        assert np.array_equal(a[k], b[k]), k

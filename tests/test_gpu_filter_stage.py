"""hcmvs_filter_sequence / Context.filter_sequence on the GPU against the scene-level oracle (tests/filter_stage.py: the snapshot loop over the
CPU oracle), bit for bit: adjust and strict, the neighbour cap and its order, a neighbour without maps, an image with too few neighbours,
a view of another size, forced batch sizes; the fusion that follows; one full-size run (64 x 1080p, 8 neighbours) on device maps."""
import importlib
import os

import numpy as np
import pytest

import filter_stage as FS
import oracle_lib as O

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")

_cache = {}


def _special():
    if "scene" not in _cache:
        _cache["scene"] = FS.special_scene()
    return _cache["scene"]


def _want(adjust, max_neighbors):
    key = (adjust, max_neighbors)
    if key not in _cache:
        maps, ids = _special()
        _cache[key] = FS.stage(maps, ids + [9], max_neighbors=max_neighbors, adjust=adjust)   # (9: an id nobody registered)
    return _cache[key]


def _run(adjust, max_neighbors, batch):
    """a fresh context, the stage with HCMVS_FILTER_BATCH = batch (None: automatic); returns (maps read back, stats)"""
    maps, ids = _special()
    old = os.environ.pop("HCMVS_FILTER_BATCH", None)
    if batch is not None:
        os.environ["HCMVS_FILTER_BATCH"] = batch
    ctx = binding.Context(0)
    try:
        FS.upload(ctx, maps)
        st = ctx.filter_sequence(ids + [9], max_neighbors=max_neighbors, adjust=adjust)
        got = [ctx.get_depthmap(i, with_normal=True) if m.get("depth") is not None else None for i, m in enumerate(maps)]
    finally:
        ctx.close()
        os.environ.pop("HCMVS_FILTER_BATCH", None)
        if old is not None:
            os.environ["HCMVS_FILTER_BATCH"] = old
    return got, st


@pytest.mark.parametrize("max_neighbors", [8, 3], ids=["all-neighbours", "cap-3"])
@pytest.mark.parametrize("adjust", [True, False], ids=["adjust", "strict"])
def test_filter_sequence_matches_the_snapshot_oracle(adjust, max_neighbors):
    maps, ids = _special()
    want, counts, skipped = _want(adjust, max_neighbors)
    assert skipped == [5, 6, 9] and len(counts) == 5
    runs = {b: _run(adjust, max_neighbors, b) for b in (None, "1", "all")}
    for b, (got, st) in runs.items():
        print("batch %s: %d filtered, %d skipped, %d/%d discarded, batches of %d, %.3f ms" % (b, st["n_filtered"], st["n_skipped"], st["n_discarded"],
                                                                                             st["n_processed"], st["batch"], st["ms_device"]))
        assert st["n_filtered"] == 5 and st["n_skipped"] == 3 and st["batch"] == (1 if b == "1" else 5)
        assert st["image_processed"] == [counts.get(i, (0, 0))[0] for i in ids + [9]]
        assert st["image_discarded"] == [counts.get(i, (0, 0))[1] for i in ids + [9]]
        assert st["n_processed"] == sum(v[0] for v in counts.values()) and st["n_discarded"] == sum(v[1] for v in counts.values())
        for i, m in enumerate(maps):
            if m.get("depth") is None:
                continue
            d, n, c = got[i]
            assert d.shape == want[i]["depth"].shape
            assert np.array_equal(d, want[i]["depth"]), "depth of image %d differs from the oracle (batch %s)" % (i, b)
            assert np.array_equal(c, want[i]["conf"]), "confidence of image %d differs from the oracle (batch %s)" % (i, b)
            assert np.array_equal(n, m["normal"])                              # untouched
        # too few usable neighbours: the maps come back as they went in
        assert np.array_equal(got[5][0], maps[5]["depth"]) and np.array_equal(got[5][2], maps[5]["conf"])
    for b in ("1", "all"):                                                        # the result does not depend on the batch
        for i, g in enumerate(runs[None][0]):
            if g is not None:
                assert np.array_equal(g[0], runs[b][0][i][0]) and np.array_equal(g[2], runs[b][0][i][2])
    # the stage is not the in-place loop: the oracle of THAT differs from what the device computed
    seq, _, _ = FS.stage(maps, ids, max_neighbors=max_neighbors, adjust=adjust, in_place=True)
    assert any(not np.array_equal(seq[i]["depth"], runs[None][0][i][0]) for i in range(5))


def test_bad_arguments_are_refused():
    maps, ids = _special()
    ctx = binding.Context(0)
    try:
        FS.upload(ctx, maps[:2])
        for kw in (dict(max_neighbors=0), dict(max_neighbors=65)):
            with pytest.raises(binding.HcmvsError) as e:
                ctx.filter_sequence([0, 1], **kw)
            assert e.value.code == binding.ERR_INVALID
        st = ctx.filter_sequence([])
        assert st["n_filtered"] == 0 and st["n_skipped"] == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("adjust", [True, False], ids=["adjust", "strict"])
def test_fuse_after_filter_sequence_equals_the_oracle(adjust):
    """filter_sequence, then fuse == the oracle's fusion of the oracle-filtered maps, point for point"""
    maps, order = FS.issue_scene()
    ids = list(range(len(maps)))
    want, counts, skipped = FS.stage(maps, ids, adjust=adjust)
    assert not skipped
    ref = O.fuse_depthmaps(want, order, 200000)
    ctx = binding.Context(0)
    try:
        FS.upload(ctx, maps)
        st = ctx.filter_sequence(ids, adjust=adjust)
        assert st["n_skipped"] == 0 and st["image_discarded"] == [counts[i][1] for i in ids]
        cloud = ctx.fuse(order, 200000)
    finally:
        ctx.close()
    assert cloud["n_points"] == ref["n_points"] > 5000 and cloud["n_depths"] == ref["n_depths"]
    assert np.array_equal(cloud["xyz"], ref["xyz"]) and np.array_equal(cloud["n_views"], ref["n_views"])
    assert np.array_equal(cloud["bgr"], ref["bgr"])


def test_full_size_64x1080p_on_device_maps():
    """64 images of 1920x1080 with 8 neighbours each, maps in caller-owned device memory: every image filtered; the images checked agree
    bit for bit with the per-image hcmvs_filter on the maps as they were (the snapshot), the normals are untouched, the batch does not matter"""
    import torch
    dev = torch.device("cuda", 0)
    n, w, h = 64, 1920, 1080
    cams, depth, normal, conf, rng, nbrs = FS.device_ring(n, w, h, 8, dev)
    gray = torch.zeros(h, w, dtype=torch.float32, device=dev)
    d0, c0, n0 = depth.clone(), conf.clone(), normal.clone()
    torch.cuda.synchronize()
    os.environ.pop("HCMVS_FILTER_BATCH", None)
    ctx = binding.Context(0)
    try:
        FS.register_device_ring(ctx, cams, depth, normal, conf, rng, nbrs, gray)
        probes = {i: ctx.filter(i, nbrs[i], adjust=True) for i in (0, 37)}
        st = ctx.filter_sequence(range(n), adjust=True)
        print("64 x 1080p, 8 neighbours, adjust: %.2f ms on the device, batches of %d, %.2f GiB, %d/%d discarded" %
              (st["ms_device"], st["batch"], st["device_bytes"] / 2 ** 30, st["n_discarded"], st["n_processed"]))
        assert st["n_filtered"] == n and st["n_skipped"] == 0
        assert all(0 < st["image_discarded"][i] < st["image_processed"][i] for i in range(n))
        assert st["image_processed"] == [int(x) for x in (d0 > 0).sum((1, 2)).tolist()]
        for i, (pd, pc, npr, nd) in probes.items():
            assert (npr, nd) == (st["image_processed"][i], st["image_discarded"][i])
            assert np.array_equal(depth[i].cpu().numpy(), pd) and np.array_equal(conf[i].cpu().numpy(), pc)
        assert torch.equal(normal, n0)
        first = depth.clone(), conf.clone()
        depth.copy_(d0); conf.copy_(c0)
        torch.cuda.synchronize()
        os.environ["HCMVS_FILTER_BATCH"] = "7"                                   # batches of 7 and a last one of 1
        st7 = ctx.filter_sequence(range(n), adjust=True)
        assert st7["batch"] == 7 and st7["image_discarded"] == st["image_discarded"]
        assert torch.equal(depth, first[0]) and torch.equal(conf, first[1])
    finally:
        os.environ.pop("HCMVS_FILTER_BATCH", None)
        ctx.close()

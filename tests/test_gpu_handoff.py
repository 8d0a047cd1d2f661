"""The hand-off between two pyramid levels on the device (hcmvs_handoff_maps_device; handoff_kernels.hip) against the host form
(binding.handoff_maps, pinned on the CPU by test_handoff_host.py): depth, normal, d_min, d_max, status and counters bit for bit (a NaN
equal to any NaN).  The destination buffers start out filled with a sentinel, so equality also shows that every pixel is written.  Then
the callers: densify_scene's `previous` init entries, its hints and densify_pyramid, each against the same chain composed by hand through
host copies and the host form."""
import copy
import importlib

import numpy as np
import pytest
import torch

import handoff_ref as R

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")
D = importlib.import_module("hc-mvs_amd.distributed")

F = np.float32
SENTINEL = 7.0
DEV = torch.device("cuda", 0)
HINT_RANGES = {"mixed": (2.0, 7.0), "clean": (0.5, 20.0), "nan_last": (2.0, 7.0), "empty": (3.0, 4.0)}
COUNTERS = ("n_valid", "n_clamped", "n_rescaled")


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def dev_handoff(ctx, mode, jobs):
    """jobs: dicts as binding.handoff_maps takes them.  The maps are read back right after the call: it has synchronised"""
    keep, items = [], []
    for m in jobs:
        sd = torch.from_numpy(np.ascontiguousarray(m["depth"], F)).to(DEV); sn = torch.from_numpy(np.ascontiguousarray(m["normal"], F)).to(DEV)
        dw, dh = m["dst_w"], m["dst_h"]
        dd = torch.full((dh * dw,), SENTINEL, dtype=torch.float32, device=DEV); dn = torch.full((dh * dw * 3,), SENTINEL, dtype=torch.float32, device=DEV)
        keep.append((sd, sn, dd, dn))
        items.append(dict(src_depth=sd.data_ptr(), src_normal=sn.data_ptr(), src_w=sd.shape[1], src_h=sd.shape[0], dst_depth=dd.data_ptr(),
                          dst_normal=dn.data_ptr(), dst_w=dw, dst_h=dh, d_min=m.get("d_min", 0.0), d_max=m.get("d_max", 0.0)))
    torch.cuda.synchronize(DEV)      # the context works on a stream of its own
    res = ctx.handoff_maps_device(items, mode)
    for r, m, (_, _, dd, dn) in zip(res, jobs, keep):
        r["depth"] = dd.cpu().numpy().reshape(m["dst_h"], m["dst_w"]); r["normal"] = dn.cpu().numpy().reshape(m["dst_h"], m["dst_w"], 3)
    return res


def same(got, want):
    return (R.same_bits(got["depth"], want["depth"]) and R.same_bits(got["normal"], want["normal"]) and got["status"] == want["status"] and
            R.same_bits(F(got["d_min"]), F(want["d_min"])) and R.same_bits(F(got["d_max"]), F(want["d_max"])) and all(got[k] == want[k] for k in COUNTERS))


def job(mode, src, dst, content, seed=0):
    d, n = R.make_maps(*src, content, seed=seed, hint=mode == "hint")
    lo, hi = HINT_RANGES[content] if mode == "hint" else (-5.0, -6.0)
    return dict(depth=d, normal=n, dst_w=dst[0], dst_h=dst[1], d_min=lo, d_max=hi)


CASES = [("init", s, d) for s, d in R.INIT_SHAPES] + [("hint", s, d) for s, d in R.HINT_SHAPES]


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("mode,src,dst", CASES)
def test_device_equals_host(ctx, mode, src, dst, content):
    m = job(mode, src, dst, content)
    want = binding.handoff_maps([m], mode)[0]
    got = dev_handoff(ctx, mode, [m])[0]
    assert same(got, want)
    # the counters of the call against the numpy statement's counts
    ref = R.handoff(mode, m["depth"], m["normal"], m["dst_w"], m["dst_h"], m["d_min"], m["d_max"])
    st = ctx.handoff_stats()
    assert st["n_pixels"] == dst[0] * dst[1] and st["n_items"] == 1 and st["ms_device"] > 0
    assert all(st[k] == ref[k] for k in COUNTERS) and st["n_empty"] == ref["status"] == want["status"]
    if mode == "init" and want["status"] == binding.HANDOFF_EMPTY:
        assert (got["d_min"], got["d_max"]) == (-5.0, -6.0) and not got["depth"].any()      # untouched; the maps are written all the same


def test_the_special_pixels_reach_the_device_form(ctx):
    """what the cases above rest on, asserted on their input: an undershoot that is clamped, a NaN that replaces hi in the middle of the map"""
    m = job("init", (37, 29), (74, 58), "mixed")
    ref = R.handoff_init(m["depth"], m["normal"], 74, 58)
    assert ref["n_negative"] >= 1 and np.isnan(ref["raw"]).any()
    got = dev_handoff(ctx, "init", [m])[0]
    assert got["n_clamped"] == ref["n_clamped"] >= ref["n_negative"] and (got["depth"] >= 0).all()
    m = dict(job("hint", (37, 29), (74, 58), "mixed"), d_min=2.0, d_max=50.0)
    ref = R.handoff_hint(m["depth"], m["normal"], 74, 58, 2.0, 50.0)
    raw = ref["raw"].reshape(-1)
    last = np.flatnonzero(np.isnan(raw))[-1]
    assert ref["n_negative"] >= 1 and 0 < last < len(raw) - 1 and ref["d_max"] == raw[last + 1:].max() < 50.0
    got = dev_handoff(ctx, "hint", [m])[0]
    assert R.same_bits(F(got["d_max"]), F(ref["d_max"])) and got["d_min"] == 0.0
    # no NaN: the range taken in survives when it is the wider one, and is widened when it is not
    m = job("hint", (37, 29), (61, 47), "clean")
    for lo, hi in ((0.5, 20.0), (3.0, 4.0), (-2.0, 1.0)):
        mm = dict(m, d_min=lo, d_max=hi)
        assert same(dev_handoff(ctx, "hint", [mm])[0], binding.handoff_maps([mm], "hint")[0])


@pytest.mark.parametrize("mode", ["init", "hint"])
def test_a_batch_of_five_mixed_sizes_equals_the_single_calls(ctx, mode):
    shapes = (R.INIT_SHAPES if mode == "init" else R.HINT_SHAPES)[:5]
    # (the fifth source is 1 x 1: a NaN there would leave init mode a second empty item)
    jobs = [job(mode, s, d, c, seed=7) for (s, d), c in zip(shapes, ["mixed", "clean", "empty", "mixed", "nan_last" if mode == "hint" else "clean"])]
    batch = dev_handoff(ctx, mode, jobs)
    st = ctx.handoff_stats()
    singles = [dev_handoff(ctx, mode, [m])[0] for m in jobs]
    hosts = binding.handoff_maps(jobs, mode)
    assert all(same(b, s) and same(b, h) for b, s, h in zip(batch, singles, hosts))
    assert st["n_items"] == 5 and st["n_pixels"] == sum(m["dst_w"] * m["dst_h"] for m in jobs)
    assert all(st[k] == sum(b[k] for b in batch) for k in COUNTERS)
    if mode == "init":
        assert [b["status"] for b in batch] == [0, 0, 1, 0, 0] and st["n_empty"] == 1     # the empty item fails neither the call nor the others


def test_refusals_leave_the_context_usable(ctx):
    cases, keep = R.refusals()
    for name, items, mode, n in cases:
        if items is None or n is not None:
            continue
        with pytest.raises(binding.HcmvsError) as e:     # refused before anything reaches the device: these addresses are never read
            ctx.handoff_maps_device(items, mode)
        assert e.value.code == binding.ERR_INVALID and "handoff_maps_device" in str(e.value), name
    with pytest.raises(binding.HcmvsError) as e:
        ctx.handoff_maps_device([], "init")
    assert e.value.code == binding.ERR_INVALID
    m = job("init", (37, 29), (61, 47), "mixed")
    assert same(dev_handoff(ctx, "init", [m])[0], binding.handoff_maps([m], "init")[0])


# ---- the callers ----------------------------------------------------------------------------------------------------------------------

FINE, COARSE = (144, 112, 135.0), (72, 56, 67.5)


def level(size, n_src=2):
    """the same scene and cameras at one level's size; the texture is band-limited to the coarse level's pixel"""
    w, h, f = size
    px = 10.0 / COARSE[2]
    scene = synth.Scene(3, min_wavelength=3.5 * px, max_wavelength=150 * px)
    base = synth.make_views(w, h, f, n_src, seed=3, scene=scene)
    views = {i: dict(gray=u["gray"], K=u["K"], R=u["R"], C=u["C"],
                     bgr=np.stack([np.clip(np.rint(u["gray"] * 255), 0, 255).astype(np.uint8)] * 3, -1).copy()) for i, u in enumerate(base)}
    return base, views


@pytest.fixture(scope="module")
def S():
    fine, fviews = level(FINE)
    coarse, cviews = level(COARSE)
    n = len(fine)
    srcs = {i: [j for j in range(n) if j != i] for i in range(n)}
    pts = {i: synth.sparse_points([fine[i]], 60, seed=40 + i) for i in range(n)}
    prev = {}       # maps of the coarse level: its ground truth with an empty border, as an estimate leaves it
    for i, u in enumerate(coarse):
        d = u["depth"].copy(); d[:4] = 0; d[-4:] = 0; d[:, :4] = 0; d[:, -4:] = 0
        prev[i] = (d, (u["normal"] * F(0.8)).astype(F))
    return dict(fine=fine, fviews=fviews, coarse=coarse, cviews=cviews, srcs=srcs, order=list(range(n)), pts=pts, prev=prev,
                p=binding.default_params(adapthalfwin=5, n_estimation_iters=2, seed=900))


def host_maps(cloud, order):
    return {i: [m.cpu().numpy().copy() for m in cloud["maps"][i]] for i in order}


def cloud_of(cloud, order):
    return cloud["n_points"], np.array(cloud["xyz"]).copy(), np.array(cloud["n_views"]).copy(), host_maps(cloud, order)


def equal_maps(a, b, order):
    return all(R.same_bits(x, y) for i in order for x, y in zip(a[i], b[i]))


def equal_clouds(a, b, order):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and equal_maps(a[3], b[3], order)


def test_densify_scene_starts_from_previous_maps(ctx, S):
    w, h, _ = FINE
    order = S["order"]
    made = {i: binding.handoff_maps([dict(depth=S["prev"][i][0], normal=S["prev"][i][1], dst_w=w, dst_h=h)], "init")[0] for i in order}
    tuples = {i: (r["depth"], r["normal"], r["d_min"], r["d_max"]) for i, r in made.items()}
    ref = cloud_of(D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], order, tuples, S["p"], device=DEV), order)
    assert ref[0] > 0 and (ref[3][0][0] > 0).mean() > 0.5
    prev = {0: dict(previous=S["prev"][0]),                                                   # numpy arrays
            1: dict(previous=tuple(torch.from_numpy(m).to(DEV) for m in S["prev"][1])),     # device tensors
            2: dict(previous=S["prev"][2])}
    assert equal_clouds(cloud_of(D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], order, prev, S["p"], device=DEV), order), ref, order)
    assert equal_clouds(cloud_of(D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], order, {0: prev[0], 1: tuples[1], 2: prev[2]}, S["p"], device=DEV), order), ref, order)
    # fuse=False: no cloud, and the maps as the estimate left them (a fusion takes the depths it merges out of them)
    res = D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], order, prev, S["p"], device=DEV, fuse=False)
    unfused = host_maps(D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], order, tuples, S["p"], device=DEV, fuse=False), order)
    assert "xyz" not in res and equal_maps(host_maps(res, order), unfused, order) and not equal_maps(unfused, ref[3], order)
    assert all(res["ranges"][i] == (tuples[i][2], tuples[i][3]) for i in order)
    empty = dict(prev)
    empty[1] = dict(previous=(np.zeros_like(S["prev"][1][0]), S["prev"][1][1]))
    with pytest.raises(ValueError, match="image 1 holds no valid depth"):
        D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], order, empty, S["p"], device=DEV)


def estimate_with_host_hint(ctx, S, img, init, prev_maps, p):
    """one direct estimate_batch_device of image img at the fine level: the hint made by the host form and uploaded here, the range
    widened by it.  Returns (depth, normal, conf) host arrays"""
    w, h, _ = FINE
    d0, n0, lo, hi = init
    hint = binding.handoff_maps([dict(depth=prev_maps[0], normal=prev_maps[1], dst_w=w, dst_h=h, d_min=lo, d_max=hi)], "hint")[0]
    t = [torch.from_numpy(np.ascontiguousarray(a, F)).to(DEV) for a in (d0, n0, np.zeros((h, w), F), hint["depth"], hint["normal"])]
    torch.cuda.synchronize(DEV)
    ctx.estimate_batch_device([dict(ref_id=img, src_ids=list(S["srcs"][img]), d_min=hint["d_min"], d_max=hint["d_max"], d_depth=t[0].data_ptr(),
                                    d_normal=t[1].data_ptr(), d_conf=t[2].data_ptr(), seed_offset=img, d_hint_depth=t[3].data_ptr(),
                                    d_hint_normal=t[4].data_ptr())], p)
    ctx.synchronize()
    return [x.cpu().numpy().copy() for x in t[:3]], hint


def test_densify_scene_takes_hints(ctx, S):
    w, h, _ = FINE
    u = S["fine"][0]
    init = {0: binding.triangulate_points(w, h, u["K"], u["R"], u["C"], S["pts"][0])}
    got = D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], [0], init, S["p"], device=DEV, hints={0: S["prev"][0]}, fuse=False)
    gmaps = host_maps(got, [0])[0]
    p = copy.copy(S["p"]); p.it_external = 0; p.n_external_iters = 1
    want, hint = estimate_with_host_hint(ctx, S, 0, init[0], S["prev"][0], p)      # the views are registered: densify_scene uploaded them
    assert all(R.same_bits(a, b) for a, b in zip(gmaps, want))
    assert got["ranges"][0] == (hint["d_min"], hint["d_max"]) and hint["d_min"] == 0.0       # widened: the coarse map's border is empty
    plain = host_maps(D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], [0], init, S["p"], device=DEV, fuse=False), [0])[0]
    assert not R.same_bits(plain[0], gmaps[0])       # the hint was offered and taken somewhere


def near_truth(depth, truth):
    return float((np.abs(depth - truth) < 0.01 * truth).mean())


def test_densify_pyramid_equals_the_stages_composed_by_hand(ctx, S):
    w, h, _ = FINE
    order, p = S["order"], S["p"]
    init = {i: dict(points=S["pts"][i]) for i in order}
    stages = [dict(views=S["cviews"], params=p, mode="triangulate"), dict(views=S["fviews"], params=p, mode="restore"),
              dict(views=S["fviews"], params=p, mode="handoff")]
    got = cloud_of(D.densify_pyramid(ctx, stages, S["srcs"], S["srcs"], order, init, device=DEV), order)
    # by hand: stage 0 ...
    a = host_maps(D.densify_scene(ctx, S["cviews"], S["srcs"], S["srcs"], order, init, p, device=DEV, fuse=False), order)
    # ... `restore` at the fine level: the triangulation, the host-made hint, one direct estimate per image ...
    for i, u in S["fviews"].items():
        ctx.upload_view(i, u["gray"], u["K"], u["R"], u["C"], bgr=u["bgr"])
    p1 = copy.copy(p); p1.it_external = 0; p1.n_external_iters = 1
    b = {}
    for i in order:
        u = S["fine"][i]
        tri = binding.triangulate_points(w, h, u["K"], u["R"], u["C"], S["pts"][i])
        b[i], _ = estimate_with_host_hint(ctx, S, i, tri, a[i][:2], p1)
    # ... and the hand-off at equal size through the host form
    made = {i: binding.handoff_maps([dict(depth=b[i][0], normal=b[i][1], dst_w=w, dst_h=h)], "init")[0] for i in order}
    tuples = {i: (r["depth"], r["normal"], r["d_min"], r["d_max"]) for i, r in made.items()}
    want = cloud_of(D.densify_scene(ctx, S["fviews"], S["srcs"], S["srcs"], order, tuples, p, device=DEV), order)
    assert want[0] > 0 and equal_clouds(got, want, order)
    # a property of the result, no tuned bar: three levels are not worse than the coarse level enlarged by nearest neighbour
    for i in order:
        truth = S["fine"][i]["depth"]
        fine, coarse = near_truth(got[3][i][0], truth), near_truth(np.repeat(np.repeat(a[i][0], 2, 0), 2, 1), truth)
        print("image %d: within 1 %% of the truth: pyramid %.3f, stage 0 enlarged %.3f" % (i, fine, coarse))
        assert fine >= coarse
    with pytest.raises(ValueError, match="stage 0"):
        D.densify_pyramid(ctx, [dict(stages[1])], S["srcs"], S["srcs"], order, init, device=DEV)

"""hcmvs_generate_plane_prior_device against the numpy statement of the rule (tests/plane_prior_ref.py) on the analytic inputs of
tests/plane_prior_cases.py: every integer decision (the sample set, the survivors of S2 and S3, the winner and the counts of every round, the
assignments, the plane count), both averages, eps, the plane table and the prior maps are compared exactly.  The inputs carry no sample
whose planarity decision the eigen-solver's last ulp could turn (asserted on the CPU in test_plane_prior_ref.py), so S2 is exact too."""
import importlib

import numpy as np
import pytest

import plane_prior_cases as cases
import plane_prior_ref as ref
import normals_clouds

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
SEEDS = (1, 2)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


_inputs, _states = {}, {}


def case_of(name):
    if name not in _inputs:
        _inputs[name] = cases.CASES[name]()
        c = _inputs[name]
        _states[name] = ref.fitting_set(c["depth"], c["normal"], c["conf"], c["region"], c["K"])
    return _inputs[name]


def expected(name, seed):
    c = case_of(name)
    return ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=_states[name], seed=seed)


def register(ctx, vid, c, with_region=True):
    h, w = c["depth"].shape
    ctx.upload_view(vid, np.zeros((h, w), np.float32), c["K"], np.eye(3), np.zeros(3))
    if with_region:
        ctx.set_prior_region(vid, np.where(c["region"], 255, 7).astype(np.uint16), 255)


def run(torch, ctx, vid, c, with_normal=True, **params):
    h, w = c["depth"].shape
    d, n, cf = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("depth", "normal", "conf"))
    prior = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda")
    pn = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") if with_normal else None
    torch.cuda.synchronize()
    planes, st = ctx.generate_plane_prior_device(vid, d.data_ptr(), n.data_ptr(), cf.data_ptr(), prior.data_ptr(), pn.data_ptr() if with_normal else None,
                                                 binding.default_plane_prior_params(**params))
    same_inputs = all(np.array_equal(t.cpu().numpy(), c[k], equal_nan=True) for t, k in ((d, "depth"), (n, "normal"), (cf, "conf")))
    return dict(prior=prior.cpu().numpy(), prior_normal=pn.cpu().numpy() if with_normal else None, planes=planes, stats=st, inputs_untouched=same_inputs)


def assert_same(got, trace, want):
    ws, gs = want["stats"], got["stats"]
    for k in ("region_pixels", "samples", "planar_samples", "fitting_samples", "min_points", "rounds", "planes", "candidates_valid", "prior_pixels"):
        assert gs[k] == ws[k], k
    assert np.array_equal(trace["stage"], want["stage"])
    assert gs["avg_spacing_all"] == ws["avg_spacing_all"] and gs["avg_spacing"] == ws["avg_spacing"]
    assert np.float32(gs["eps"]) == np.float32(ws["eps"])
    assert np.array_equal(trace["rounds"], want["rounds"])
    assert np.array_equal(trace["assignment"], want["assignment"])
    assert len(got["planes"]) == len(want["planes"])
    for g, e in zip(got["planes"], want["planes"]):
        assert np.array_equal(g["normal"], e["normal"]) and g["n_inliers"] == e["n_inliers"] and g["box_fallback"] == e["box_fallback"]
        assert np.array_equal(g["centre"], e["centre"]) and np.array_equal(g["quad"], e["quad"])
    assert np.array_equal(got["prior"], want["prior"])
    assert np.array_equal(got["prior_normal"], want["prior_normal"])
    assert got["inputs_untouched"]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_equals_the_numpy_statement(torch, ctx, name, seed):
    c = case_of(name)
    vid = list(cases.CASES).index(name)
    register(ctx, vid, c)
    assert np.array_equal(ctx.get_prior_region(vid).astype(bool), c["region"])
    got = run(torch, ctx, vid, c, seed=seed)
    want = expected(name, seed)
    assert want["stats"]["planes"] >= 1 and want["stats"]["prior_pixels"] > 0
    print(name, seed, {k: got["stats"][k] for k in ("samples", "planar_samples", "fitting_samples", "rounds", "planes", "ms_device", "device_bytes")})
    assert_same(got, ctx.plane_prior_trace(vid), want)


def test_the_fallback_case_takes_the_box(torch, ctx):
    c = case_of("grazing")
    register(ctx, 2, c)
    got = run(torch, ctx, 2, c, seed=1)
    assert [p["box_fallback"] for p in got["planes"]] == [1]


def test_the_same_call_twice_gives_the_same_bits(torch, ctx):
    c = case_of("crease")
    register(ctx, 0, c)
    a = run(torch, ctx, 0, c, seed=3)
    ta = ctx.plane_prior_trace(0)
    b = run(torch, ctx, 0, c, seed=3)
    tb = ctx.plane_prior_trace(0)
    assert a["prior"].tobytes() == b["prior"].tobytes() and a["prior_normal"].tobytes() == b["prior_normal"].tobytes()
    assert all(np.array_equal(ta[k], tb[k]) for k in ta)
    assert {k: v for k, v in a["stats"].items() if not k.startswith("ms_")} == {k: v for k, v in b["stats"].items() if not k.startswith("ms_")}
    # another seed, another result: the seed is really read (the neighbourhood: the k = 20 test below)
    other = run(torch, ctx, 0, c, seed=4)
    assert not np.array_equal(other["prior"], a["prior"])


def test_without_the_optional_outputs(torch, ctx):
    c = case_of("two_blobs")
    register(ctx, 3, c)
    a = run(torch, ctx, 3, c, with_normal=False, seed=1)
    assert np.array_equal(a["prior"], expected("two_blobs", 1)["prior"])


def zero_result(got, c):
    return not got["prior"].any() and not got["prior_normal"].any() and got["planes"] == [] and got["stats"]["planes"] == 0 and got["inputs_untouched"]


def test_degenerate_inputs_give_an_all_zero_prior(torch, ctx):
    c = dict(case_of("two_blobs"))
    # no region registered
    register(ctx, 10, c, with_region=False)
    assert not ctx.get_prior_region(10).any()
    got = run(torch, ctx, 10, c)
    assert zero_result(got, c) and got["stats"]["region_pixels"] == 0
    # a region no pixel belongs to (the label does not occur); removing a region
    ctx.set_prior_region(10, np.full((4, 5), 7, np.uint16), 255)
    got = run(torch, ctx, 10, c)
    assert zero_result(got, c) and got["stats"]["region_pixels"] == 0
    ctx.set_prior_region(10, None)
    assert not ctx.get_prior_region(10).any()
    # ten samples: one fewer than a neighbourhood and its centre
    few = np.zeros_like(c["region"]); few[20, 10:20] = True
    c10 = dict(c, region=few, conf=np.full_like(c["conf"], 0.05))
    register(ctx, 10, c10)
    got = run(torch, ctx, 10, c10)
    assert zero_result(got, c10) and got["stats"]["samples"] == 10 and got["stats"]["region_pixels"] == 10
    want = ref.generate(c10["depth"], c10["normal"], c10["conf"], c10["region"], c10["K"])
    assert want["stats"]["samples"] == 10 and not want["prior"].any()
    # no usable depth anywhere (NaN, infinity, zero, negative)
    bad = c["depth"].copy(); bad[::4] = np.nan; bad[1::4] = np.inf; bad[2::4] = 0; bad[3::4] = -1
    cb = dict(c, depth=bad)
    register(ctx, 10, cb)
    got = run(torch, ctx, 10, cb)
    assert zero_result(got, cb) and got["stats"]["samples"] == 0 and got["stats"]["region_pixels"] == int(c["region"].sum())
    # every sample non-planar enough: nothing survives S2 when the threshold cannot be met
    got = run(torch, ctx, 10, c, planarity_min=2.0)
    assert got["stats"]["planar_samples"] == 0 and not got["prior"].any()
    # releasing the view drops the region
    register(ctx, 10, c)
    assert ctx.get_prior_region(10).any()
    ctx.upload_view(10, np.zeros(c["depth"].shape, np.float32), c["K"], np.eye(3), np.zeros(3))
    assert not ctx.get_prior_region(10).any()


def test_refusals(torch, ctx):
    c = case_of("two_blobs")
    h, w = c["depth"].shape
    register(ctx, 20, c)
    d, n, cf = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("depth", "normal", "conf"))
    prior = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    pn = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    good = dict(vid=20, depth=d.data_ptr(), normal=n.data_ptr(), conf=cf.data_ptr(), prior=prior.data_ptr(), pn=pn.data_ptr(), params={})

    def refused(**kw):
        a = dict(good); a.update(kw)
        with pytest.raises(binding.HcmvsError) as e:
            ctx.generate_plane_prior_device(a["vid"], a["depth"], a["normal"], a["conf"], a["prior"], a["pn"], binding.default_plane_prior_params(**a["params"]))
        assert e.value.code == binding.ERR_INVALID
        return str(e.value)

    for k in ("depth", "normal", "conf", "prior"):
        assert "null" in refused(**{k: None})
    assert "unknown view" in refused(vid=999)
    for params, word in ((dict(probability=0.0), "probability"), (dict(probability=1.0), "probability"), (dict(probability=float("nan")), "probability"),
                         (dict(min_points_div=0.0), "min_points_div"), (dict(min_points_div=float("inf")), "min_points_div"),
                         (dict(epsilon_mul=-1.0), "epsilon_mul"), (dict(epsilon_mul=float("nan")), "epsilon_mul"),
                         (dict(n_neighbors=2), "n_neighbors"), (dict(n_neighbors=32), "n_neighbors"), (dict(max_rounds=0), "max_rounds")):
        assert word in refused(params=params)
    assert "overlaps the depth" in refused(prior=d.data_ptr())
    assert "overlaps the conf" in refused(prior=cf.data_ptr() + 4 * (h * w - 1))
    assert "overlaps the normal" in refused(prior=n.data_ptr() + 8)
    assert "overlaps" in refused(pn=d.data_ptr())
    assert "overlaps" in refused(pn=prior.data_ptr())
    # an unsupported K
    K = c["K"].copy(); K[2, 0] = 1e-3
    ctx.upload_view(21, np.zeros((h, w), np.float32), K, np.eye(3), np.zeros(3))
    assert "K" in refused(vid=21)
    # a rescaled view has no region
    ctx.upload_view(22, np.random.RandomState(0).uniform(size=(h, w)).astype(np.float32), c["K"], np.eye(3), np.zeros(3))
    ctx.rescale_view(22, 23, 0.5)
    with pytest.raises(binding.HcmvsError) as e:
        ctx.set_prior_region(23, np.full((h, w), 255, np.uint16), 255)
    assert e.value.code == binding.ERR_INVALID and "rescale" in str(e.value)
    with pytest.raises(binding.HcmvsError):
        ctx.set_prior_region(999, np.full((h, w), 255, np.uint16), 255)
    # nothing of the refused calls ran: the good call still works
    planes, st = ctx.generate_plane_prior_device(20, good["depth"], good["normal"], good["conf"], good["prior"], good["pn"])
    assert st["planes"] == 1


def test_the_region_is_resampled_as_the_ignore_mask_is(ctx):
    c = case_of("two_blobs")
    register(ctx, 30, c, with_region=False)
    rng = np.random.RandomState(5)
    labels = rng.choice(np.array([0, 9, 255], np.uint16), size=(37, 53))
    ctx.set_prior_region(30, labels, 255)
    ctx.set_ignore_mask(30, labels, [255])
    assert np.array_equal(ctx.get_prior_region(30), 1 - ctx.ignore_mask(30))
    ctx.set_ignore_mask(30, None, [])


def test_the_output_feeds_the_depth_prior_entry(torch, ctx):
    c = case_of("two_blobs")
    register(ctx, 3, c)
    h, w = c["depth"].shape
    d, n, cf = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("depth", "normal", "conf"))
    prior = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    ctx.generate_plane_prior_device(3, d.data_ptr(), n.data_ptr(), cf.data_ptr(), prior.data_ptr())
    ctx.set_depth_prior_device(3, prior.data_ptr())
    ctx.set_depth_prior_device(3, None)


def test_point_normals_keep_their_bits_after_the_search_moved(ctx):
    """hcmvs_estimate_point_normals on cloud "b" of normals_clouds.py (outliers and a far cluster: the climb over several levels): the bits
    the library gave before the search moved into the header it shares with the plane priors (knn_grid.h), recorded on the device"""
    import os
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_normals_cloud_b.npz"))
    K = np.array([[20.0, 0, 7.5], [0, 20.0, 7.5], [0, 0, 1]])
    for i, centre in enumerate(normals_clouds.CENTRES):
        ctx.upload_view(40 + i, np.zeros((16, 16), np.float32), K, np.eye(3), centre)
    xyz, first = normals_clouds.cloud("b")
    for k in (16, 32):
        got = ctx.estimate_point_normals(xyz, np.ones(len(xyz), np.uint32), first + 40, k)
        assert got.tobytes() == gold["k%d" % k].tobytes(), k


@pytest.mark.parametrize("k", [20])
def test_a_wider_neighbourhood_runs_the_second_kernel_instances(torch, ctx, k):
    """n_neighbors above 16: the planarity and spacing kernels with the candidate list of 32, against the numpy statement"""
    c = case_of("two_blobs")
    register(ctx, 3, c)
    got = run(torch, ctx, 3, c, seed=2, n_neighbors=k)
    want = ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], seed=2, n_neighbors=k)
    assert not want["flags"]["S2"].any() and want["stats"]["planes"] >= 1
    assert want["stats"]["planar_samples"] != expected("two_blobs", 2)["stats"]["planar_samples"]      # the neighbourhood is really read
    assert_same(got, ctx.plane_prior_trace(3), want)


def test_huge_depths_are_no_samples(torch, ctx):
    """a depth whose point ray * depth is not finite in float32 is not a sample (the search grid is undefined for such points): the call
    ends, and gives what it gives with those pixels' depths invalid"""
    c = dict(case_of("two_blobs"))
    d = c["depth"].copy()
    ys, xs = np.nonzero(c["region"])
    K = c["K"].copy(); K[0, 0] = K[1, 1] = 20.0      # a wide camera: |ray_x| > 1.3 right of column 75, where the largest depths overflow
    far = (xs > 75) & (ys % 3 == 0)
    d[ys[far], xs[far]] = np.float32(3.4e38)
    c = dict(c, depth=d, K=K)
    register(ctx, 4, c)
    got = run(torch, ctx, 4, c, seed=1)
    want = ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], seed=1)
    assert want["stats"]["samples"] < int((c["region"] & (c["conf"] < np.float32(0.18))).sum())       # some were refused as samples
    assert_same(got, ctx.plane_prior_trace(4), want)


# Measured on the CPU (the numpy statement feeding the oracle's prior path, device association), next to EFFECT_WITHOUT / EFFECT_WITH of
# tests/test_gpu_prior.py and on its scene: the label is the pixels whose ground truth is the scene's plane (48 % of the low-contrast region:
# the sphere covers the rest and gets no prior); one plane is found from 2 719 fitting-set samples.  Fraction of the region's pixels
# within 1 % of the ground truth after outer iteration 2: 0.1847 without the generated prior, 0.4766 with it.
PLANE_EFFECT_WITHOUT, PLANE_EFFECT_WITH = 0.1847, 0.4766


def test_a_generated_prior_repairs_the_low_contrast_region(torch, ctx):
    """the scene of test_gpu_prior.py::test_the_prior_repairs_a_low_contrast_region with a GENERATED prior: labels = the plane's pixels, maps
    from prior_cases.start_maps, the prior from the device, then outer iteration 2 with and without it.  The gain must be at least half of
    what the CPU gives"""
    import prior_cases as PC
    synth = importlib.import_module("hc-mvs_amd.synth")
    views = [dict(v) for v in synth.make_views(96, 80, 90.0, 3, seed=12)]
    g = views[0]["gray"].copy(); reg = (slice(24, 56), slice(28, 72))
    g[reg] = g[reg].mean() + (g[reg] - g[reg].mean()) * 0.05
    views[0]["gray"] = g.astype(np.float32)
    d, n, c, dmin, dmax = PC.start_maps(views, 0)
    gt = views[0]["depth"]
    sc = synth.Scene(12)
    K = views[0]["K"]
    xs, ys = np.meshgrid(np.arange(96.0), np.arange(80.0))
    ray = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)
    tp = sc.plane_d / (ray @ sc.plane_n)
    label = np.abs(gt - tp) < 1e-4 * tp
    for i, v in enumerate(views):
        ctx.upload_view(800 + i, v["gray"], v["K"], v["R"], v["C"])
    ctx.set_prior_region(800, np.where(label, 255, 0).astype(np.uint16), 255)
    dd, dn, dc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (d, n, c))
    prior = torch.zeros((80, 96), dtype=torch.float32, device="cuda")
    planes, st = ctx.generate_plane_prior_device(800, dd.data_ptr(), dn.data_ptr(), dc.data_ptr(), prior.data_ptr())
    assert st["planes"] >= 1
    pg = binding.default_params(adapthalfwin=6, n_estimation_iters=2, it_external=2, n_external_iters=3, seed=11, **PC.KW)
    ctx.set_viewspread(False)
    ctx.set_prior_params()                                                     # the reference's defaults: 0.5, 0.2, 2
    frac = []
    for p in (None, prior.data_ptr()):
        ctx.set_depth_prior_device(800, p)
        out, _, _ = ctx.estimate(800, [801, 802, 803], pg, dmin, dmax, d, n)
        ok = (out > 0) & (np.abs(out - gt) < 0.01 * gt)
        frac.append(float(ok[reg].mean()))
    ctx.set_depth_prior_device(800, None)
    print("fraction within 1 %% in the region: without %.4f, with the generated prior %.4f (planes %d)" % (frac[0], frac[1], st["planes"]))
    assert PLANE_EFFECT_WITH - PLANE_EFFECT_WITHOUT >= 0.1
    assert frac[1] - frac[0] >= 0.5 * (PLANE_EFFECT_WITH - PLANE_EFFECT_WITHOUT)

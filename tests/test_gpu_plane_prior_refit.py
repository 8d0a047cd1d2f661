"""hcmvs_generate_plane_prior_device with refit_iters > 0 (least-squares steps on the winner of a round) against
its statement tests/plane_prior_refit_ref.py: everything test_gpu_plane_prior.assert_same compares, the refit trace (steps, counts and the
plane as bits), the cluster trace and the stats, exactly.  refit_iters = 0 gives the bytes of a params struct that never set the field; one
input meets each reason the steps end for; the end-to-end scene of test_gpu_plane_prior.py with refit_iters = 4 agrees with the CPU (the
statement feeding the oracle) bit for bit."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_plane_prior_refit as G  # noqa: E402
import plane_prior_cases as cases  # noqa: E402
import plane_prior_ref as ref  # noqa: E402
import plane_prior_refit_ref as refit  # noqa: E402
import test_gpu_plane_prior as GP  # noqa: E402
import test_gpu_plane_prior_cluster as GC  # noqa: E402

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
SEEDS = (1, 2)
NAMES = list(cases.CASES) + ["doorway"]

torch = GP.torch
ctx = GP.ctx


def expected(name, **params):
    c, state = GC.case_of(name)
    return refit.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **params)


def device(torch, ctx, name, **params):
    c, _ = GC.case_of(name)
    vid = 200 + NAMES.index(name)
    GP.register(ctx, vid, c)
    got = GP.run(torch, ctx, vid, c, **params)
    return got, ctx.plane_prior_trace(vid), ctx.plane_prior_cluster_trace(), ctx.get_plane_prior_refit_trace()


def assert_same(got, trace, clusters, refits, want):
    GC.assert_same(got, trace, clusters, want)
    steps, planes = refits
    assert steps.dtype == np.int32 and np.array_equal(steps, want["refits"])
    assert planes.dtype == np.float32 and planes.tobytes() == want["refit_planes"].tobytes()
    assert got["stats"]["refit_rounds"] == want["stats"]["refit_rounds"] and got["stats"]["refit_steps"] == want["stats"]["refit_steps"]
    assert got["stats"]["refit_steps"] == int(steps[:, 1].sum()) and got["stats"]["refit_rounds"] == int((steps[:, 1] > 0).sum())


def plain(stats):
    return {k: v for k, v in stats.items() if not k.startswith("ms_")}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("iters", [1, 4])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_device_equals_the_statement(torch, ctx, name, iters, seed):
    want = expected(name, refit_iters=iters, seed=seed)
    got, trace, clusters, refits = device(torch, ctx, name, refit_iters=iters, seed=seed)
    print(name, iters, seed, refits[0].tolist(), {k: got["stats"][k] for k in ("rounds", "planes", "refit_rounds", "refit_steps", "ms_rounds")})
    assert want["stats"]["planes"] >= 1 and want["stats"]["refit_steps"] >= 1
    assert_same(got, trace, clusters, refits, want)
    # the plane table carries the final normal of its round
    final = refits[1][clusters[:, 3] == 1]
    assert len(final) == len(got["planes"]) and all(np.array_equal(p["normal"], f[:3]) for p, f in zip(got["planes"], final))


@pytest.mark.parametrize("seed", SEEDS)
def test_the_refitted_plane_is_what_the_clustering_clusters(torch, ctx, seed):
    want = expected("doorway", refit_iters=4, cluster_mul=2.0, seed=seed)
    got, trace, clusters, refits = device(torch, ctx, "doorway", refit_iters=4, cluster_mul=2.0, seed=seed)
    print(seed, clusters.tolist(), refits[0].tolist())
    assert want["stats"]["planes"] == 2 and want["stats"]["refit_steps"] >= 2 and (want["clusters"][:, 1] > 1).any()
    assert_same(got, trace, clusters, refits, want)
    assert got["stats"]["cluster_left"] == int((refits[0][:, 2] - clusters[:, 2])[clusters[:, 3] == 1].sum())


def test_no_steps_give_the_bytes_of_a_struct_that_never_had_the_field(torch, ctx):
    """refit_iters = 0 against a params struct filled field by field up to cluster_mul, the last field the struct had before"""
    c, _ = GC.case_of("crease")
    GP.register(ctx, 200, c)
    h, w = c["depth"].shape
    d, n, cf = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("depth", "normal", "conf"))
    results = []
    for mul in (0.0, 2.0):
        old = binding.PlanePriorParams(255, 0.18, 0.3, 10, 0.01, 80.0, 2.0, 0.25, 256, 3, mul)
        new = binding.default_plane_prior_params(seed=3, cluster_mul=mul, refit_iters=0)
        pair = []
        for p in (old, new):
            prior = torch.full((h, w), -1.0, dtype=torch.float32, device="cuda"); pn = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
            planes, st = ctx.generate_plane_prior_device(200, d.data_ptr(), n.data_ptr(), cf.data_ptr(), prior.data_ptr(), pn.data_ptr(), p)
            pair.append((prior.cpu().numpy().tobytes(), pn.cpu().numpy().tobytes(), planes, plain(st), ctx.plane_prior_trace(200), ctx.plane_prior_cluster_trace(),
                         ctx.get_plane_prior_refit_trace()))
        a, b = pair
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and len(a[2]) == len(b[2]) >= 2
        assert all(np.array_equal(x[k], y[k]) for x, y in zip(a[2], b[2]) for k in x)
        assert all(np.array_equal(a[4][k], b[4][k]) for k in a[4]) and np.array_equal(a[5], b[5])
        assert np.array_equal(a[6][0], b[6][0]) and a[6][1].tobytes() == b[6][1].tobytes()
        assert b[3]["refit_rounds"] == 0 and b[3]["refit_steps"] == 0
        # the trace of a call without steps: the candidate's counts, and the candidate's plane, which the plane table holds
        win = b[4]["rounds"][:, 0] >= 0
        assert not b[6][0][:, :2].any() and np.array_equal(b[6][0][:, 2:], np.where(win[:, None], b[4]["rounds"][:, 1:5], 0))
        results.append(b)
    want = expected("crease", refit_iters=0, seed=3)
    assert results[0][0] == want["prior"].tobytes() and results[0][6][1].tobytes() == want["refit_planes"].tobytes()


@pytest.mark.parametrize("name,params", G.STOP_CALLS, ids=[n for n, _ in G.STOP_CALLS])
def test_every_reason_the_steps_end_for(torch, ctx, name, params):
    """two_blobs with a tiny eps: planes of a few samples, whose steps end for a band below three samples, for the count and at a fixed
    point (and the moments saturate: E = -20); the crease with min_points at the winner's cnt_0: the first step loses the count"""
    want = expected(name, **params)
    stops = set(want["refit_stops"])
    assert stops >= ({"band", "count", "fixed"} if name == "two_blobs" else {"count"})
    got, trace, clusters, refits = device(torch, ctx, name, **params)
    print(name, refits[0].tolist(), want["refit_stops"])
    assert_same(got, trace, clusters, refits, want)


def test_the_same_call_twice_gives_the_same_bits(torch, ctx):
    a = device(torch, ctx, "plane_and_sphere", refit_iters=4, seed=3)
    b = device(torch, ctx, "plane_and_sphere", refit_iters=4, seed=3)
    assert a[0]["prior"].tobytes() == b[0]["prior"].tobytes() and a[0]["prior_normal"].tobytes() == b[0]["prior_normal"].tobytes()
    assert all(np.array_equal(a[1][k], b[1][k]) for k in a[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3][0], b[3][0]) and a[3][1].tobytes() == b[3][1].tobytes()
    assert plain(a[0]["stats"]) == plain(b[0]["stats"]) and a[0]["stats"]["refit_steps"] > 0


def test_a_bad_refit_iters_is_refused(torch, ctx):
    c, _ = GC.case_of("doorway")
    GP.register(ctx, 204, c)
    h, w = c["depth"].shape
    d, n, cf = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("depth", "normal", "conf"))
    prior = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    for bad in (-1, 17, 1000):
        with pytest.raises(binding.HcmvsError) as e:
            ctx.generate_plane_prior_device(204, d.data_ptr(), n.data_ptr(), cf.data_ptr(), prior.data_ptr(), None, binding.default_plane_prior_params(refit_iters=bad))
        assert e.value.code == binding.ERR_INVALID and "refit_iters" in str(e.value)
    assert binding.default_plane_prior_params().refit_iters == 0
    planes, st = ctx.generate_plane_prior_device(204, d.data_ptr(), n.data_ptr(), cf.data_ptr(), prior.data_ptr(), None, binding.default_plane_prior_params(refit_iters=16))
    assert st["planes"] >= 1 and st["refit_steps"] >= 1


def test_end_to_end_the_device_equals_the_statement_feeding_the_oracle(torch, ctx):
    """the scene of test_gpu_plane_prior.py::test_a_generated_prior_repairs_the_low_contrast_region with refit_iters = 4: the prior of the
    device against the statement's, then outer iteration 2 with it on the device against the oracle with the statement's.  The share of
    the region within 1 % of the truth is printed (DESIGN.md section 5, D13 records it next to 0.4766); no threshold is asserted"""
    import oracle_lib as O
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
    want = refit.generate(d, n, c, label, K, refit_iters=4)
    assert want["stats"]["planes"] >= 1 and want["stats"]["refit_steps"] >= 1 and not want["flags"]["S2"].any()
    for i, v in enumerate(views):
        ctx.upload_view(900 + i, v["gray"], v["K"], v["R"], v["C"])
    ctx.set_prior_region(900, np.where(label, 255, 0).astype(np.uint16), 255)
    dd, dn, dc = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (d, n, c))
    prior = torch.zeros((80, 96), dtype=torch.float32, device="cuda")
    planes, st = ctx.generate_plane_prior_device(900, dd.data_ptr(), dn.data_ptr(), dc.data_ptr(), prior.data_ptr(), None, binding.default_plane_prior_params(refit_iters=4))
    steps, fin = ctx.get_plane_prior_refit_trace()
    assert np.array_equal(steps, want["refits"]) and fin.tobytes() == want["refit_planes"].tobytes()
    assert prior.cpu().numpy().tobytes() == want["prior"].tobytes()
    kw = dict(adapthalfwin=6, n_estimation_iters=2, it_external=2, n_external_iters=3, seed=11, **PC.KW)
    pg = binding.default_params(**kw)
    po = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, **kw)
    ctx.set_viewspread(False)
    ctx.set_prior_params()                                                     # the reference's defaults: 0.5, 0.2, 2
    ctx.set_depth_prior_device(900, prior.data_ptr())
    out, on, oc = ctx.estimate(900, [901, 902, 903], pg, dmin, dmax, d, n)
    ctx.set_depth_prior_device(900, None)
    ed, en, ec, _ = PC.estimate(views, po, dmin, dmax, d, n, prior=want["prior"], para_prior=0.5, sigma_prior=0.2, photo2geo=2)
    assert np.array_equal(out, ed) and np.array_equal(on, en) and np.array_equal(oc, ec)
    ok = (out > 0) & (np.abs(out - gt) < 0.01 * gt)
    print("fraction within 1 %% in the region with the refitted prior: %.4f (without the refit %.4f; planes %d, steps %d)" %
          (float(ok[reg].mean()), GP.PLANE_EFFECT_WITH, st["planes"], st["refit_steps"]))

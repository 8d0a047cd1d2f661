"""hcmvs_generate_plane_prior_device with cluster_mul > 0 (a plane keeps the largest connected component of its
inliers) against the numpy statement tests/plane_prior_ref.py, on the inputs of plane_prior_cases.CLUSTER_CASES and on three of
plane_prior_cases.CASES: everything test_gpu_plane_prior.assert_same compares, the cluster trace and the three cluster stats, exactly."""
import importlib

import numpy as np
import pytest

import plane_prior_cases as cases
import plane_prior_ref as ref
import test_gpu_plane_prior as GP

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
SEEDS = (1, 2)
NAMES = list(cases.CLUSTER_CASES) + ["crease", "two_blobs", "plane_and_sphere"]

torch = GP.torch
ctx = GP.ctx
_inputs, _states = {}, {}


def case_of(name):
    """the case and its fitting set (S1 .. S3 depend on neither the seed, min_points_div nor cluster_mul), made once"""
    if name in cases.CASES:
        return GP.case_of(name), GP._states[name]
    if name not in _inputs:
        _inputs[name] = cases.CLUSTER_CASES[name]()
        c = _inputs[name]
        _states[name] = ref.fitting_set(c["depth"], c["normal"], c["conf"], c["region"], c["K"])
    return _inputs[name], _states[name]


def expected(name, **params):
    c, state = case_of(name)
    return ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **params)


def device(torch, ctx, name, **params):
    c, _ = case_of(name)
    vid = 100 + NAMES.index(name)
    GP.register(ctx, vid, c)
    got = GP.run(torch, ctx, vid, c, **params)
    return got, ctx.plane_prior_trace(vid), ctx.plane_prior_cluster_trace()


def assert_same(got, trace, clusters, want):
    GP.assert_same(got, trace, want)
    assert np.array_equal(clusters, want["clusters"])
    gs, ws = got["stats"], want["stats"]
    assert np.float32(gs["cluster_eps"]) == np.float32(ws["cluster_eps"])
    assert gs["cluster_rejects"] == ws["cluster_rejects"] and gs["cluster_left"] == ws["cluster_left"]


def gap_share(case, prior):
    return float((prior[case["gap"]] > 0).mean())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mul", [2.0, 3.0])
@pytest.mark.parametrize("name", list(cases.CLUSTER_CASES))
def test_device_equals_the_statement_on_the_new_cases(torch, ctx, name, mul, seed):
    want = expected(name, cluster_mul=mul, seed=seed)
    got, trace, clusters = device(torch, ctx, name, cluster_mul=mul, seed=seed)
    print(name, mul, seed, clusters.tolist(), {k: got["stats"][k] for k in ("rounds", "planes", "cluster_rejects", "cluster_left", "ms_rounds")})
    assert want["stats"]["planes"] >= 1 and (want["clusters"][:, 1] > 1).any()         # the clustering had something to separate
    assert_same(got, trace, clusters, want)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("mul", [2.0, 3.0])
def test_islands_too_small_for_a_plane_are_rejected(torch, ctx, mul, seed):
    """min_points_div = 4: no island holds min_points samples, the only round is rejected and the prior is all zero"""
    want = expected("islands", cluster_mul=mul, seed=seed, min_points_div=4.0)
    got, trace, clusters = device(torch, ctx, "islands", cluster_mul=mul, seed=seed, min_points_div=4.0)
    assert want["stats"]["planes"] == 0 and want["stats"]["cluster_rejects"] >= 1 and not want["prior"].any()
    assert_same(got, trace, clusters, want)
    assert not got["prior"].any() and not got["prior_normal"].any() and got["planes"] == []


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["crease", "two_blobs", "plane_and_sphere"])
def test_device_equals_the_statement_on_the_existing_cases(torch, ctx, name, seed):
    want = expected(name, cluster_mul=3.0, seed=seed)
    got, trace, clusters = device(torch, ctx, name, cluster_mul=3.0, seed=seed)
    print(name, seed, clusters.tolist(), got["stats"]["ms_rounds"])
    assert want["stats"]["planes"] >= 1
    assert_same(got, trace, clusters, want)


def test_a_wide_cell_gives_the_bits_of_no_clustering(torch, ctx):
    off, toff, coff = device(torch, ctx, "doorway", seed=1)
    wide, twide, cwide = device(torch, ctx, "doorway", cluster_mul=40.0, seed=1)
    assert off["prior"].tobytes() == wide["prior"].tobytes() and off["prior_normal"].tobytes() == wide["prior_normal"].tobytes()
    assert all(np.array_equal(toff[k], twide[k]) for k in toff)
    assert [p["n_inliers"] for p in off["planes"]] == [p["n_inliers"] for p in wide["planes"]]
    assert all(np.array_equal(a["quad"], b["quad"]) and np.array_equal(a["centre"], b["centre"]) for a, b in zip(off["planes"], wide["planes"]))
    # off: 0, 0, cnt_0, 1 per round with a winner; wide: one component holding every inlier
    win = toff["rounds"][:, 0] >= 0
    assert np.array_equal(coff[win], np.stack([0 * toff["rounds"][win, 1], 0 * toff["rounds"][win, 1], toff["rounds"][win, 1], 1 + 0 * toff["rounds"][win, 1]], 1))
    assert not coff[~win].any() and np.array_equal(cwide[:, 2:], coff[:, 2:]) and (cwide[win, 1] == 1).all()
    assert off["stats"]["cluster_eps"] == 0 and off["stats"]["cluster_left"] == 0 and wide["stats"]["cluster_left"] == 0
    assert_same(off, toff, coff, expected("doorway", seed=1))


def test_a_tiny_cell_reaches_the_cap(torch, ctx):
    """cluster_mul = 1e-9: (u - u0) / cell passes 2^30 for nearly every inlier; the cells at the cap merge, as the statement has it"""
    want = expected("doorway", cluster_mul=1e-9, seed=1)
    got, trace, clusters = device(torch, ctx, "doorway", cluster_mul=1e-9, seed=1)
    print(clusters.tolist())
    assert want["clusters"][0, 0] > 100                  # many cells, most of them a sample of their own
    assert_same(got, trace, clusters, want)


def test_the_same_call_twice_gives_the_same_bits(torch, ctx):
    a, ta, ca = device(torch, ctx, "doorway", cluster_mul=2.0, seed=3)
    b, tb, cb = device(torch, ctx, "doorway", cluster_mul=2.0, seed=3)
    assert a["prior"].tobytes() == b["prior"].tobytes() and a["prior_normal"].tobytes() == b["prior_normal"].tobytes()
    assert all(np.array_equal(ta[k], tb[k]) for k in ta) and np.array_equal(ca, cb)
    assert {k: v for k, v in a["stats"].items() if not k.startswith("ms_")} == {k: v for k, v in b["stats"].items() if not k.startswith("ms_")}


def test_the_doorway_is_no_longer_painted_over(torch, ctx):
    c, _ = case_of("doorway")
    off, _, _ = device(torch, ctx, "doorway", seed=1)
    on, _, _ = device(torch, ctx, "doorway", cluster_mul=2.0, seed=1)
    print("share of the gap's pixels with a prior: off %.3f, cluster_mul 2 %.3f" % (gap_share(c, off["prior"]), gap_share(c, on["prior"])))
    assert gap_share(c, off["prior"]) > 0.5 and gap_share(c, on["prior"]) < 0.1
    assert len(off["planes"]) == 1 and len(on["planes"]) == 2
    assert off["inputs_untouched"] and on["inputs_untouched"]


def test_a_bad_cluster_mul_is_refused(torch, ctx):
    c, _ = case_of("doorway")
    GP.register(ctx, 100, c)
    h, w = c["depth"].shape
    d, n, cf = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("depth", "normal", "conf"))
    prior = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(binding.HcmvsError) as e:
            ctx.generate_plane_prior_device(100, d.data_ptr(), n.data_ptr(), cf.data_ptr(), prior.data_ptr(), None, binding.default_plane_prior_params(cluster_mul=bad))
        assert e.value.code == binding.ERR_INVALID and "cluster_mul" in str(e.value)
    assert binding.default_plane_prior_params().cluster_mul == 0.0

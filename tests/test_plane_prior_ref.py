"""The plane-prior rule as its numpy statement computes it (tests/plane_prior_ref.py) on the analytic inputs of tests/plane_prior_cases.py: per
generating plane the angle and the offset error of the plane found, and the share of the region whose prior lies within 1 % of the truth.

RECORDED holds, per case, the worst values this statement gave at the seeds 1, 2, 3, 7 and 11 (angle in degrees and relative offset per
generating plane: the largest; share: the smallest).  The asserted bound is the worst value plus a quarter of itself -- for the share,
a quarter more of the shortfall 1 - share --, the order by which the seeds differ.  The same seed gives the same bits, and no input
carries a sample whose planarity decision (S2) a last-ulp difference of an eigen-solver could turn: that is what lets the device be compared
decision by decision (test_gpu_plane_prior.py)."""
import numpy as np
import pytest

import plane_prior_cases as cases
import plane_prior_ref as ref

SEEDS = (1, 2, 3, 7, 11)
RECORDED = {
    "crease": dict(angle=[1.896, 0.6388], offset=[0.003702, 0.003988], share=0.8879),
    "plane_and_sphere": dict(angle=[0.4163], offset=[0.0003687], share=0.9847),
    "grazing": dict(angle=[0.2484], offset=[0.01045], share=0.6749),
    "two_blobs": dict(angle=[0.9492], offset=[0.005318], share=0.9550),
}
_cache = {}


def stages(name):
    """a case of either dict and its fitting set, made once"""
    if name not in _cache:
        c = (cases.CASES.get(name) or cases.CLUSTER_CASES[name])()
        _cache[name] = (c, ref.fitting_set(c["depth"], c["normal"], c["conf"], c["region"], c["K"]))
    return _cache[name]


def generate(name, seed):
    c, state = stages(name)
    return c, ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, seed=seed)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_planes_and_prior_against_the_truth(name):
    rec = RECORDED[name]
    worst_angle, worst_offset, worst_share = np.zeros(len(rec["angle"])), np.zeros(len(rec["angle"])), 1.0
    for seed in SEEDS:
        c, res = generate(name, seed)
        errs, share = cases.evaluate(c, res)
        assert all(e is not None for e in errs)
        worst_angle = np.maximum(worst_angle, [e[0] for e in errs]); worst_offset = np.maximum(worst_offset, [e[1] for e in errs])
        worst_share = min(worst_share, share)
    print(name, "angle", worst_angle, "offset", worst_offset, "share", worst_share)
    assert (worst_angle <= 1.25 * np.array(rec["angle"])).all()
    assert (worst_offset <= 1.25 * np.array(rec["offset"])).all()
    assert worst_share >= 1.0 - 1.25 * (1.0 - rec["share"])


@pytest.mark.parametrize("name", list(cases.CASES))
def test_no_input_carries_a_flagged_sample(name):
    c, state = stages(name)
    flags = state["out"]["flags"]["S2"]
    assert len(flags) == state["out"]["stats"]["samples"] > 1000 and not flags.any()
    st = state["out"]["stats"]
    assert st["samples"] > st["planar_samples"] > st["fitting_samples"] > 0.4 * st["planar_samples"]   # S2 removes some, S3 roughly the sparser half


def test_the_same_seed_gives_the_same_bits_and_another_seed_another_result():
    c, a = generate("crease", 2)
    b = ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], seed=2)       # from scratch: the shared stages are not what agrees
    assert a["prior"].tobytes() == b["prior"].tobytes() and np.array_equal(a["rounds"], b["rounds"]) and np.array_equal(a["assignment"], b["assignment"])
    assert a["stats"] == b["stats"]
    _, other = generate("crease", 3)
    assert not np.array_equal(other["rounds"], a["rounds"])


def test_the_sphere_yields_few_planes():
    for seed in SEEDS:
        c, res = generate("plane_and_sphere", seed)
        on_plane = c["planes"][0][2]
        sizes = sorted((p["n_inliers"] for p in res["planes"]), reverse=True)
        assert len(sizes) <= 4 and sizes[0] > 0.8 * res["stats"]["fitting_samples"] and sum(sizes[1:]) < 0.2 * res["stats"]["fitting_samples"]
        # the large plane is the scene's: its samples lie where the ground truth is the plane
        big = int(np.argmax([p["n_inliers"] for p in res["planes"]]))
        assert on_plane[res["assignment"] == big].mean() > 0.99


def test_the_grazing_plane_takes_the_box_and_the_crease_does_not():
    for seed in SEEDS:
        assert [p["box_fallback"] for p in generate("grazing", seed)[1]["planes"]] == [1]
        assert [p["box_fallback"] for p in generate("crease", seed)[1]["planes"]] == [0, 0]
    q = generate("grazing", 1)[1]["planes"][0]["quad"]
    assert (q * 2 == np.rint(q * 2)).all() and q[0, 0] < q[1, 0] and q[0, 1] < q[2, 1]


def test_two_blobs_share_one_plane():
    for seed in SEEDS:
        c, res = generate("two_blobs", seed)
        assert res["stats"]["planes"] == 1
        asg = res["assignment"]
        assert (asg[8:40, 6:38] == 0).sum() > 300 and (asg[44:74, 56:90] == 0).sum() > 300
        assert not res["prior"][~c["region"]].any()


def test_degenerate_inputs():
    c = cases.CASES["two_blobs"]()
    none = ref.generate(c["depth"], c["normal"], c["conf"], np.zeros_like(c["region"]), c["K"])
    assert none["stats"]["region_pixels"] == 0 and not none["prior"].any() and none["planes"] == []
    few = np.zeros_like(c["region"]); few[20, 10:20] = True
    res = ref.generate(c["depth"], c["normal"], np.full_like(c["conf"], 0.05), few, c["K"])
    assert res["stats"]["samples"] == 10 and res["stats"]["planar_samples"] == 0 and not res["prior"].any()


def test_the_draws_are_the_counter_based_stream():
    """splitmix64 on (seed, candidate, draw): the values of the mesh sampling's stream, pinned by its first outputs"""
    assert ref.mix64(0) == 0xE220A8397B1DCDAF and ref.mix64(1) == 0x910A2DEC89025CC1
    u = [ref.draw(ref.mix64(5 ^ ref.mix64(c)), k) for c in range(64) for k in range(6)]
    assert all(0.0 <= v < 1.0 for v in u) and len(set(u)) == len(u) and abs(np.mean(u) - 0.5) < 0.06
    assert ref.draw_below(ref.mix64(1), 0, 1) == 0

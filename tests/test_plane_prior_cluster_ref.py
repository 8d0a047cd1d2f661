"""The plane-prior rule with inlier clustering as its numpy statement computes it (tests/plane_prior_ref.py
with cluster_mul > 0): on the inputs of plane_prior_cases.CLUSTER_CASES it separates what the unclustered rule paints across -- the figures
in the assertions follow from the rule (components, ties, the rejected round), none is a value the device gave.  That cluster_mul = 0
leaves the unclustered rule's bits is held by tests/test_plane_prior_golden.py."""
import numpy as np
import pytest

import plane_prior_ref as ref
import test_plane_prior_ref as TR

SEEDS = (1, 2)
stages = TR.stages


def generate(name, **params):
    c, state = stages(name)
    return c, ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, **params)


def same_bits(a, b):
    """the maps, the round trace, the flags, every stat of b and the planes, compared exactly"""
    for k in ("prior", "prior_normal", "stage", "assignment", "rounds"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(a["flags"]["S2"], b["flags"]["S2"])
    for k, v in b["stats"].items():
        assert a["stats"][k] == v and type(a["stats"][k]) is type(v), k
    assert len(a["planes"]) == len(b["planes"])
    for p, q in zip(a["planes"], b["planes"]):
        assert set(p) == set(q)
        for k in q:
            assert np.asarray(p[k]).tobytes() == np.asarray(q[k]).tobytes(), k


def sizes(res):
    return [p["n_inliers"] for p in res["planes"]]


def gap_share(c, res):
    return float((res["prior"][c["gap"]] > 0).mean())


@pytest.mark.parametrize("name", list(TR.cases.CLUSTER_CASES))
def test_no_new_input_carries_a_flagged_sample(name):
    c, state = stages(name)
    flags = state["out"]["flags"]["S2"]
    assert len(flags) == state["out"]["stats"]["samples"] > 400 and not flags.any()       # (the islands: nine squares of 64 pixels, a tenth of them bad)
    assert state["out"]["stats"]["fitting_samples"] > 0.4 * state["out"]["stats"]["planar_samples"] > 0


@pytest.mark.parametrize("seed", SEEDS)
def test_the_doorway_becomes_two_planes(seed):
    c, off = generate("doorway", seed=seed)
    assert len(off["planes"]) == 1 and gap_share(c, off) > 0.5
    assert int(c["gap"].sum()) == 64 * 20
    for mul in (2.0, 3.0):
        _, on = generate("doorway", cluster_mul=mul, seed=seed)
        s = sizes(on)
        assert len(s) == 2 and s[0] == 1606 and 954 <= s[1] <= 957
        assert gap_share(c, on) < 0.1
        print("doorway", seed, mul, s, "gap pixels with a prior:", int((on["prior"][c["gap"]] > 0).sum()), "off:", int((off["prior"][c["gap"]] > 0).sum()))
        # the first round met both walls as components; what it left, the second round found
        assert on["clusters"][0, 1] >= 2 and on["clusters"][0, 2] == s[0] and on["stats"]["cluster_left"] >= s[1]
        asg = on["assignment"]
        left, right = set(np.unique(asg[:, :38]).tolist()) - {-1}, set(np.unique(asg[:, 58:]).tolist()) - {-1}
        assert not (asg[:, 38:58] >= 0).any() and len(left) == 1 and len(right) == 1 and left | right == {0, 1}   # a wall each


def test_the_islet_is_a_plane_of_its_own_or_stays_free():
    c, a = generate("islet", cluster_mul=2.0, seed=1)
    assert sizes(a)[1:] == [46] and a["clusters"][0, 1] == 2
    assert (a["assignment"][30:38, 78:86] == 1).sum() == 46
    c, b = generate("islet", cluster_mul=2.0, seed=2)
    assert len(b["planes"]) == 1 and sizes(b) == sizes(a)[:1]
    assert b["rounds"][1:, 0].tolist() == [-1, -1] and not b["clusters"][1:].any()          # two failed rounds end the detection
    assert (b["assignment"][30:38, 78:86] == -1).all() and not b["prior"][30:38, 78:86].any()
    assert b["stats"]["cluster_left"] == 46 and b["stats"]["cluster_rejects"] == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_islands_below_min_points_are_rejected(seed):
    c, res = generate("islands", cluster_mul=2.0, seed=seed, min_points_div=4.0)
    st = res["stats"]
    assert st["min_points"] == 73 and ref.fail_limit(0.01, 73, st["fitting_samples"], 256) == 1
    assert res["clusters"].tolist() == [[res["clusters"][0, 0], 8, 51, 0]] and st["rounds"] == 1
    assert res["rounds"][0, 0] >= 0 and res["rounds"][0, 1] >= 73                           # the trace keeps the winner and its unclustered counts
    assert st["planes"] == 0 and st["cluster_rejects"] == 1 and st["cluster_left"] == 0
    assert not res["prior"].any() and not res["prior_normal"].any() and (res["assignment"] == -1).all()


def test_islands_become_planes_one_by_one():
    for seed in SEEDS:
        c, res = generate("islands", cluster_mul=2.0, seed=seed, min_points_div=80.0)
        assert sizes(res) == [51, 51, 36, 36, 33, 32, 31, 23]                                 # two natural ties: the smallest (cv, cu) first
        acc = res["clusters"][res["clusters"][:, 3] == 1]
        assert acc[:, 1].tolist() == [8, 7, 6, 5, 4, 3, 2, 1] and acc[:, 2].tolist() == sizes(res)
        failed = int((res["rounds"][:, 0] < 0).sum())
        assert failed == (1 if seed == 1 else 0) and res["stats"]["rounds"] == 8 + failed
        # every plane lies inside one square
        for i in range(8):
            ys, xs = np.nonzero(res["assignment"] == i)
            assert ys.max() - ys.min() < 8 and xs.max() - xs.min() < 8


def test_a_tie_goes_to_the_smallest_cell():
    c, res = generate("mirror", cluster_mul=2.0, seed=1)
    assert sizes(res) == [864, 864] and res["clusters"][:, 1].tolist() == [2, 1]
    n = res["planes"][0]["normal"]
    assert np.array_equal(np.abs(n), [0, 0, 1])
    b1, b2 = ref.frame(n)
    assert np.array_equal(b1, [0, n[2], 0]) and np.array_equal(b2, [-1, 0, 0])         # v = -x: the smallest cv is the largest x
    assert (np.nonzero(res["assignment"] == 0)[1] >= 60).all() and (np.nonzero(res["assignment"] == 1)[1] < 36).all()


@pytest.mark.parametrize("name", ["doorway", "crease"])
def test_a_wide_cell_changes_nothing(name):
    for seed in SEEDS:
        _, off = generate(name, seed=seed)
        _, wide = generate(name, cluster_mul=40.0, seed=seed)
        same_bits(wide, {k: v for k, v in off.items() if k != "stats"} | dict(stats={k: v for k, v in off["stats"].items() if k != "cluster_eps"}))
        assert np.array_equal(wide["clusters"][:, 2:], off["clusters"][:, 2:]) and wide["stats"]["cluster_eps"] > 0


def test_an_unusable_cell_clusters_nothing():
    """float32(avg * mul) underflows to 0 (mul the smallest float32, avg below a half): all inliers are one component"""
    _, off = generate("doorway", seed=1)
    assert 0 < off["stats"]["avg_spacing"] < 0.5
    _, tiny = generate("doorway", cluster_mul=1e-45, seed=1)
    assert tiny["stats"]["cluster_eps"] == 0 and tiny["prior"].tobytes() == off["prior"].tobytes()
    assert tiny["clusters"].tolist() == [[0, 1, off["rounds"][0, 1], 1]]

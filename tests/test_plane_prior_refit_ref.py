"""The plane-prior rule with the least-squares refit of a round's winner as its statement computes it
(tests/plane_prior_refit_ref.py), on the analytic inputs of tests/plane_prior_cases.py.

With refit_iters = 0 the statement returns what tests/plane_prior_ref.py returns.  With refit_iters = 4, at the seeds 1, 2, 3, 7 and 11: the
worst angle per generating plane is at most half of the no-refit value recorded in tests/test_plane_prior_ref.py (RECORDED there), the worst
share of the region within 1 % of the truth is not below the no-refit share, and REFIT_RECORDED holds the statement's own worst values,
asserted with the bound of that file: the worst value plus a quarter of itself, for the share a quarter more of the shortfall.
tests/golden/plane_prior_refit_statement.json holds what the statement returns (tests/golden/make_golden_plane_prior_refit.py)."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_plane_prior_refit as G  # noqa: E402
import plane_prior_cases as cases  # noqa: E402
import plane_prior_ref as ref  # noqa: E402
import plane_prior_refit_ref as refit  # noqa: E402
import test_plane_prior_ref as TR  # noqa: E402

SEEDS = TR.SEEDS
REFIT_RECORDED = {
    "crease": dict(angle=[0.04264, 0.06942], offset=[0.0001329, 0.0009493], share=0.9821),
    "plane_and_sphere": dict(angle=[0.004161], offset=[0.00004071], share=0.9863),
    "grazing": dict(angle=[0.007353], offset=[0.001197], share=0.9689),
    "two_blobs": dict(angle=[0.02639], offset=[0.00007542], share=0.9574),
}
_results = {}

with open(G.PATH) as f:
    GOLDEN = json.load(f)


def generate(name, seed, **params):
    """refit_iters = 4 unless given; every result is made once"""
    params.setdefault("refit_iters", 4)
    key = (name, seed, tuple(sorted(params.items())))
    if key not in _results:
        c, state = TR.stages(name)
        _results[key] = refit.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, seed=seed, **params)
    return TR.stages(name)[0], _results[key]


@pytest.mark.parametrize("mul", [0.0, 2.0])
@pytest.mark.parametrize("name", ["crease", "doorway"])
def test_without_steps_the_statement_is_the_one_without_the_refit(name, mul):
    c, state = TR.stages(name)
    for seed in (1, 2):
        want = ref.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], state=state, seed=seed, cluster_mul=mul)
        _, got = generate(name, seed, refit_iters=0, cluster_mul=mul)
        for k in ("prior", "prior_normal", "stage", "assignment", "rounds", "clusters"):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
        assert {k: v for k, v in got["stats"].items() if not k.startswith("refit_")} == want["stats"]
        assert len(got["planes"]) == len(want["planes"]) >= 1
        for g, e in zip(got["planes"], want["planes"]):
            assert set(g) == set(e) and all(np.array_equal(g[k], e[k]) for k in e)
        # what the refit's trace says of a call without it: the candidate's counts and plane
        win = got["rounds"][:, 0] >= 0
        assert np.array_equal(got["refits"][:, :2], np.zeros((len(win), 2))) and np.array_equal(got["refits"][:, 2:], np.where(win[:, None], got["rounds"][:, 1:5], 0))
        assert got["stats"]["refit_rounds"] == 0 and got["stats"]["refit_steps"] == 0 and got["refit_stops"] == [None] * len(win)
        assert not got["refit_planes"][~win].any() and (np.abs(np.linalg.norm(got["refit_planes"][win, :3], axis=1) - 1) < 1e-6).all()


@pytest.mark.parametrize("name", list(cases.CASES))
def test_refitted_planes_and_prior_against_the_truth(name):
    before, rec = TR.RECORDED[name], REFIT_RECORDED[name]
    worst_angle, worst_offset, worst_share = np.zeros(len(rec["angle"])), np.zeros(len(rec["angle"])), 1.0
    for seed in SEEDS:
        c, res = generate(name, seed)
        errs, share = cases.evaluate(c, res)
        assert all(e is not None for e in errs)
        worst_angle = np.maximum(worst_angle, [e[0] for e in errs]); worst_offset = np.maximum(worst_offset, [e[1] for e in errs])
        worst_share = min(worst_share, share)
        assert res["stats"]["refit_steps"] > 0 and res["stats"]["refit_rounds"] > 0
    print(name, "angle", worst_angle, "offset", worst_offset, "share", worst_share)
    assert (worst_angle <= 0.5 * np.array(before["angle"])).all()           # the refit at least halves the no-refit angle
    assert worst_share >= before["share"]                                    # and does not lose share
    assert (worst_angle <= 1.25 * np.array(rec["angle"])).all()
    assert (worst_offset <= 1.25 * np.array(rec["offset"])).all()
    assert worst_share >= 1.0 - 1.25 * (1.0 - rec["share"])


def test_the_same_seed_gives_the_same_bits_and_another_seed_another_result():
    c, a = generate("crease", 2)
    b = refit.generate(c["depth"], c["normal"], c["conf"], c["region"], c["K"], seed=2, refit_iters=4)       # from scratch
    for k in ("prior", "prior_normal", "rounds", "assignment", "refits", "refit_planes"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["stats"] == b["stats"] and a["refit_stops"] == b["refit_stops"]
    _, other = generate("crease", 3)
    assert not np.array_equal(other["refit_planes"], a["refit_planes"])


def test_a_round_ends_at_a_fixed_point_before_the_steps_are_exhausted():
    hit = 0
    for name in cases.CASES:
        for seed in SEEDS:
            _, res = generate(name, seed)
            for row, stop in zip(res["refits"], res["refit_stops"]):
                if stop == "fixed":
                    assert row[0] <= 4 and row[1] == row[0] - 1          # the last step solved repeated its predecessor: it is not kept again
                    hit += row[0] < 4
                elif stop == "iters":
                    assert row[0] == row[1] == 4
    assert hit >= 4
    _, res = generate("grazing", 1)
    assert res["refits"][0, :2].tolist() == [2, 1] and res["refit_stops"] == ["fixed"]


def test_the_steps_do_not_wait_for_the_counts_to_grow():
    """the grazing floor: at no seed does a step raise a count the winner had, yet the step is kept, and over the seeds the worst refitted
    normal is 30 times closer to the truth than the worst candidate's"""
    worst_on = worst_off = 0.0
    for seed in SEEDS:
        c, res = generate("grazing", seed)
        _, off = generate("grazing", seed, refit_iters=0)
        assert (res["refits"][0, 2:] <= off["rounds"][0, 1:5]).all() and res["refits"][0, 1] >= 1
        worst_on = max(worst_on, cases.evaluate(c, res)[0][0][0]); worst_off = max(worst_off, cases.evaluate(c, off)[0][0][0])
    assert worst_on * 30 < worst_off


def test_the_plane_counts_and_the_fallbacks_are_those_without_the_refit():
    for seed in SEEDS:
        assert [p["box_fallback"] for p in generate("grazing", seed)[1]["planes"]] == [1]
        assert [p["box_fallback"] for p in generate("crease", seed)[1]["planes"]] == [0, 0]
        c, res = generate("two_blobs", seed)
        assert res["stats"]["planes"] == 1
        asg = res["assignment"]
        assert (asg[8:40, 6:38] == 0).sum() > 300 and (asg[44:74, 56:90] == 0).sum() > 300
        assert not res["prior"][~c["region"]].any()
        c, res = generate("plane_and_sphere", seed)
        sizes = sorted((p["n_inliers"] for p in res["planes"]), reverse=True)
        assert len(sizes) <= 4 and sizes[0] > 0.8 * res["stats"]["fitting_samples"] and sum(sizes[1:]) < 0.2 * res["stats"]["fitting_samples"]
        big = int(np.argmax([p["n_inliers"] for p in res["planes"]]))
        assert c["planes"][0][2][res["assignment"] == big].mean() > 0.99


def test_every_stop_is_met():
    stops = {s for name, p in G.STOP_CALLS for s in generate(name, **p)[1]["refit_stops"]}
    assert {"band", "count", "fixed"} <= stops
    name, p = G.STOP_CALLS[1]
    _, res = generate(name, **p)
    assert res["refit_stops"] == ["count"] and res["refits"][0, :2].tolist() == [1, 0] and res["refits"][0, 2] == res["rounds"][0, 1] == res["stats"]["min_points"]
    assert np.array_equal(res["planes"][0]["normal"], res["refit_planes"][0, :3])      # step 0 is kept: the candidate's plane


def test_the_moments_do_not_depend_on_the_order_and_decode_from_any_split():
    c, state = TR.stages("crease")
    pix, P, N = state["fit"]
    O, E = [float(v) for v in P[17]], refit.refit_scale(np.float32(0.18))
    assert E == -2
    sums = refit.moment_sums(P[:500], O, E)
    perm = np.random.RandomState(0).permutation(500)
    assert refit.moment_sums(P[:500][perm], O, E) == sums
    part = [a + b for a, b in zip(refit.moment_sums(P[:123], O, E), refit.moment_sums(P[123:500], O, E))]
    assert part == sums
    for t in sums:
        hi, lo = refit.split_words(t)
        assert (hi << 32) + lo == t and 0 <= lo < 1 << 32


def test_the_file_holds_the_calls_the_generator_lists():
    assert [(r["case"], r["params"]) for r in GOLDEN] == [(n, p) for n, p in G.calls(cases.CASES)]
    assert len(GOLDEN) == 16 + 2 + 2


@pytest.mark.parametrize("rec", GOLDEN, ids=["%s-%s" % (r["case"], "-".join("%s=%s" % kv for kv in r["params"].items())) for r in GOLDEN])
def test_the_statement_returns_the_recorded_bits(rec):
    p = dict(rec["params"])
    _, got = generate(rec["case"], p.pop("seed"), **p)
    enc = json.loads(json.dumps(G.encode(got)))
    for part in ("arrays", "stats"):
        assert set(enc[part]) == set(rec[part])
        for k, v in rec[part].items():
            assert enc[part][k] == v and type(enc[part][k]) is type(v), (part, k)
    assert enc["planes"] == rec["planes"] and enc["stops"] == rec["stops"] and enc["steps"] == rec["steps"]

"""The speckle filter on the CPU: the library's host form (hc-mvs_amd/csrc/speckle_host.h, a sequential flood
fill, through tests/speckle_host_shim.cpp) against the numpy statement (tests/speckle_ref.py, connected components of the edge graph) on
every case of tests/speckle_cases.py, bit for bit; and the filter's effect on the final maps of two oracle estimates, as exact counts.

    python tests/test_speckle_ref.py        prints the EFFECT table below"""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import speckle_cases as SC
import speckle_lib as SL
import speckle_ref as R

synth = importlib.import_module("hc-mvs_amd.synth")


def _same(got, want, what):
    for key in ("depth", "normal", "conf", "labels"):
        if want[key] is None:
            assert got[key] is None
            continue
        assert R.same_bits(got[key], want[key]), "%s: %s differs at %d elements" % (what, key, int((got[key] != want[key]).sum()))
    assert {k: got["stats"][k] for k in R.COUNTERS} == want["stats"], what


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_form_equals_the_statement(name):
    case = SC.by_name(name)
    n, c = SC.aux(case["depth"])
    want = R.remove_speckles(case["depth"], n, c, SC.thr_of(case), case["speckle_size"])
    got = SL.host(case["depth"], n, c, SC.thr_of(case), case["speckle_size"])
    _same(got, want, name)
    # without the optional maps, and without the labels
    got = SL.host(case["depth"], None, None, SC.thr_of(case), case["speckle_size"], want_labels=False)
    assert R.same_bits(got["depth"], want["depth"]) and got["stats"] == want["stats"]
    # untouched where nothing is removed: every other value is left bit for bit
    kept = ~((want["labels"] >= 0) & (want["depth"] == 0))
    assert R.same_bits(got["depth"][kept], case["depth"][kept])


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_form_is_idempotent(name):
    case = SC.by_name(name)
    n, c = SC.aux(case["depth"])
    once = SL.host(case["depth"], n, c, SC.thr_of(case), case["speckle_size"])
    twice = SL.host(once["depth"], once["normal"], once["conf"], SC.thr_of(case), case["speckle_size"])
    for key in ("depth", "normal", "conf"):
        assert R.same_bits(twice[key], once[key]), key
    assert twice["stats"]["n_removed"] == 0 and twice["stats"]["n_small"] == 0
    assert twice["stats"]["n_valid"] == once["stats"]["n_valid"] - once["stats"]["n_removed"]


def test_the_cases_hold_what_they_claim():
    st = lambda name: R.remove_speckles(SC.by_name(name)["depth"], speckle_size=SC.by_name(name)["speckle_size"])["stats"]
    s = st("serpentine_64x48")
    assert s["n_segments"] == 1 and s["largest"] == 24 * 64 + 24 and s["n_removed"] == 0
    assert st("serpentine_64x48_removed")["n_removed"] == 24 * 64 + 24
    s = st("serpentine_517x259")
    assert s["n_segments"] == 1 + 129 and s["n_small"] == 129 and s["n_removed"] == 129 * 516 and s["largest"] == 130 * 517 + 129
    s = st("comb_131x37")
    assert s["n_segments"] == 1 and R.segments(SC.by_name("comb_131x37")["depth"])[0].max() == 0
    s = st("checkerboard_70x33")
    assert s["n_segments"] == 70 * 33 == s["n_small"] == s["n_removed"] and s["largest"] == 1
    assert st("full_67x35_exact")["n_removed"] == 0 and st("full_67x35_one_more")["n_removed"] == 67 * 35
    s = st("sized_99_100")
    assert (s["n_segments"], s["n_small"], s["n_removed"], s["largest"]) == (2, 1, 99, 100)
    assert st("ramp_300x1")["n_segments"] == 1 and st("ramp_80x20")["n_segments"] == 1
    assert st("one_pixel_valid")["n_removed"] == 1 and st("one_pixel_valid_kept")["n_removed"] == 0 and st("one_pixel_invalid")["n_valid"] == 0
    assert st("special_values_size0")["n_removed"] == 0 and st("special_values_size1")["n_removed"] == 0
    sp = R.remove_speckles(SC.by_name("special_values")["depth"], speckle_size=2)
    d0 = SC.by_name("special_values")["depth"]
    assert np.isinf(d0[2, 5]) and sp["labels"][2, 5] == 2 * 20 + 5 and sp["labels"][2, 6] == 2 * 20 + 6 and sp["depth"][2, 5] == 0   # infinite: valid, alone
    assert sp["labels"][4, 8] == -1 and np.isneginf(sp["depth"][4, 8]) and sp["labels"][1, 1] == -1 and np.isnan(sp["depth"][1, 1])
    assert sp["depth"].view(np.uint32)[1, 3] == 0x7FC12345 and sp["depth"].view(np.uint32)[6, 12] == 0x80000000
    # segments cross the tile borders of the device form in both directions
    for name in ("blobs_200x50", "blobs_130x70", "serpentine_517x259"):
        lab, _ = R.segments(SC.by_name(name)["depth"])
        ys, xs = np.nonzero(lab >= 0)
        ry, rx = np.divmod(lab[ys, xs], lab.shape[1])
        assert ((ry // SC.TILE_H != ys // SC.TILE_H) & (rx // SC.TILE_W != xs // SC.TILE_W)).any(), name


def test_asymmetric_pairs_are_not_joined():
    d = SC.by_name("asymmetric_band_66x18")["depth"]
    a, b = np.float32(2.0), np.float32(2.0) * (np.float32(1) + np.float32(0.00702))
    diff = np.abs(a - b)
    assert diff / b < R.THR <= diff / a                      # the pair passes seen from b and fails seen from a
    assert SL.lib().ss_joined(a, b, R.THR) == 0 and SL.lib().ss_joined(b, a, R.THR) == 0
    lab, _ = R.segments(d)
    # a segment holds one depth value only: a pair inside the band never joined two
    for root in np.unique(lab):
        assert len(np.unique(d[lab == root])) == 1


# ---- the effect on finished maps ---------------------------------------------------------------------------
# Final maps of the CPU oracle (device association): a splat of 80 sparse points, then three outer iterations of two sweeps each
# (adapthalfwin 6, seed 11), every iteration starting from the maps of the one before.  The statement with speckle_size 100 and the
# default threshold is applied to the final depth map.  "wrong": valid and more than 1 % off the ground truth.
# Produced by:  python tests/test_speckle_ref.py
#                          valid, wrong, removed wrong, removed good
EFFECT = {
    "low_contrast_96x80": (5408, 1714, 834, 27),
    "plain_160x120": (15476, 1457, 1225, 112),
}


def effect_scene(name):
    if name == "low_contrast_96x80":   # the scene of tests/test_gpu_prior.py: a region of the reference image at 5 % contrast
        views = [dict(v) for v in synth.make_views(96, 80, 90.0, 3, seed=12)]
        g = views[0]["gray"].copy(); reg = (slice(24, 56), slice(28, 72))
        g[reg] = g[reg].mean() + (g[reg] - g[reg].mean()) * 0.05
        views[0]["gray"] = g.astype(np.float32)
        return views
    return synth.make_views(160, 120, 150.0, 3, seed=3)


_FINAL = {}


def final_maps(name):
    """(views, depth, normal, conf) of the oracle's estimate; computed once per scene and left unchanged"""
    if name not in _FINAL:
        import oracle_lib as O
        import scene_oracle as SO
        views = effect_scene(name)
        pts = synth.sparse_points(views, 80, seed=5)
        d, n, dmin, dmax = SO.splat(views[0], pts)
        c = None
        for it in range(3):
            p = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, it_external=it, n_external_iters=3, adapthalfwin=6,
                                 n_estimation_iters=2, seed=11)
            d, n, c, _ = O.estimate(views, p, dmin, dmax, d, n, conf=c)
        _FINAL[name] = (views, d, n, c)
    return _FINAL[name]


def effect_counts(name):
    views, d, n, c = final_maps(name)
    gt = views[0]["depth"]
    valid = d > 0
    wrong = valid & ~(np.abs(d - gt) < 0.01 * gt)
    out = R.remove_speckles(d, n, c, speckle_size=100)
    gone = valid & (out["depth"] == 0)
    return int(valid.sum()), int(wrong.sum()), int((gone & wrong).sum()), int((gone & ~wrong).sum())


@pytest.mark.parametrize("name", sorted(EFFECT))
def test_effect_on_finished_maps(name):
    got = effect_counts(name)
    print("%s: valid %d, wrong %d, removed wrong %d, removed good %d" % ((name,) + got))
    assert got == EFFECT[name]
    views, d, n, c = final_maps(name)
    host = SL.host(d, n, c, None, 100)
    _same(host, R.remove_speckles(d, n, c, speckle_size=100), name)


if __name__ == "__main__":
    for name in sorted(EFFECT):
        print('    "%s": %r,' % (name, effect_counts(name)))

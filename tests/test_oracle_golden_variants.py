"""The oracle's estimate with a keep-mask (hcor_params.keep) and with view spread (hcor_params.spread_maps) against committed fixtures,
bit for bit and with equal counts.  tests/golden/estimate_variants_*.npz were recorded from the separate masked and view-spread oracle
sources that existed before both were folded into oracle/hcmvs_oracle.c (tests/golden/make_golden_mask_spread.py): they hold the one
process_pixel, the two sweep drivers, the score loop and the end pass to what those copies computed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_mask_spread as G  # noqa: E402


@pytest.mark.parametrize("name", list(G.CASES))
def test_masked_and_spread_estimates_match_the_committed_fixtures(name):
    want = np.load(G.path(name))
    got = G.run(name)
    for k in ("depth", "normal", "conf"):
        assert np.array_equal(got[k], want[k]), k
    assert int(got["evals"]) == int(want["evals"])
    assert tuple(int(x) for x in got["spread"]) == tuple(int(x) for x in want["spread"])
    ign = G.keep_mask() == 0
    assert ign.any() and (got["conf"][ign] == 0).all() and (got["normal"][ign] == 0).all()
    if G.CASES[name][1]:
        assert got["spread"][0] > 0 and got["spread"][1] > 0

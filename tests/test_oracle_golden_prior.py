"""The oracle's estimate with a depth prior (hcor_params.prior_map) and its sweeps-only entry (hcor_estimate_sweeps) against committed
fixtures, bit for bit and with equal counts.  tests/golden/estimate_prior_*.npz were recorded from the separate prior oracle source
(single-threaded, raster order) that existed before it was folded into oracle/hcmvs_oracle.c (tests/golden/make_golden_prior.py).  Every
case runs in both sweep orders, the device-association ones also with 1, 3 and 8 threads of the row wavefront: the prior path is
invariant under the visiting order and the thread count, which the separate source could not show."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_prior as G  # noqa: E402

ROWS = [dict(order=O.ORDER_ROWS, n_threads=t) for t in (1, 3, 8)]
ZIGZAG = dict(order=O.ORDER_ZIGZAG, n_threads=1)
RUNS = [(name, kw) for name, case in G.CASES.items() for kw in ([ZIGZAG] + ROWS if case[0] == "device" else [ZIGZAG, ROWS[0]])]

_INPUTS = {}


def inputs(arith):
    """built once per arithmetic and left unchanged (O.estimate copies the maps)"""
    if arith not in _INPUTS:
        _INPUTS[arith] = G.inputs(arith)
    return _INPUTS[arith]


@pytest.mark.parametrize("name,kw", RUNS, ids=["%s-%s%d" % (n, "rows" if kw["order"] == O.ORDER_ROWS else "zigzag", kw["n_threads"]) for n, kw in RUNS])
def test_prior_estimates_match_the_committed_fixtures(name, kw):
    want = np.load(G.path(name))
    got = G.run(name, inputs(G.CASES[name][0]), **kw)
    for k in ("depth", "normal", "conf"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("evals", "evals_prior", "pixels_prior"):
        assert int(got[k]) == int(want[k]), k
    assert int(got["evals_prior"]) > 0

"""Generates tests/golden/estimate_prior_*.npz: the oracle's estimate with a depth prior (--n-para_prior, --sigma-prior, --n-photo2geo) and
its sweeps-only entry on the small synthetic scene of make_golden_mask_spread.py, held by tests/test_oracle_golden_prior.py.  The
committed files were written by the separate prior oracle source (single-threaded, raster order) this repository had before it was
folded into oracle/hcmvs_oracle.c; they pin the merged code path -- both sweep orders, any thread count -- to those bits.  Regenerate
only when the oracle's arithmetic changes on purpose.
Run from the repo root: python tests/golden/make_golden_prior.py

The files hold results only (depth, normal, conf, evals, evals_prior, pixels_prior); inputs() rebuilds the inputs from seeds, for the
generator and for the test alike.  A sweeps-only case starts from the recorded result of the case it continues."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
import make_golden_mask_spread as MS  # noqa: E402
import oracle_lib as O  # noqa: E402
import prior_cases as PC  # noqa: E402

W, H, SEED, EST, ARITH = MS.W, MS.H, MS.SEED, MS.EST, MS.ARITH
PRIOR_SEED = 5
AUTHORS = dict(para_prior=0.4, sigma_prior=0.2, photo2geo=1)     # --n-para_prior 0.4 --n-photo2geo 1
DEFAULTS = dict(para_prior=0.5, sigma_prior=0.2, photo2geo=2)    # the reference's
# name: (arithmetic, it_external, n_external_iters, prior options, sweeps-only (first, n) or None, the case it continues or None)
CASES = {
    "reference": ("reference", 1, 3, AUTHORS, None, None),
    "device": ("device", 1, 3, AUTHORS, None, None),
    "device_last": ("device", 2, 3, DEFAULTS, None, None),                   # ends with the end pass
    "device_sweeps": ("device", 1, 3, AUTHORS, (2, 2), "device"),
    "device_sweeps_last": ("device", 1, 2, AUTHORS, (2, 2), "device"),       # sweeps-only, ends with the end pass
}


def path(name):
    return os.path.join(HERE, "estimate_prior_%s.npz" % name)


def inputs(arith):
    """make_golden_mask_spread.inputs (views, the maps after outer iteration 0 of the plain estimate, the keep-mask) and the prior"""
    inp = MS.inputs(arith)
    inp["prior"] = PC.make_prior(inp["views"][0], PRIOR_SEED)
    return inp


def run(name, inp=None, start=None, **over):
    """the estimate of case `name`: dict(depth, normal, conf, evals, evals_prior, pixels_prior).  start: (depth, normal, conf) of a
    sweeps-only case (default: the recorded result of the case it continues); over: overrides of order / n_threads"""
    arith, it, n_ext, pk, sweeps, frm = CASES[name]
    inp = inp or inputs(arith)
    kw = dict(ARITH[arith]); kw.update(over)
    p = O.default_params(it_external=it, n_external_iters=n_ext, seed=SEED, **EST, **kw)
    d, n, c = inp["depth"], inp["normal"], inp["conf"]
    if sweeps is not None:
        if start is None:
            with np.load(path(frm)) as z:
                start = (z["depth"], z["normal"], z["conf"])
        d, n, c = start
    st = {}
    d, n, c, ev = O.estimate(inp["views"], p, inp["dmin"], inp["dmax"], d, n, keep=inp["keep"], conf=c, prior=inp["prior"], prior_params=pk,
                             sweeps=sweeps, stats=st)
    assert ev == st["evals"]
    return dict(depth=d, normal=n, conf=c, evals=np.uint64(ev), evals_prior=np.uint64(st["evals_prior"]), pixels_prior=np.uint64(st["pixels_prior"]))


if __name__ == "__main__":
    done = {}
    for name, (arith, it, n_ext, pk, sweeps, frm) in CASES.items():
        inp = inputs(arith)
        r = run(name, inp, start=None if frm is None else tuple(done[frm][k] for k in ("depth", "normal", "conf")))
        done[name] = r
        ign = inp["keep"] == 0
        est = PC.estimated_pixels((H, W), 7, inp["keep"])
        inner = PC.estimated_pixels((H, W), 7)
        assert (ign & inner).any(), "the mask ignores nothing"
        share = float((PC.usable(inp["prior"]) & est).sum()) / float(est.sum())
        assert r["evals_prior"] > 0 and 0.5 < share < 0.9, "the term was not at work"
        assert int(r["pixels_prior"]) == int((PC.usable(inp["prior"]) & est).sum())
        np.savez_compressed(path(name), **r)
        assert os.path.getsize(path(name)) <= 126461
        print("%-20s evals %d evals_prior %d pixels_prior %d share %.3f valid %.3f ignored %d bytes %d" % (
            name, r["evals"], r["evals_prior"], r["pixels_prior"], share, float((r["depth"] > 0).mean()), int(ign.sum()), os.path.getsize(path(name))))

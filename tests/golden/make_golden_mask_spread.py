"""Generates tests/golden/estimate_variants_*.npz: the oracle's estimate with a keep-mask (--ignore-mask-label) and with view spread
(--n-viewspread) on one small synthetic scene, held by tests/test_oracle_golden_variants.py.  The committed files were written by the
separate masked and view-spread oracle sources this repository had before they were folded into oracle/hcmvs_oracle.c; they pin the
merged code paths to those bits.  Regenerate only when the oracle's arithmetic changes on purpose.
Run from the repo root: python tests/golden/make_golden_mask_spread.py

The files hold results only (depth, normal, conf, evals, the four spread counters); inputs() rebuilds the inputs from seeds, for the
generator and for the test alike."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402
import scene_oracle as SO  # noqa: E402

synth = importlib.import_module("hc-mvs_amd.synth")

W, H, F, SCENE_SEED, SEED = 72, 56, 80.0, 11, 777
EST = dict(adapthalfwin=5, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4)
ARITH = {"reference": dict(arith_mode=O.ARITH_REFERENCE, order=O.ORDER_ZIGZAG, n_threads=1),
         "device": dict(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=4)}
# name: (arithmetic, view spread, it_external, n_external_iters); the last one runs the masked end pass
CASES = {
    "mask_reference": ("reference", False, 1, 3),
    "mask_device": ("device", False, 1, 3),
    "mask_spread_reference": ("reference", True, 1, 3),
    "mask_spread_device": ("device", True, 1, 3),
    "mask_device_last": ("device", False, 1, 2),
}


def path(name):
    return os.path.join(HERE, "estimate_variants_%s.npz" % name)


def keep_mask():
    """blobs plus a one-pixel line"""
    rng = np.random.default_rng(9)
    keep = np.ones((H, W), np.uint8)
    yy, xx = np.mgrid[:H, :W]
    for _ in range(5):
        cy, cx, r = rng.integers(8, H - 8), rng.integers(8, W - 8), rng.integers(3, 8)
        keep[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 0
    keep[:, W // 3] = 0
    return keep


def inputs(arith):
    """views, the reference view's maps after outer iteration 0, the spread maps (each source view's own estimate at outer iteration 0 of
    2: raw scores, no end pass), the keep-mask -- all by the plain estimate, which tests/golden/estimate_96x80_v3*.npz pin"""
    views = synth.make_views(W, H, F, 2, seed=SCENE_SEED)

    def first(i, n_ext):
        vs = [views[i]] + [v for k, v in enumerate(views) if k != i]
        d0, n0, dmin, dmax = SO.splat(views[i], synth.sparse_points(vs, 50, seed=20 + i))
        p = O.default_params(it_external=0, n_external_iters=n_ext, seed=SEED + i, **EST, **ARITH[arith])
        return O.estimate(vs, p, dmin, dmax, d0, n0)[:3] + (dmin, dmax)

    d, n, c, dmin, dmax = first(0, 3)
    maps = [first(i, 2)[:3] for i in (1, 2)]
    return dict(views=views, depth=d, normal=n, conf=c, dmin=dmin, dmax=dmax, maps=maps, keep=keep_mask())


def run(name, inp=None):
    """the estimate of case `name`: dict(depth, normal, conf, evals, spread)"""
    arith, spread, it, n_ext = CASES[name]
    inp = inp or inputs(arith)
    p = O.default_params(it_external=it, n_external_iters=n_ext, seed=SEED, **EST, **ARITH[arith])
    O.stats(reset=True)
    d, n, c, ev = O.estimate(inp["views"], p, inp["dmin"], inp["dmax"], inp["depth"], inp["normal"], keep=inp["keep"],
                             maps=inp["maps"] if spread else None, on=spread, conf=inp["conf"])
    return dict(depth=d, normal=n, conf=c, evals=np.uint64(ev), spread=np.array(O.stats(), np.uint64))


if __name__ == "__main__":
    for name, (arith, spread, it, n_ext) in CASES.items():
        inp = inputs(arith)
        r = run(name, inp)
        ign = inp["keep"] == 0
        inner = np.zeros((H, W), bool); inner[7:H - 7, 7:W - 7] = True
        assert (ign & inner).any() and (r["conf"][ign] == 0).all(), "the mask ignores nothing"
        if spread:  # not vacuous: slots were scored and accepted
            assert r["spread"][0] > 0 and r["spread"][1] > 0, r["spread"]
        else:
            assert not r["spread"].any()
        np.savez_compressed(path(name), **r)
        assert os.path.getsize(path(name)) <= 126461
        print("%-24s evals %d spread %s valid %.3f ignored %d bytes %d" % (name, r["evals"], tuple(int(x) for x in r["spread"]),
              float((r["depth"] > 0).mean()), int(ign.sum()), os.path.getsize(path(name))))

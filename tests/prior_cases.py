"""Inputs the prior tests share (CPU and GPU): prior maps over synth scenes and the maps an outer iteration >= 1 starts from."""
import importlib

import numpy as np

import oracle_lib as O
import scene_oracle as SO

synth = importlib.import_module("hc-mvs_amd.synth")

KW = dict(propagate_halfwin=5, propagate_step=4)


def make_prior(view, seed=0, zeros=0.3, odd=True):
    """the analytic depth of the view times 1 + u, u uniform in +-3 %; about 30 % of the pixels set to 0; a sprinkle (about 1 % each) of
    negative, NaN and infinite values for the validity rule"""
    rng = np.random.default_rng(1000 + seed)
    d = view["depth"].astype(np.float32)
    p = (d * (1.0 + rng.uniform(-0.03, 0.03, d.shape))).astype(np.float32)
    p[rng.uniform(size=d.shape) < zeros] = 0
    if odd:
        r = rng.uniform(size=d.shape)
        p[r < 0.01] = -p[r < 0.01] - 1.0
        p[(r >= 0.01) & (r < 0.02)] = np.nan
        p[(r >= 0.02) & (r < 0.025)] = np.inf
        p[(r >= 0.025) & (r < 0.03)] = -np.inf
    return p


def usable(prior):
    """the validity rule: finite and > 0"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(prior) & (prior > 0)


def start_maps(views, seed=0, **kw):
    """depth, normal, conf (the score), dmin, dmax as outer iteration 0 of the plain estimate leaves them, on the CPU"""
    pts = synth.sparse_points(views, 80, seed=5 + seed)
    d0, n0, dmin, dmax = SO.splat(views[0], pts)
    p0 = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, it_external=0, n_external_iters=3, adapthalfwin=5, n_estimation_iters=1)
    for k, v in kw.items():
        setattr(p0, k, v)
    d, n, c, _ = O.estimate(views, p0, dmin, dmax, d0, n0)
    return d, n, c, dmin, dmax


def estimated_pixels(shape, border, keep=None):
    h, w = shape
    m = np.zeros(shape, bool)
    m[border:h - border, border:w - border] = True
    return m if keep is None else m & (np.asarray(keep) != 0)


def estimate(views, params, d_min, d_max, depth, normal, conf=None, prior=None, keep=None, gra=None, sweeps=None, **prior_params):
    """oracle_lib.estimate with a prior (prior_params: para_prior, sigma_prior, photo2geo) and with its counters:
    depth, normal, conf, dict(evals, evals_prior, pixels_prior)"""
    st = {}
    d, n, c, _ = O.estimate(views, params, d_min, d_max, depth, normal, gra=gra, keep=keep, conf=conf, prior=prior, prior_params=prior_params,
                            sweeps=sweeps, stats=st)
    return d, n, c, st

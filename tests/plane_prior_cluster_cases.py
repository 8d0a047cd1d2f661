"""Inputs of the plane-prior clustering tests, built with the helpers of tests/plane_prior_cases.py: one plane
whose usable samples fall into several islands, so that a plane's inliers are not connected.  All are 96 x 80 with K = _K(96, 80, 90).  A case
is the dict plane_prior_cases makes, plus `gap` for the doorway: the (h, w) bool mask of the strip of the region that has no usable sample."""
import numpy as np

import plane_prior_cases as PC

W, H = 96, 80
NOISE = dict(depth_noise=0.002, outliers=0.02, normal_noise=0.05, bad_conf=0.1)


def _tilted(seed):
    """the plane n = (0.2, -0.3, 1) normalised through (0, 0, 5) over the region [8:72, 6:90], with the noise of the blobs case"""
    rng = np.random.RandomState(seed)
    K = PC._K(W, H, 90.0)
    ray = PC._rays(K, W, H)
    n = np.array([0.2, -0.3, 1.0]); n /= np.linalg.norm(n)
    d = n[2] * 5.0
    truth = PC._plane_depth(ray, n, d)
    region = np.zeros((H, W), bool); region[8:72, 6:90] = True
    return PC._case(rng, K, truth, PC._facing(n, ray), region, [(n, d, region.copy())], **NOISE)


def doorway():
    """(a) two walls either side of a doorway: no usable sample in a strip 20 px wide"""
    c = _tilted(500)
    c["conf"][:, 38:58] = 0.4
    gap = np.zeros((H, W), bool); gap[:, 38:58] = True
    c["gap"] = gap & c["region"]
    return c


def islet():
    """(b) a large part and an 8 x 8 islet far from it"""
    c = _tilted(600)
    keep = np.zeros((H, W), bool); keep[8:72, 6:56] = True; keep[30:38, 78:86] = True
    c["conf"][~keep] = 0.4
    return c


def islands():
    """(c) nine 8 x 8 squares, none of which holds min_points samples at the default share"""
    c = _tilted(800)
    keep = np.zeros((H, W), bool)
    for r in (12, 36, 60):
        for col in (16, 44, 72):
            keep[r:r + 8, col:col + 8] = True
    c["conf"][~keep] = 0.4
    return c


def mirror():
    """(d) noise-free and fronto-parallel, two blobs of the same size: a tie between two components"""
    K = PC._K(W, H, 90.0)
    region = np.zeros((H, W), bool); region[20:60, 8:36] = True; region[20:60, 60:88] = True
    n = np.array([0.0, 0.0, 1.0])
    depth = np.where(region, 5.0, 0.0).astype(np.float32)
    normal = np.zeros((H, W, 3), np.float32); normal[..., 2] = -1.0
    conf = np.full((H, W), 0.05, np.float32)
    return dict(depth=depth, normal=normal, conf=conf, region=region, K=K, truth=np.where(region, 5.0, np.inf), planes=[(n, 5.0, region.copy())])


CASES = dict(doorway=doorway, islet=islet, islands=islands, mirror=mirror)

"""Inputs of the plane-prior tests, built analytically (ground truth plus noise, no estimate needed).  Every case is a dict: depth (h, w) f32,
normal (h, w, 3) f32, conf (h, w) f32 (the score: lower is better), region (h, w) bool, K (3, 3), truth (h, w) f64 noise-free depth, and
planes: the generating planes as (unit normal, offset d of n . X = d, (h, w) bool mask of the region pixels they generate)."""
import importlib

import numpy as np

synth = importlib.import_module("hc-mvs_amd.synth")


def _K(w, h, focal):
    return np.array([[focal, 0, (w - 1) / 2.0], [0, focal, (h - 1) / 2.0], [0, 0, 1]], np.float64)


def _rays(K, w, h):
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], -1)


def _plane_depth(ray, n, d):
    den = ray @ n
    with np.errstate(divide="ignore", invalid="ignore"):
        t = d / den
    return np.where((np.abs(den) > 1e-9) & (t > 0), t, np.inf)


def _facing(n, ray):
    n = np.broadcast_to(n, ray.shape)
    return np.where(((n * ray).sum(-1) > 0)[..., None], -n, n)


def _noisy(rng, truth, nrm, region, depth_noise, outliers, normal_noise, bad_conf):
    """depth * (1 + depth_noise * N(0, 1)); a share `outliers` of the pixels gets a depth off by -50 .. +50 %; the normals are disturbed by
    normal_noise * N(0, 1) per component and normalised; a share `bad_conf` of the pixels has a score above conf_max"""
    h, w = truth.shape
    depth = truth * (1.0 + depth_noise * rng.normal(size=(h, w)))
    gross = rng.uniform(size=(h, w)) < outliers
    depth = np.where(gross, truth * rng.uniform(0.5, 1.5, size=(h, w)), depth)
    n = nrm + normal_noise * rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    conf = np.where(rng.uniform(size=(h, w)) < bad_conf, 0.4, 0.05) + 0.02 * rng.uniform(size=(h, w))
    depth = np.where(np.isfinite(depth), depth, 0.0)
    return depth.astype(np.float32), n.astype(np.float32), conf.astype(np.float32)


def _case(rng, K, truth, nrm, region, planes, **noise):
    depth, normal, conf = _noisy(rng, np.where(np.isfinite(truth), truth, 0.0), nrm, region, **noise)
    return dict(depth=depth, normal=normal, conf=conf, region=region, K=K, truth=truth, planes=planes)


def crease(seed=0, w=96, h=80):
    """(a) two planes meeting in a vertical crease at the image centre: 0.3 % depth noise, 5 % gross outliers, noisy normals"""
    rng = np.random.RandomState(100 + seed)
    K = _K(w, h, 90.0)
    ray = _rays(K, w, h)
    n1 = np.array([0.45, 0.05, 1.0]); n1 /= np.linalg.norm(n1)
    n2 = np.array([-0.5, -0.08, 1.0]); n2 /= np.linalg.norm(n2)
    d1, d2 = n1[2] * 6.0, n2[2] * 6.0   # both through (0, 0, 6)
    t1, t2 = _plane_depth(ray, n1, d1), _plane_depth(ray, n2, d2)
    truth = np.minimum(t1, t2)           # a ridge towards the camera: the nearer plane is the visible one
    left = t1 <= t2                      # the pixels of the first plane
    region = np.zeros((h, w), bool); region[5:h - 5, 6:w - 6] = True
    nrm = np.where(left[..., None], _facing(n1, ray), _facing(n2, ray))
    return _case(rng, K, truth, nrm, region, [(n1, d1, region & left), (n2, d2, region & ~left)], depth_noise=0.003, outliers=0.05, normal_noise=0.08, bad_conf=0.1)


def plane_and_sphere(seed=0, w=160, h=120):
    """(b) synth.Scene's tilted plane with the sphere in front of it; the region covers both.  Only the plane is a generating plane"""
    rng = np.random.RandomState(200 + seed)
    K = _K(w, h, 150.0)
    sc = synth.Scene(2)
    _, depth, normal = sc.render(K, np.eye(3), np.zeros(3), w, h, quantise=False)
    ray = _rays(K, w, h)
    tp = _plane_depth(ray, sc.plane_n, sc.plane_d)
    on_plane = np.abs(depth.astype(np.float64) - tp) < 1e-4 * tp
    truth = np.where(on_plane, tp, depth.astype(np.float64))
    region = np.zeros((h, w), bool); region[8:h - 8, 10:w - 10] = True
    return _case(rng, K, truth, normal.astype(np.float64), region, [(sc.plane_n, sc.plane_d, region & on_plane)], depth_noise=0.001, outliers=0.01, normal_noise=0.03,
                 bad_conf=0.3)


def grazing(seed=0, w=96, h=80):
    """(c) one plane seen at a grazing angle: the rectangle around its inliers, taken in the plane's frame, has a corner behind the camera"""
    rng = np.random.RandomState(300 + seed)
    K = _K(w, h, 30.0)
    ray = _rays(K, w, h)
    n = np.array([0.3, -1.0, 0.5])       # a floor falling away from the camera; |n_x| is its smallest component, so both frame axes have a z part
    d = -0.5 / np.linalg.norm(n); n /= np.linalg.norm(n)
    t = _plane_depth(ray, n, d)
    region = np.isfinite(t) & (t < 30.0)
    region[:3] = False; region[-3:] = False; region[:, :3] = False; region[:, -3:] = False
    truth = np.where(region, t, np.inf)
    return _case(rng, K, truth, _facing(n, ray), region, [(n, d, region.copy())], depth_noise=0.001, outliers=0.01, normal_noise=0.03, bad_conf=0.05)


def two_blobs(seed=0, w=96, h=80):
    """(d) a region of two disjoint blobs on the same plane"""
    rng = np.random.RandomState(400 + seed)
    K = _K(w, h, 90.0)
    ray = _rays(K, w, h)
    n = np.array([0.2, -0.3, 1.0]); n /= np.linalg.norm(n)
    d = n[2] * 5.0
    truth = _plane_depth(ray, n, d)
    region = np.zeros((h, w), bool); region[8:40, 6:38] = True; region[44:74, 56:90] = True
    return _case(rng, K, truth, _facing(n, ray), region, [(n, d, region.copy())], depth_noise=0.002, outliers=0.02, normal_noise=0.05, bad_conf=0.1)


CASES = dict(crease=crease, plane_and_sphere=plane_and_sphere, grazing=grazing, two_blobs=two_blobs)

# The inputs of the clustering tests (S4c): one plane whose usable samples fall into several islands, so that a plane's inliers are not
# connected.  All are 96 x 80 with K = _K(96, 80, 90); the doorway has `gap` on top, the (h, w) bool mask of the strip of the region that has
# no usable sample.
W, H = 96, 80


def _tilted(seed):
    """the plane n = (0.2, -0.3, 1) normalised through (0, 0, 5) over the region [8:72, 6:90], with the noise of the blobs case"""
    rng = np.random.RandomState(seed)
    K = _K(W, H, 90.0)
    ray = _rays(K, W, H)
    n = np.array([0.2, -0.3, 1.0]); n /= np.linalg.norm(n)
    d = n[2] * 5.0
    truth = _plane_depth(ray, n, d)
    region = np.zeros((H, W), bool); region[8:72, 6:90] = True
    return _case(rng, K, truth, _facing(n, ray), region, [(n, d, region.copy())], depth_noise=0.002, outliers=0.02, normal_noise=0.05, bad_conf=0.1)


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
    K = _K(W, H, 90.0)
    region = np.zeros((H, W), bool); region[20:60, 8:36] = True; region[20:60, 60:88] = True
    n = np.array([0.0, 0.0, 1.0])
    depth = np.where(region, 5.0, 0.0).astype(np.float32)
    normal = np.zeros((H, W, 3), np.float32); normal[..., 2] = -1.0
    conf = np.full((H, W), 0.05, np.float32)
    return dict(depth=depth, normal=normal, conf=conf, region=region, K=K, truth=np.where(region, 5.0, np.inf), planes=[(n, 5.0, region.copy())])


CLUSTER_CASES = dict(doorway=doorway, islet=islet, islands=islands, mirror=mirror)


def evaluate(case, result):
    """per generating plane the best-matching found plane's angle (degrees) and relative offset error, and the share of the generating planes'
    region pixels whose prior is within 1 % of the truth.  Returns (list of (angle, offset) or None when no plane matches, share)"""
    errs = []
    for n, d, mask in case["planes"]:
        best = None
        for t in result["planes"]:
            m = t["normal"].astype(np.float64)
            ang = float(np.degrees(np.arccos(min(1.0, abs(float(m @ n))))))
            nc = float(t["nc"]) if "nc" in t else float(m @ t["centre"])
            off = abs(abs(nc) - abs(d)) / abs(d)
            if best is None or (ang, off) < best:
                best = (ang, off)
        errs.append(best)
    mask = np.zeros_like(case["region"])
    for _, _, m in case["planes"]:
        mask |= m
    truth = case["truth"][mask]
    pr = result["prior"][mask].astype(np.float64)
    share = float((np.abs(pr - truth) <= 0.01 * truth).mean())
    return errs, share

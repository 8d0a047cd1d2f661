"""numpy restatement of Scene::PointCloudFilter (SceneDensify.cpp:4188-4320; DensifyPointCloud --filter-point-cloud < 0), the
spec hcmvs_point_cloud_filter is checked against: brute force over all points for every (point, view) pair, float32 with the
association DESIGN.md section 5 states, and the reference's swap-with-last removal order.  Test infrastructure, no GPU."""
import math

import numpy as np

F = np.float32


def cone(cam):
    """apex float(C) and cos^2 of the half-angle float(ComputeFOV(0) / width) (Image.cpp:215-226); None when uncalibrated"""
    if cam is None or cam.get("K") is None or not cam.get("width"):
        return None
    w = int(cam["width"])
    angle = F(2.0 * math.atan(w / (float(np.asarray(cam["K"])[0, 0]) * 2.0)) / w)
    c = F(math.cos(float(angle)))
    return np.asarray(cam["C"], np.float64).astype(F), F(c * c)


def pairs_by_view(n_views, view_ids, n_images):
    """point indices of every image's pairs, and the number of view entries that name no image"""
    nv = np.asarray(n_views, np.int64)
    pt = np.repeat(np.arange(len(nv)), nv)
    vi = np.asarray(view_ids, np.int64)
    out = [pt[vi == j] for j in range(n_images)]
    return out, int((vi >= n_images).sum())


def visibility(xyz, n_views, view_ids, cameras, targets=None, chunk=1 << 22):
    """int64 visibility of every point (or of the points `targets` only): for every pair (X, j) every point P in j's cone around the ray
    to X that passes TConeIntersect::Classify (Ray.inl:986-1002) and is not depth-similar (Util.inl:658-669) votes +|views(P)| when
    behind X, -|views(X)| in front"""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    nv = np.asarray(n_views, np.int64)
    cols = np.arange(len(xyz)) if targets is None else np.asarray(targets, np.int64)
    P = xyz[cols]
    vis = np.zeros(len(cols), np.int64)
    per_view, _ = pairs_by_view(n_views, view_ids, len(cameras))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j, cam in enumerate(cameras):
            cn = cone(cam)
            if cn is None or len(per_view[j]) == 0:
                continue
            Cf, cosSq = cn
            E = P - Cf
            e2 = (E[:, 0] * E[:, 0] + E[:, 1] * E[:, 1]) + E[:, 2] * E[:, 2]
            lim = cosSq * e2
            rows = max(1, chunk // max(len(cols), 1))
            for s in range(0, len(per_view[j]), rows):
                idx = per_view[j][s:s + rows]
                D = xyz[idx] - Cf
                dist = np.sqrt((D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2])
                d = D / dist[:, None]
                maxH = dist * F(1.02)
                t = (d[:, 0:1] * E[None, :, 0] + d[:, 1:2] * E[None, :, 1]) + d[:, 2:3] * E[None, :, 2]
                ok = ~(np.abs(t) < F(1e-4)) & ~(t < 0) & ~(t > maxH[:, None]) & (t * t > lim[None, :])
                ok &= ~(np.abs(dist[:, None] - t) / dist[:, None] < F(0.01))
                behind = t > dist[:, None]
                vis += (ok & behind).sum(0) * nv[cols]
                vis -= ((ok & ~behind) * nv[idx][:, None]).sum(0)
    return vis


def removal_order(vis, th_remove):
    """RFOREACH + PointCloud::RemovePoint (PointCloud.cpp:54-69): cList::RemoveAt moves the last element into the hole
    (List.h:1070-1077); returns the indices of the kept points in their output order"""
    order = np.arange(len(vis))
    size = len(vis)
    for i in np.nonzero(np.asarray(vis) <= th_remove)[0][::-1]:
        size -= 1
        order[i] = order[size]
    return order[:size]


def filter_cloud(xyz, n_views, view_ids, cameras, th_remove=-1):
    vis = visibility(xyz, n_views, view_ids, cameras)
    return vis, removal_order(vis, th_remove)

"""A context gives back the device memory it took: a whole lifetime (upload, estimate, maps, fusion, a post-filter chain, colours,
normals, the visibility filter, destroy) leaves the device's free memory where it was before the context was created."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")

W, H, N = 640, 480, 4  # the post-filter chain's state alone is ~360 B per pixel: some 400 MB for the four images


def scene():
    views = synth.make_views(W, H, 600.0, N - 1, seed=31, baseline=(0.04, 0.09))
    for v in views:
        v["bgr"] = np.stack([np.clip(np.rint(v["gray"] * 255), 0, 255).astype(np.uint8)] * 3, -1).copy()
    pts = [synth.sparse_points([v], 300, seed=40 + i) for i, v in enumerate(views)]
    return views, pts


def lifetime(views, pts, free):
    """one context from create to destroy; returns the least free memory seen while it lived"""
    seen = [free()]
    ctx = binding.Context(0)
    try:
        ids = list(range(N))
        for i, v in enumerate(views):
            ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"], bgr=v["bgr"])
        p = binding.default_params(n_estimation_iters=2)
        for i in ids:
            d0, n0, dmin, dmax = ctx.splat_init(i, pts[i])
            d, n, c = ctx.estimate(i, [j for j in ids if j != i], p, dmin, dmax, d0, n0)
            ctx.set_depthmap(i, d, n, c, dmin, dmax)
            ctx.set_neighbors(i, [j for j in ids if j != i])
        seen.append(free())
        cap = N * W * H
        cloud = ctx.fuse_cloud(ids, cap, 4 * cap)
        assert cloud["n_points"] > 1000
        seen.append(free())
        ctx.postfilter_sequence(ids, ids)
        seen.append(free())
        xyz, nv, vids = cloud["xyz"], cloud["n_views"], cloud["view_ids"]
        ctx.estimate_point_colors(xyz, nv, vids)
        ctx.estimate_point_normals(xyz, nv, vids)
        ctx.point_cloud_filter(xyz, nv, vids, [dict(K=v["K"], R=v["R"], C=v["C"], width=W, height=H) for v in views])
        seen.append(free())
    finally:
        ctx.close()
    return min(seen)


def test_context_gives_back_its_memory():
    """The first lifetime is not measured: it loads the kernels and grows what the runtime keeps for the process (kernel scratch,
    queues).  Each of the two lifetimes after it must end within 5 % of its peak use of where it began."""
    import torch
    free = lambda: torch.cuda.mem_get_info(0)[0]  # noqa: E731
    views, pts = scene()
    lifetime(views, pts, free)
    for _ in range(2):
        before = free()
        peak = before - lifetime(views, pts, free)
        lost = before - free()
        assert peak > 200 << 20, "the scene used %.1f MB: too little to tell a leak from allocator granularity" % (peak / 2**20)
        assert lost < 0.05 * peak, "%.1f MB of the %.1f MB used were not given back" % (lost / 2**20, peak / 2**20)

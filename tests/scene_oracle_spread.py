"""Scene-level oracle harness with view spread (test infrastructure only): tests/scene_oracle.py::densify with --n-viewspread, i.e. what
hc-mvs_amd/distributed.py::densify_scene(viewspread=True) computes, played on the CPU with tests/oracle_spread.c.

Two schedules:

  interleave=False  batch: every estimate of outer iteration i >= 1 reads the maps of its source views as outer iteration i - 1 left
                    them, post-filters included (a snapshot taken before the iteration: Jacobi order)
  interleave=True   the reference's order: in EVERY outer iteration >= 1 the images are estimated one after the other (ids ascending,
                    each followed by its post-filter in the filtered iterations) and read the live maps -- images < k as this iteration
                    left them (after the end pass in the last one), images > k from the previous one
"""
import numpy as np

import oracle_lib as O
import oracle_spread_lib as S
import scene_oracle as SO


def densify(views, srcs, neighbors, order, init, n_external_iters=1, postfilter=False, interleave=False, viewspread=True, mode=O.ARITH_DEVICE,
            seed=1234, n_threads=8, fuse=True, pf_kw=None, fuse_kw=None, **est_kw):
    """Arguments and result as scene_oracle.densify (no hints); the result also holds spread=(scored, accepted, dropped, outside)."""
    ids = sorted(views)
    assert ids == list(range(len(ids)))
    gra = {i: SO.gradient_map(views[i]) for i in ids}
    cur = {}
    for i in ids:
        d0, n0, dmin, dmax = init[i]
        cur[i] = dict(K=views[i]["K"], R=views[i]["R"], C=views[i]["C"], depth=np.ascontiguousarray(d0, np.float32).copy(),
                      normal=np.ascontiguousarray(n0, np.float32).copy(), conf=np.zeros(d0.shape, np.float32), bgr=views[i].get("bgr"),
                      d_min=float(dmin), d_max=float(dmax), neighbors=[n for n in neighbors[i] if n in views][:31])
    filled, evals = [], 0
    S.stats(reset=True)

    def estimate(i, it, offered):
        nonlocal evals
        p = O.default_params(arith_mode=mode, order=O.ORDER_ROWS, n_threads=n_threads, it_external=it, n_external_iters=n_external_iters,
                             seed=(seed + i) & 0xFFFFFFFF, **est_kw)
        vs = [views[i]] + [views[s] for s in srcs[i]]
        maps = None
        if offered is not None:
            maps = [(offered[s]["depth"], offered[s]["normal"], offered[s]["conf"]) for s in srcs[i]]
        d, n, c, ev = S.estimate(vs, p, cur[i]["d_min"], cur[i]["d_max"], cur[i]["depth"], cur[i]["normal"], maps=maps, on=viewspread, gra=gra[i])
        cur[i]["depth"], cur[i]["normal"], cur[i]["conf"] = d, n, c
        evals += ev

    def post(i):
        dd, nd, cd, nf = O.postfilter([cur[k] for k in ids], i, gra[i], order, mode=mode, **(pf_kw or {}))
        for k in ids:
            cur[k]["depth"] = dd[k]
        cur[i]["normal"], cur[i]["conf"] = nd, cd
        filled.append(nf)

    for it in range(n_external_iters):
        filt = postfilter and it in (1, 2)
        spread = viewspread and it >= 1
        if (filt or spread) and interleave:
            for i in ids:
                estimate(i, it, cur if spread else None)  # the live maps (S.estimate works on copies of image i's own)
                if filt:
                    post(i)
        else:
            snap = None
            if spread:
                snap = {k: dict(depth=cur[k]["depth"].copy(), normal=cur[k]["normal"].copy(), conf=cur[k]["conf"].copy()) for k in ids}
            for i in ids:
                estimate(i, it, snap)
            if filt:
                for i in ids:
                    post(i)
    out = dict(maps={i: (cur[i]["depth"].copy(), cur[i]["normal"].copy(), cur[i]["conf"].copy()) for i in ids}, filled=filled, evals=evals,
               spread=S.stats())
    if fuse:
        h, w = cur[ids[0]]["depth"].shape
        out["cloud"] = O.fuse_depthmaps([cur[k] for k in ids], list(order), h * w * len(ids) // 2 + 16, **(fuse_kw or {}))
    return out

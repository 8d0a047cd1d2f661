"""TEST INFRASTRUCTURE: the prior schedule of distributed.densify_scene(priors=...) over a scene with the oracle variant
(tests/oracle_prior.c), as scene_oracle.py plays the plain one: per outer iteration every image's estimate; on outer iteration
n_external_iters - 2 an image with a prior then has it registered and runs the reference's two extra sweeps (indices n_estimation_iters
and n_estimation_iters + 1, SceneDensify.cpp:983-1031); on the last outer iteration the prior stays registered.  No post-filters, no view
spread, no hints.  With fewer than two outer iterations the priors are never used."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle_lib as O
import oracle_prior_lib as OP
import scene_oracle as SO


def densify(views, srcs, neighbors, order, init, priors, prior_params=None, n_external_iters=3, mode=O.ARITH_DEVICE, seed=1234, fuse=True, fuse_kw=None,
            **est_kw):
    """views, srcs, neighbors, order, init, est_kw as scene_oracle.densify takes them; priors: {id: (h, w) float32}; prior_params:
    dict(para_prior, sigma_prior, photo2geo), missing keys the reference's defaults.
    Returns dict(maps={id: (depth, normal, conf)}, cloud=..., evals, evals_prior)."""
    ids = sorted(views)
    assert ids == list(range(len(ids)))
    pk = dict(OP.PRIOR_DEFAULTS); pk.update(prior_params or {})
    gra = {i: SO.gradient_map(views[i]) for i in ids}
    cur = {}
    for i in ids:
        d0, n0, dmin, dmax = init[i]
        cur[i] = dict(K=views[i]["K"], R=views[i]["R"], C=views[i]["C"], depth=np.ascontiguousarray(d0, np.float32).copy(),
                      normal=np.ascontiguousarray(n0, np.float32).copy(), conf=np.zeros(d0.shape, np.float32), bgr=views[i].get("bgr"),
                      d_min=float(dmin), d_max=float(dmax), neighbors=[n for n in neighbors[i] if n in views][:31])
    registered = set()
    evals = evals_prior = 0
    n_sweeps = est_kw.get("n_estimation_iters", O.default_params().n_estimation_iters)

    def image(i, it):       # the images of an outer iteration do not read each other's maps (no view spread, no post-filter): one thread each
        ev = evp = 0
        p = O.default_params(arith_mode=mode, it_external=it, n_external_iters=n_external_iters, seed=(seed + i) & 0xFFFFFFFF, **est_kw)
        vs = [views[i]] + [views[s] for s in srcs[i]]
        runs = [None]
        if it == n_external_iters - 2 and i in priors:
            runs.append((n_sweeps, 2))
        for sweeps in runs:
            if sweeps is not None:
                registered.add(i)
            d, n, c, st = OP.estimate(vs, p, cur[i]["d_min"], cur[i]["d_max"], cur[i]["depth"], cur[i]["normal"], conf=cur[i]["conf"], gra=gra[i],
                                      prior=priors[i] if i in registered else None, sweeps=sweeps, **pk)
            cur[i]["depth"], cur[i]["normal"], cur[i]["conf"] = d, n, c
            ev += st["evals"]; evp += st["evals_prior"]
        return ev, evp

    with ThreadPoolExecutor(max_workers=min(len(ids), 8)) as pool:
        for it in range(n_external_iters):
            for ev, evp in pool.map(lambda i: image(i, it), ids):
                evals += ev; evals_prior += evp
    out = dict(maps={i: (cur[i]["depth"].copy(), cur[i]["normal"].copy(), cur[i]["conf"].copy()) for i in ids}, evals=evals, evals_prior=evals_prior)
    if fuse:
        h, w = cur[ids[0]]["depth"].shape
        out["cloud"] = O.fuse_depthmaps([cur[k] for k in ids], list(order), h * w * len(ids) // 2 + 16, **(fuse_kw or {}))
    return out

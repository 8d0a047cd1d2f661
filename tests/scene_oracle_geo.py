"""The scene-level oracle of distributed.densify_scene(geo=...): the batch schedule of tests/scene_oracle.py::densify with the
geometric-consistency term (tests/oracle_geo.c).  From outer iteration 1 on every estimate is offered its source views' maps as the previous
outer iteration left them; the term blends from outer iteration max(1, photo2geo) on.  No post-filter, no interleaving."""
import numpy as np

import oracle_geo_lib as G
import oracle_lib as O
import scene_oracle as SO


def densify(views, srcs, init, geo, n_external_iters=3, seed=1234, **est_kw):
    """views: {id: dict(gray, K, R, C)}; srcs: {id: [ids]}; init: {id: (depth0, normal0, d_min, d_max)}; geo: dict of the term's options
    (None: off); est_kw: oracle estimate parameters.  Returns dict(maps={id: (depth, normal, conf)}, evals, evals_geo, pixels_geo)."""
    ids = sorted(views)
    gra = {i: SO.gradient_map(views[i]) for i in ids}
    cur = {i: dict(depth=np.ascontiguousarray(init[i][0], np.float32).copy(), normal=np.ascontiguousarray(init[i][1], np.float32).copy(),
                   conf=np.zeros(init[i][0].shape, np.float32)) for i in ids}
    tot = dict(evals=0, evals_geo=0, pixels_geo=0)
    for it in range(n_external_iters):
        snap = None
        if geo is not None and it >= 1:
            snap = {k: (cur[k]["depth"].copy(), cur[k]["normal"].copy(), cur[k]["conf"].copy()) for k in ids}
        for i in ids:
            p = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, it_external=it, n_external_iters=n_external_iters,
                                 seed=(seed + i) & 0xFFFFFFFF, **est_kw)
            vs = [views[i]] + [views[s] for s in srcs[i]]
            maps = None if snap is None else [snap[s] for s in srcs[i]]
            d, n, c, st = G.estimate(vs, p, init[i][2], init[i][3], cur[i]["depth"], cur[i]["normal"], maps=maps, geo=dict(geo, on=1) if geo is not None else None,
                                     gra=gra[i])
            cur[i]["depth"], cur[i]["normal"], cur[i]["conf"] = d, n, c
            for k in tot:
                tot[k] += st[k]
    return dict(maps={i: (cur[i]["depth"], cur[i]["normal"], cur[i]["conf"]) for i in ids}, **tot)

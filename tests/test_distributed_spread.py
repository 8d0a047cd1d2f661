"""densify_scene(viewspread=True) with two ranks on the CPU (gloo), the oracle standing in for the device context: the per-iteration
all-gather that gives every rank the previous iteration's maps of its source views (batch schedule) and the live maps of the interleaved
schedule must give what one process gives, which is what the scene-level harness tests/scene_oracle.py gives with viewspread=True."""
import importlib
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O  # noqa: E402

D = importlib.import_module("hc-mvs_amd.distributed")

KW = dict(adapthalfwin=5, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4)


def _context():
    import scene_oracle as SO

    class SpreadOracleContext(SO.OracleContext):
        """OracleContext with the three view-spread entry points of binding.Context (the maps are host pointers here)"""

        def __init__(self):
            super().__init__()
            self.spread_on, self.spread = False, {}

        def set_viewspread(self, on):
            self.spread_on = bool(on)

        def set_spread_maps_device(self, vid, d, n, c):
            if d:
                self.spread[vid] = (d, n, c)
            else:
                self.spread.pop(vid, None)

        def estimate_batch_device(self, items, p):
            for it in items:
                i = it["ref_id"]
                h, w = self.views[i]["gray"].shape
                d = self._arr(it["d_depth"], h * w).reshape(h, w); n = self._arr(it["d_normal"], 3 * h * w).reshape(h, w, 3)
                c = self._arr(it["d_conf"], h * w).reshape(h, w)
                kw = {k: getattr(p, k) for k, _ in p._fields_ if k not in ("seed",)}
                po = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=4, seed=(p.seed + it.get("seed_offset", 0)) & 0xFFFFFFFF, **kw)
                vs = [self.views[i]] + [self.views[s] for s in it["src_ids"]]
                maps = []
                for s in it["src_ids"]:
                    if s not in self.spread:
                        maps.append(None)
                        continue
                    sh, sw = self.views[s]["gray"].shape
                    pd, pn, pc = self.spread[s]
                    assert pd != it["d_depth"], "an estimate must not read what it writes"
                    maps.append((self._arr(pd, sh * sw).reshape(sh, sw).copy(), self._arr(pn, 3 * sh * sw).reshape(sh, sw, 3).copy(),
                                 self._arr(pc, sh * sw).reshape(sh, sw).copy()))
                dd, nn, cc, _ = O.estimate(vs, po, it["d_min"], it["d_max"], d, n, maps=maps, on=self.spread_on, gra=self.gra[i])
                d[...] = dd; n[...] = nn; c[...] = cc

    return SpreadOracleContext()


def _scene_worker(rank, world, port, ret, interleave):
    import scene_oracle as SO
    binding = importlib.import_module("hc-mvs_amd.binding")
    if world > 1:
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        views, srcs, neighbors, order, init = SO.ring_scene(n=5, w=96, h=80, f=90.0, n_points=60)
        p = binding.Params()
        po = O.default_params()
        for k, _ in p._fields_:
            setattr(p, k, getattr(po, k))
        p.seed = 900
        for k, v in KW.items():
            setattr(p, k, v)
        cloud = D.densify_scene(_context(), views, srcs, neighbors, order, init, p, device=torch.device("cpu"), n_external_iters=3, postfilter=True,
                                interleave=interleave, viewspread=True)
        ret[rank] = (cloud["n_points"], cloud["xyz"].tobytes(), {i: cloud["maps"][i][0].numpy().tobytes() for i in order})
    finally:
        if world > 1:
            dist.destroy_process_group()


def test_densify_scene_viewspread_two_ranks_both_schedules():
    import scene_oracle as SO
    clouds = {}
    for interleave in (False, True):
        mgr = mp.Manager()
        single = mgr.dict()
        mp.spawn(_scene_worker, args=(1, 0, single, interleave), nprocs=1, join=True)
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        ret = mgr.dict()
        mp.spawn(_scene_worker, args=(2, port, ret, interleave), nprocs=2, join=True)
        assert len(ret) == 2 and single[0][0] > 1000
        for r in (0, 1):
            assert ret[r][0] == single[0][0] and ret[r][1] == single[0][1]
            for i in single[0][2]:
                assert ret[r][2][i] == single[0][2][i]
        views, srcs, neighbors, order, init = SO.ring_scene(n=5, w=96, h=80, f=90.0, n_points=60)
        want = SO.densify(views, srcs, neighbors, order, init, viewspread=True, n_external_iters=3, postfilter=True, interleave=interleave, seed=900, **KW)
        assert want["spread"][0] > 0
        assert want["cloud"]["n_points"] == single[0][0] and want["cloud"]["xyz"].tobytes() == single[0][1]
        clouds[interleave] = single[0][1]
    assert clouds[False] != clouds[True]

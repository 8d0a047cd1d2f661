"""densify_scene(speckle_size=100): the maps it returns are the maps of the call without the option put through the numpy statement of
the speckle filter (tests/speckle_ref.py), bit for bit, and the counters it reports are the statement's.  The fused point counts with
and without the filter are printed."""
import importlib

import numpy as np
import pytest
import torch

import scene_oracle as S
import speckle_ref as R

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
D = importlib.import_module("hc-mvs_amd.distributed")


@pytest.mark.parametrize("batch", [32, 3])
def test_densify_scene_filters_the_finished_maps(batch):
    views, srcs, neighbors, order, init = S.ring_scene(n=4, w=128, h=96, f=120.0, n_points=80)
    kw = dict(adapthalfwin=6, n_estimation_iters=2)
    dev = torch.device("cuda", 0)
    ctx = binding.Context(0)
    try:
        p = binding.default_params(seed=900, **kw)
        run = lambda **more: D.densify_scene(ctx, views, srcs, neighbors, order, init, p, device=dev, n_external_iters=2, batch=batch, **more)
        off = run(fuse=False)
        assert "speckle" not in off
        off_maps = {i: [t.cpu().numpy() for t in off["maps"][i]] for i in order}
        on = run(fuse=False, speckle_size=100)
        total = {k: 0 for k in R.COUNTERS}
        for i in order:
            want = R.remove_speckles(*off_maps[i], thr=R.THR, speckle_size=100)
            for got, key in zip(on["maps"][i], ("depth", "normal", "conf")):
                assert R.same_bits(got.cpu().numpy(), want[key]), "image %d: %s" % (i, key)
            for k in R.COUNTERS:
                total[k] = max(total[k], want["stats"][k]) if k == "largest" else total[k] + want["stats"][k]
        assert total["n_removed"] > 0 and {k: on["speckle"][k] for k in R.COUNTERS} == total
        zero = run(fuse=False, speckle_size=0)
        for i in order:
            for a, b in zip(zero["maps"][i], off_maps[i]):
                assert R.same_bits(a.cpu().numpy(), b)
        with pytest.raises(ValueError):
            run(fuse=False, speckle_size=-1)
        if batch == 32:
            print("fused points: %d without the filter, %d with speckle_size=100 (%d of %d valid pixels removed)" %
                  (run()["n_points"], run(speckle_size=100)["n_points"], total["n_removed"], total["n_valid"]))
    finally:
        ctx.close()

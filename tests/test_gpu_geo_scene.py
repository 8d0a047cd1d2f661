"""distributed.densify_scene(geo=...) and DensifyPointCloud --geo-consistency 1 (files in, files out) on the GPU against the scene oracle
with the geometric-consistency term (tests/scene_oracle_geo.py), bit for bit, and the combinations they refuse."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import scene_oracle as SO
import scene_oracle_geo as SG
import test_gpu_driver_spread as DS
import test_gpu_schedule as GS

pytestmark = pytest.mark.gpu
mvsio = importlib.import_module("hc-mvs_amd.mvsio")
EXE = GS.EXE

binding = importlib.import_module("hc-mvs_amd.binding")
D = importlib.import_module("hc-mvs_amd.distributed")

KW = dict(adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4)


def test_densify_scene_with_geo_matches_the_scene_oracle():
    """three outer iterations on one context; the term blends from outer iteration 1 on, on the maps outer iteration it - 1 left"""
    import torch
    views, srcs, neighbors, order, init = SO.ring_scene(n=3, w=96, h=80, f=90.0, n_points=80)
    g = SO.gradient_map(views[0])[7:-7, 7:-7]
    geo = dict(para_tapa=0.26, para_tapa2=0.26, photo2geo=1, max_px=2.0, txthreshold=float(np.percentile(g, 40)) + 0.5, txthreshold2=float(np.percentile(g, 75)) + 0.5)
    want = SG.densify(views, srcs, init, geo, n_external_iters=3, seed=900, **KW)
    plain = SG.densify(views, srcs, init, None, n_external_iters=3, seed=900, **KW)
    assert want["evals_geo"] > 0 and want["pixels_geo"] > 0
    assert not all(np.array_equal(plain["maps"][i][0], want["maps"][i][0]) for i in order)       # the term is at work
    ctx = binding.Context(0)
    try:
        p = binding.default_params(seed=900, **KW)
        cloud = D.densify_scene(ctx, views, srcs, neighbors, order, init, p, device=torch.device("cuda", 0), n_external_iters=3, geo=geo, fuse=False)
        for i in order:
            d, n, c = [t.cpu().numpy() for t in cloud["maps"][i]]
            assert np.array_equal(d, want["maps"][i][0]), "depth map %d" % i
            assert np.array_equal(n, want["maps"][i][1]) and np.array_equal(c, want["maps"][i][2]), "normal / confidence map %d" % i
        # the switch and the registered maps are gone again: the same call without geo= is the plain result
        cloud = D.densify_scene(ctx, views, srcs, neighbors, order, init, p, device=torch.device("cuda", 0), n_external_iters=3, fuse=False)
        for i in order:
            assert np.array_equal(cloud["maps"][i][0].cpu().numpy(), plain["maps"][i][0]), "plain depth map %d" % i
        assert ctx.get_geo_stats() == dict(evals_geo=0, pixels_geo=0)
    finally:
        ctx.close()


def test_densify_scene_refuses_geo_with_viewspread_hints_and_priors():
    import torch
    views, srcs, neighbors, order, init = SO.ring_scene(n=3, w=96, h=80, f=90.0, n_points=60)
    ctx = binding.Context(0)
    try:
        p = binding.default_params(seed=1, **KW)
        prior = {0: np.ones((80, 96), np.float32)}
        hints = {0: (np.ones((80, 96), np.float32), np.zeros((80, 96, 3), np.float32))}
        for kw in (dict(viewspread=True), dict(priors=prior), dict(plane_priors={0: np.zeros((80, 96), np.uint16)}), dict(hints=hints)):
            with pytest.raises(ValueError) as e:
                D.densify_scene(ctx, views, srcs, neighbors, order, init, p, device=torch.device("cuda", 0), n_external_iters=3, geo=True, fuse=False, **kw)
            assert "geo" in str(e.value)
    finally:
        ctx.close()


def test_driver_geo_consistency_matches_the_scene_oracle(tmp_path):
    """DensifyPointCloud --geo-consistency 1 with the authors' weights over three outer iterations: the maps it writes are the scene
    oracle's; the refused combinations end the run with the parse error"""
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path)
    views, verts, scene_path = GS._driver_scene(tmp, n=4, w=128, h=96)
    oviews, srcs, neighbors, order, init = DS._oracle_inputs(views, verts)
    g = SO.gradient_map(oviews[0])[7:-7, 7:-7]
    tx = (float(np.floor(np.percentile(g, 40))) + 0.5, float(np.floor(np.percentile(g, 75))) + 0.5)
    kw = dict(adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4, photometric_flow=0.0)
    geo = dict(para_tapa=0.26, para_tapa2=0.125, photo2geo=1, max_px=2.0, txthreshold=tx[0], txthreshold2=tx[1])
    want = SG.densify(oviews, srcs, init, geo, n_external_iters=3, seed=779, **kw)
    assert want["evals_geo"] > 0 and want["pixels_geo"] > 0      # the term was at work (the test above: it changes the maps)

    def args(out, extra):
        return [EXE, "-i", scene_path, "-o", out, "--resolution-level", "0", "--min-resolution", "64", "--number-views", "3", "--n-EstimationIters", "2",
                "--n-EstimationIters-external", "3", "--n-adapthalfwin", "6", "--n-propagatehalfwin", "5", "--n-propagatestep", "4",
                "--n-photometric_flow", "0", "--min-views-trust-point", "1", "--n-postfilter", "0", "--seed", "779", "-v", "3"] + extra
    geo_args = ["--geo-consistency", "1", "--n-para_tapa", "0.26", "--n-para_tapa2", "0.125", "--n-photo2geo", "1", "--geo-max-px", "2",
                "--n-txthreshold", repr(tx[0]), "--n-txthreshold2", repr(tx[1])]
    out = os.path.join(tmp, "dense.mvs")
    r = subprocess.run(args(out, geo_args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Geometric consistency: para_tapa 0.26" in r.stdout
    for i in range(4):
        dm = mvsio.read_dmap(os.path.join(tmp, "depth%04d.dmap" % i))
        assert np.array_equal(dm["depth"], want["maps"][i][0]), "depth map %d differs from the oracle" % i
        assert np.array_equal(dm["normal"], want["maps"][i][1]) and np.array_equal(dm["conf"], want["maps"][i][2])
    for extra in (["--n-viewspread", "1"], ["--restore-hypothesis", "1"], ["--depth-priors", tmp], ["--plane-priors", "1"]):
        r = subprocess.run(args(os.path.join(tmp, "x.mvs"), geo_args + extra), capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "--geo-consistency 1 is not combined with " + extra[0] in r.stderr

"""Depth priors through the scene path: distributed.densify_scene(priors=...) and DensifyPointCloud --depth-priors (files in, files out)
against the scene-level oracle's prior schedule (tests/scene_oracle.py, priors=), bit for bit: on outer iteration n - 2 the priors are
registered after the ordinary estimate and the reference's two extra sweeps run; on the last outer iteration they stay registered.
The oracle's answer is computed once for both tests."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import prior_cases as PC
import scene_oracle as SO
import test_gpu_driver_spread as DS
import test_gpu_schedule as GS

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
D = importlib.import_module("hc-mvs_amd.distributed")
mvsio = importlib.import_module("hc-mvs_amd.mvsio")

EXE = GS.EXE
SEED, OUTER = 779, 2      # two outer iterations: the extra sweeps follow iteration 0 (below photo2geo: they run without the term), iteration 1 blends it
KW = dict(adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4, photometric_flow=0.0)
PRIOR = dict(para_prior=0.4, sigma_prior=0.2, photo2geo=1)      # the authors' schedule


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """four images of 128 x 96, priors for three of them, and the oracle's answer -- computed once for both tests"""
    tmp = str(tmp_path_factory.mktemp("prior_scene"))
    views, verts, scene_path = GS._driver_scene(tmp, n=4, w=128, h=96)
    oviews, srcs, neighbors, order, init = DS._oracle_inputs(views, verts)
    priors = {i: PC.make_prior(views[i], seed=i) for i in (0, 1, 3)}
    want = SO.densify(oviews, srcs, neighbors, order, init, priors=priors, prior_params=PRIOR, n_external_iters=OUTER, seed=SEED, **KW)
    assert want["evals_prior"] > 0      # the term was at work (tests/test_prior_oracle.py: it changes the maps)
    return dict(tmp=tmp, views=views, scene_path=scene_path, oviews=oviews, srcs=srcs, neighbors=neighbors, order=order, init=init, priors=priors, want=want)


def test_densify_scene_with_priors_matches_the_scene_oracle(scene):
    import torch
    s = scene
    ctx = binding.Context(0)
    try:
        p = binding.default_params(seed=SEED, **KW)
        dev = torch.device("cuda", 0)
        priors = dict(s["priors"])
        priors[1] = torch.from_numpy(priors[1]).to(dev)        # one of them in device memory
        cloud = D.densify_scene(ctx, s["oviews"], s["srcs"], s["neighbors"], s["order"], s["init"], p, device=dev, n_external_iters=OUTER, priors=priors,
                                prior_params=PRIOR)
        assert cloud["priors_used"] is True
        want = s["want"]
        for i in s["order"]:
            d, n, c = [t.cpu().numpy() for t in cloud["maps"][i]]
            assert np.array_equal(d, want["cloud"]["depths"][i]), "depth map %d" % i
            assert np.array_equal(n, want["maps"][i][1]) and np.array_equal(c, want["maps"][i][2]), "normal / confidence map %d" % i
        assert cloud["n_points"] == want["cloud"]["n_points"] > 1000 and np.array_equal(cloud["xyz"], want["cloud"]["xyz"])
        # fewer than two outer iterations: the priors are never used, which is noted, not raised
        one = D.densify_scene(ctx, s["oviews"], s["srcs"], s["neighbors"], s["order"], s["init"], p, device=dev, n_external_iters=1, priors=s["priors"],
                              prior_params=PRIOR, fuse=False)
        assert one["priors_used"] is False
        with pytest.raises(ValueError):
            D.densify_scene(ctx, s["oviews"], s["srcs"], s["neighbors"], s["order"], s["init"], p, device=dev, n_external_iters=OUTER, priors=s["priors"], viewspread=True)
    finally:
        ctx.close()


def _args(scene_path, out, extra):
    return [EXE, "-i", scene_path, "-o", out, "--resolution-level", "0", "--min-resolution", "64", "--number-views", "3", "--n-EstimationIters", "2",
            "--n-EstimationIters-external", str(OUTER), "--n-adapthalfwin", "6", "--n-propagatehalfwin", "5", "--n-propagatestep", "4",
            "--n-photometric_flow", "0", "--min-views-trust-point", "1", "--n-postfilter", "0", "--seed", str(SEED), "-v", "3"] + extra


def test_driver_depth_priors_match_the_scene_oracle(scene):
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    s = scene
    tmp = s["tmp"]
    folder = os.path.join(tmp, "priors")
    os.makedirs(folder, exist_ok=True)
    for i, m in s["priors"].items():
        v = s["views"][i]
        mvsio.write_dmap(os.path.join(folder, "depth%04d.prior.dmap" % i), m, v["K"], v["R"], v["C"], 0.0, 0.0, [i])
    out = os.path.join(tmp, "dense.mvs")
    prior_args = ["--depth-priors", folder, "--n-para_prior", "0.4", "--sigma-prior", "0.2", "--n-photo2geo", "1"]
    r = subprocess.run(_args(s["scene_path"], out, prior_args), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "3 of 4 images to estimate have one" in r.stdout
    want = s["want"]
    for i in range(4):
        dm = mvsio.read_dmap(os.path.join(tmp, "depth%04d.dmap" % i))
        assert np.array_equal(dm["depth"], want["maps"][i][0]), "depth map %d differs from the oracle" % i
        assert np.array_equal(dm["normal"], want["maps"][i][1]) and np.array_equal(dm["conf"], want["maps"][i][2])
    ply = mvsio.read_ply(out[:-4] + ".ply")
    xyz = np.stack([ply["x"], ply["y"], ply["z"]], -1)
    assert len(xyz) == want["cloud"]["n_points"] and np.array_equal(xyz, want["cloud"]["xyz"])
    # a prior of another size than the image is an error naming the file; the exclusive options are errors
    bad = os.path.join(folder, "depth0002.prior.dmap")
    v = s["views"][2]
    mvsio.write_dmap(bad, np.ones((48, 64), np.float32), v["K"], v["R"], v["C"], 0.0, 0.0, [2])
    r = subprocess.run(_args(s["scene_path"], os.path.join(tmp, "x.mvs"), prior_args + ["--resume", "0"]), capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and bad in r.stderr and "64x48" in r.stderr
    os.remove(bad)
    for extra in (["--n-viewspread", "1"], ["--restore-hypothesis", "1"]):
        r = subprocess.run(_args(s["scene_path"], os.path.join(tmp, "x.mvs"), prior_args + extra), capture_output=True, text=True, timeout=900)
        assert r.returncode != 0 and "--depth-priors" in r.stderr and extra[0] in r.stderr

"""DensifyPointCloud --plane-priors 1 --plane-clusters 1 (files in, files out) on the scene of test_gpu_driver_plane_prior.py: --ransac-cluster
is the cell of the inlier clustering, the "read and unused" note is gone, and the exported priors are what
Context.generate_plane_prior_device makes of the same live maps with cluster_mul = 2 (through densify_scene, which estimates the same
scene to the same bits); --plane-clusters 1 without --plane-priors 1 exits non-zero and names both options."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import test_gpu_driver_plane_prior as DPP
import test_gpu_driver_spread as DS
import test_gpu_schedule as GS

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
D = importlib.import_module("hc-mvs_amd.distributed")
mvsio = importlib.import_module("hc-mvs_amd.mvsio")

EXE = GS.EXE
LABELLED = DPP.LABELLED


def test_the_exported_priors_are_the_clustered_ones(tmp_path):
    import torch
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path)
    views, verts, scene_path = GS._driver_scene(tmp, n=4, w=128, h=96)
    labels = np.zeros((96, 128), np.uint8); labels[10:86, 12:116] = 255; labels[:5] = 9
    os.makedirs(os.path.join(tmp, "seman"))
    for i in LABELLED:
        mvsio.write_pgm(os.path.join(tmp, "seman", "view%03d.quad.pgm" % i), labels)
    wa, P = os.path.join(tmp, "A"), os.path.join(tmp, "P")
    os.makedirs(wa)
    ransac = ["--ransac-probability", "0.02", "--ransac-min-points", "60"]
    a = subprocess.run(DPP._args(scene_path, wa, ["--plane-priors", "1", "--plane-clusters", "1", "--ransac-cluster", "2", "--export-priors", P] + ransac),
                       capture_output=True, text=True, timeout=900)
    assert a.returncode == 0, a.stdout + a.stderr
    assert "read and unused" not in a.stdout + a.stderr
    assert "cells of 2 average spacings" in a.stdout and a.stdout.count("Plane clusters of image") == len(LABELLED)
    assert sorted(os.listdir(P)) == ["depth%04d.prior.dmap" % i for i in LABELLED]
    exported = {i: mvsio.read_dmap(os.path.join(P, "depth%04d.prior.dmap" % i))["depth"] for i in LABELLED}
    oviews, srcs, neighbors, order, init = DS._oracle_inputs(views, verts)
    ctx = binding.Context(0)
    try:
        cloud = D.densify_scene(ctx, oviews, srcs, neighbors, order, init, binding.default_params(seed=DPP.SEED, **DPP.KW), device=torch.device("cuda", 0),
                                n_external_iters=DPP.OUTER, prior_params=DPP.PRIOR, plane_priors={i: labels.astype(np.uint16) for i in LABELLED},
                                plane_prior_params=binding.default_plane_prior_params(seed=DPP.SEED, probability=0.02, min_points_div=60.0, cluster_mul=2.0), fuse=False)
        for i in LABELLED:
            assert np.array_equal(cloud["plane_prior_maps"][i].cpu().numpy(), exported[i]), "exported prior %d" % i
        for i in range(4):
            assert np.array_equal(cloud["maps"][i][0].cpu().numpy(), mvsio.read_dmap(os.path.join(wa, "depth%04d.dmap" % i))["depth"]), "depth map %d" % i
    finally:
        ctx.close()
    # the switch without the generation: an error that names both options, before anything is read
    r = subprocess.run(DPP._args(scene_path, os.path.join(tmp, "X"), ["--plane-clusters", "1"]), capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "--plane-clusters" in r.stderr and "--plane-priors" in r.stderr

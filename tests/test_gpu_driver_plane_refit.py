"""DensifyPointCloud --plane-refit n (files in, files out) on the small scene with label files of test_gpu_driver_plane_prior.py:
--plane-refit 0 writes the files a run without the option writes; --plane-refit 4 --export-priors writes the priors the library call gives on
the same live maps (through densify_scene(plane_prior_params=...), which estimates the same scene to the same bits), and says so with -v."""
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

LABELLED = DPP.LABELLED


def files_of(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder)) if name.endswith(".dmap")}


def test_no_steps_write_the_same_files_and_four_steps_the_priors_of_the_library(tmp_path):
    import torch
    assert os.path.exists(DPP.EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path)
    views, verts, scene_path = GS._driver_scene(tmp, n=4, w=128, h=96)
    labels = np.zeros((96, 128), np.uint8); labels[10:86, 12:116] = 255; labels[:5] = 9
    os.makedirs(os.path.join(tmp, "seman"))
    for i in LABELLED:
        mvsio.write_pgm(os.path.join(tmp, "seman", "view%03d.quad.pgm" % i), labels)
    ransac = ["--ransac-probability", "0.02", "--ransac-min-points", "60"]
    runs = {}
    for key, extra in (("plain", []), ("zero", ["--plane-refit", "0"]), ("four", ["--plane-refit", "4"])):
        work, P = os.path.join(tmp, key), os.path.join(tmp, "P" + key)
        os.makedirs(work)
        r = subprocess.run(DPP._args(scene_path, work, ["--plane-priors", "1", "--export-priors", P] + ransac + extra), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("Plane refit:" in r.stdout) == (key == "four") and ("Plane refit of image" in r.stdout) == (key == "four")
        runs[key] = (files_of(work), files_of(P))
    assert sorted(runs["plain"][1]) == ["depth%04d.prior.dmap" % i for i in LABELLED] and len(runs["plain"][0]) == 4
    assert runs["zero"] == runs["plain"]                                            # --plane-refit 0: byte for byte the files of a run without it
    assert runs["four"][1] != runs["plain"][1] and sorted(runs["four"][1]) == sorted(runs["plain"][1])
    exported = {i: mvsio.read_dmap(os.path.join(tmp, "Pfour", "depth%04d.prior.dmap" % i))["depth"] for i in LABELLED}
    assert all((m > 0).sum() > 1000 and not m[labels != 255].any() for m in exported.values())
    oviews, srcs, neighbors, order, init = DS._oracle_inputs(views, verts)
    ctx = binding.Context(0)
    try:
        cloud = D.densify_scene(ctx, oviews, srcs, neighbors, order, init, binding.default_params(seed=DPP.SEED, **DPP.KW), device=torch.device("cuda", 0),
                                n_external_iters=DPP.OUTER, prior_params=DPP.PRIOR, plane_priors={i: labels.astype(np.uint16) for i in LABELLED},
                                plane_prior_params=binding.default_plane_prior_params(seed=DPP.SEED, probability=0.02, min_points_div=60.0, refit_iters=4), fuse=False)
        for i in LABELLED:
            assert np.array_equal(cloud["plane_prior_maps"][i].cpu().numpy(), exported[i]), "exported prior %d" % i
        for i in range(4):
            assert np.array_equal(cloud["maps"][i][0].cpu().numpy(), mvsio.read_dmap(os.path.join(tmp, "four", "depth%04d.dmap" % i))["depth"]), "depth map %d" % i
    finally:
        ctx.close()
    # the refused uses
    for extra in (["--plane-refit", "4"], ["--plane-priors", "1", "--plane-refit", "17"]):
        r = subprocess.run(DPP._args(scene_path, os.path.join(tmp, "X"), extra), capture_output=True, text=True, timeout=900)
        assert r.returncode != 0 and "--plane-refit" in r.stderr

"""DensifyPointCloud --plane-priors 1 (files in, files out) on a small scene with label files: run A generates the priors on outer iteration
n - 2 and exports them, run B reads the exported files with --depth-priors -- both write bit-identical depth maps; the exported priors are
what Context.generate_plane_prior_device makes of the same live maps (through densify_scene(plane_priors=...), which estimates the same
scene to the same bits); the refused combinations exit non-zero and name both options."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import test_gpu_driver_spread as DS
import test_gpu_schedule as GS

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
D = importlib.import_module("hc-mvs_amd.distributed")
mvsio = importlib.import_module("hc-mvs_amd.mvsio")

EXE = GS.EXE
SEED, OUTER = 779, 2
KW = dict(adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4, photometric_flow=0.0)
PRIOR = dict(para_prior=0.4, sigma_prior=0.2, photo2geo=1)
LABELLED = (0, 1, 3)          # image 2 has no label file: no prior, a warning


def _args(scene_path, work, extra):
    return [EXE, "-i", scene_path, "-o", os.path.join(work, "dense.mvs"), "-w", work, "--resolution-level", "0", "--min-resolution", "64", "--number-views", "3",
            "--n-EstimationIters", "2", "--n-EstimationIters-external", str(OUTER), "--n-adapthalfwin", "6", "--n-propagatehalfwin", "5", "--n-propagatestep", "4",
            "--n-photometric_flow", "0", "--min-views-trust-point", "1", "--n-postfilter", "0", "--seed", str(SEED), "--n-para_prior", "0.4", "--sigma-prior", "0.2",
            "--n-photo2geo", "1", "-v", "3"] + extra


def test_generated_exported_and_supplied_priors_agree(tmp_path):
    import torch
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path)
    views, verts, scene_path = GS._driver_scene(tmp, n=4, w=128, h=96)
    labels = np.zeros((96, 128), np.uint8); labels[10:86, 12:116] = 255; labels[:5] = 9
    os.makedirs(os.path.join(tmp, "seman"))
    for i in LABELLED:
        mvsio.write_pgm(os.path.join(tmp, "seman", "view%03d.quad.pgm" % i), labels)
    wa, wb, P = os.path.join(tmp, "A"), os.path.join(tmp, "B"), os.path.join(tmp, "P")
    os.makedirs(wa); os.makedirs(wb)
    ransac = ["--ransac-probability", "0.02", "--ransac-min-points", "60"]
    a = subprocess.run(_args(scene_path, wa, ["--plane-priors", "1", "--export-priors", P, "--ransac-cluster", "2"] + ransac), capture_output=True, text=True, timeout=900)
    assert a.returncode == 0, a.stdout + a.stderr
    assert "3 of 4 images to estimate have a label image" in a.stdout and "view002.quad" in a.stderr and "--ransac-cluster is read and unused" in a.stdout + a.stderr
    assert sorted(os.listdir(P)) == ["depth%04d.prior.dmap" % i for i in LABELLED]
    b = subprocess.run(_args(scene_path, wb, ["--depth-priors", P]), capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stdout + b.stderr
    assert "3 of 4 images to estimate have one" in b.stdout
    for i in range(4):
        fa, fb = (open(os.path.join(w, "depth%04d.dmap" % i), "rb").read() for w in (wa, wb))
        assert fa == fb, "depth map file %d differs between the generated and the supplied priors" % i
    exported = {i: mvsio.read_dmap(os.path.join(P, "depth%04d.prior.dmap" % i))["depth"] for i in LABELLED}
    assert all((m > 0).sum() > 1000 and not m[labels != 255].any() for m in exported.values())
    # the same live maps through the binding: densify_scene estimates this scene as the driver does, and generates with the same parameters
    oviews, srcs, neighbors, order, init = DS._oracle_inputs(views, verts)
    ctx = binding.Context(0)
    try:
        cloud = D.densify_scene(ctx, oviews, srcs, neighbors, order, init, binding.default_params(seed=SEED, **KW), device=torch.device("cuda", 0), n_external_iters=OUTER,
                                prior_params=PRIOR, plane_priors={i: labels.astype(np.uint16) for i in LABELLED},
                                plane_prior_params=binding.default_plane_prior_params(seed=SEED, probability=0.02, min_points_div=60.0), fuse=False)
        for i in LABELLED:
            assert np.array_equal(cloud["plane_prior_maps"][i].cpu().numpy(), exported[i]), "exported prior %d" % i
        for i in range(4):
            assert np.array_equal(cloud["maps"][i][0].cpu().numpy(), mvsio.read_dmap(os.path.join(wa, "depth%04d.dmap" % i))["depth"]), "depth map %d" % i
    finally:
        ctx.close()
    # fewer than two outer iterations: a note, no prior, no file
    wc, Pc = os.path.join(tmp, "C"), os.path.join(tmp, "Pc")
    os.makedirs(wc)
    args = _args(scene_path, wc, ["--plane-priors", "1", "--export-priors", Pc])
    args[args.index("--n-EstimationIters-external") + 1] = "1"
    c = subprocess.run(args, capture_output=True, text=True, timeout=900)
    assert c.returncode == 0 and "needs two outer iterations" in c.stderr and os.listdir(Pc) == []
    # the refused combinations
    for extra in (["--depth-priors", P], ["--n-viewspread", "1"], ["--restore-hypothesis", "1"]):
        r = subprocess.run(_args(scene_path, os.path.join(tmp, "X"), ["--plane-priors", "1"] + extra), capture_output=True, text=True, timeout=900)
        assert r.returncode != 0 and "--plane-priors" in r.stderr and extra[0] in r.stderr

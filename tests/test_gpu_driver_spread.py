"""DensifyPointCloud --n-viewspread 1 (files in, files out) against the scene-level oracle harness with view spread
(tests/scene_oracle.py, viewspread=True) in the same schedule, bit for bit: the batch schedule (the maps of the previous outer iteration, copied)
and --n-postfilter-interleave 1 (the reference's order on the live maps; with four outer iterations the last one is estimated image
after image without a filter).  And the combinations the driver refuses or leaves alone."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scene_files as SF
import scene_oracle as SO
import test_gpu_schedule as GS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import select_views as SV  # noqa: E402

pytestmark = pytest.mark.gpu
mvsio = importlib.import_module("hc-mvs_amd.mvsio")

EXE = GS.EXE


def _args(scene_path, out, seed, outer, extra):
    return [EXE, "-i", scene_path, "-o", out, "--resolution-level", "0", "--min-resolution", "64", "--number-views", "3", "--n-EstimationIters", "2",
            "--n-EstimationIters-external", str(outer), "--n-adapthalfwin", "6", "--n-propagatehalfwin", "5", "--n-propagatestep", "4",
            "--n-photometric_flow", "0", "--min-views-trust-point", "1", "--seed", str(seed), "-v", "3"] + extra


def _oracle_inputs(views, verts):
    n = len(views)
    cams = [dict(K=v["K"], R=v["R"], C=v["C"]) for v in views]
    sizes = [(v["width"], v["height"]) for v in views]
    vlist = [(x["X"], [j for j, _ in x["views"]]) for x in verts]
    g8 = [np.clip(np.rint(v["gray"] * 255), 0, 255).astype(np.uint8) for v in views]
    oviews, srcs, neighbors, init = {}, {}, {}, {}
    for i in range(n):
        sel = SV.select(cams, sizes, vlist, i, number_views=3)
        assert sel is not None
        srcs[i] = [s[0] for s in sel["srcs"]]
        assert all(abs(s[1] - 1) < 0.15 for s in sel["srcs"])
        neighbors[i] = [nb["id"] for nb in sel["neighbors"]]
        oviews[i] = dict(K=views[i]["K"], R=views[i]["R"], C=views[i]["C"], gray=SF.driver_gray(g8[i]), bgr=np.stack([g8[i]] * 3, -1).copy())
        pts = np.ascontiguousarray(np.stack([verts[k]["X"] for k in sel["points"]]), np.float32)
        init[i] = SO.splat(oviews[i], pts)
    order = sorted(range(n), key=lambda i: -len(neighbors[i]))
    return oviews, srcs, neighbors, order, init


@pytest.mark.parametrize("interleave,outer", [(0, 3), (1, 4)], ids=["batch", "interleaved"])
def test_driver_viewspread_matches_the_scene_oracle(tmp_path, interleave, outer):
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path)
    views, verts, scene_path = GS._driver_scene(tmp)
    out = os.path.join(tmp, "dense.mvs")
    seed = 778
    r = subprocess.run(_args(scene_path, out, seed, outer, ["--n-viewspread", "1", "--n-postfilter-interleave", str(interleave)]),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "not available" not in r.stderr
    oviews, srcs, neighbors, order, init = _oracle_inputs(views, verts)
    want = SO.densify(oviews, srcs, neighbors, order, init, viewspread=True, n_external_iters=outer, postfilter=True, interleave=bool(interleave), seed=seed, n_threads=16,
                       adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4, photometric_flow=0.0)
    assert want["spread"][0] > 0 and want["spread"][2] == 0
    plain = SO.densify(oviews, srcs, neighbors, order, init, n_external_iters=outer, postfilter=True, interleave=bool(interleave), seed=seed, n_threads=16, fuse=False,
                       adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4, photometric_flow=0.0)
    assert not all(np.array_equal(plain["maps"][i][0], want["maps"][i][0]) for i in range(len(views)))
    for i in range(len(views)):
        dm = mvsio.read_dmap(os.path.join(tmp, "depth%04d.dmap" % i))
        assert np.array_equal(dm["depth"], want["maps"][i][0]), "depth map %d differs from the oracle (%s schedule)" % (i, "interleaved" if interleave else "batch")
        assert np.array_equal(dm["normal"], want["maps"][i][1]) and np.array_equal(dm["conf"], want["maps"][i][2])
    ply = mvsio.read_ply(out[:-4] + ".ply")
    xyz = np.stack([ply["x"], ply["y"], ply["z"]], -1)
    assert len(xyz) == want["cloud"]["n_points"] > 10000 and np.array_equal(xyz, want["cloud"]["xyz"])
    m = re.search(r"(\d+) depth-maps, (\d+) depths, (\d+) points", r.stdout)
    assert m and int(m.group(3)) == want["cloud"]["n_points"]


def test_driver_viewspread_default_is_off_and_several_devices_are_refused(tmp_path):
    """without the flag (or with 0) the run is today's; with --devices a,b the combination is refused with a clear error"""
    tmp = str(tmp_path)
    views, verts, scene_path = GS._driver_scene(tmp, n=4, w=128, h=96)
    outs = []
    for k, extra in enumerate([[], ["--n-viewspread", "0"]]):
        out = os.path.join(tmp, "dense%d.mvs" % k)
        r = subprocess.run(_args(scene_path, out, 5, 2, extra), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([mvsio.read_dmap(os.path.join(tmp, "depth%04d.dmap" % i))["depth"] for i in range(4)])
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
    oviews, srcs, neighbors, order, init = _oracle_inputs(views, verts)
    want = SO.densify(oviews, srcs, neighbors, order, init, n_external_iters=2, postfilter=True, seed=5, n_threads=16, fuse=False,
                      adapthalfwin=6, n_estimation_iters=2, propagate_halfwin=5, propagate_step=4, photometric_flow=0.0)
    assert all(np.array_equal(outs[0][i], want["maps"][i][0]) for i in range(4))
    r = subprocess.run(_args(scene_path, os.path.join(tmp, "x.mvs"), 5, 2, ["--n-viewspread", "1", "--devices", "0,0"]), capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "--n-viewspread" in r.stderr and "one device" in r.stderr

"""DensifyPointCloud --n-filter 1|2 (files in, files out): the final .dmap files are the maps of the --n-filter 0 run put through
Context.filter_sequence (pinned against the oracle in test_gpu_filter_stage.py), byte for byte; the .ply is the fusion of those maps;
--devices 0,0 gives the same files; --n-filter 0 is the run without the option."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import scene_files as SF
import test_gpu_schedule as GS

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import select_views as SV  # noqa: E402

pytestmark = pytest.mark.gpu
mvsio = importlib.import_module("hc-mvs_amd.mvsio")
binding = importlib.import_module("hc-mvs_amd.binding")

EXE = GS.EXE
N, W, H = 5, 160, 120


def _run(scene, work, *extra):
    os.makedirs(work, exist_ok=True)
    r = subprocess.run([EXE, "-i", scene, "-w", work, "-o", os.path.join(work, "dense.mvs"), "--resolution-level", "0", "--min-resolution", "64",
                        "--number-views", "3", "--n-nOptimize", "0", "--n-EstimationIters", "2", "--n-EstimationIters-external", "2", "--n-adapthalfwin", "5",
                        "--min-views-trust-point", "1", "--seed", "11", "-v", "2"] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _files(work):
    return [open(os.path.join(work, "depth%04d.dmap" % i), "rb").read() for i in range(N)] + [open(os.path.join(work, "dense.ply"), "rb").read()]


def _with_maps(raw, dm, depth, conf):
    """the bytes of a complete DR file with depth and confidence replaced (header, ids, camera and normals as they are)"""
    px = depth.size
    tail = px * 4 + px * 12 + px * 4
    head = len(raw) - tail
    assert raw[head:head + px * 4] == dm["depth"].tobytes()
    return raw[:head] + depth.tobytes() + raw[head + px * 4:head + px * 16] + conf.tobytes()


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path_factory.mktemp("filter_driver"))
    views, verts, scene = GS._driver_scene(tmp, n=N, w=W, h=H)
    _run(scene, os.path.join(tmp, "off"), "--n-filter", "0")
    return tmp, views, verts, scene


def test_n_filter_0_is_the_run_without_the_option(plain):
    tmp, views, verts, scene = plain
    r = _run(scene, os.path.join(tmp, "none"))
    assert "Depth-maps filtered:" not in r.stdout
    assert _files(os.path.join(tmp, "none")) == _files(os.path.join(tmp, "off"))


@pytest.mark.parametrize("mode", [1, 2], ids=["adjust", "strict"])
def test_driver_filter_stage(plain, mode):
    tmp, views, verts, scene = plain
    work = os.path.join(tmp, "mode%d" % mode)
    r = _run(scene, work, "--n-filter", str(mode))
    m = re.search(r"Depth-maps filtered: (\d+) images, (\d+)/(\d+) depths discarded \((\d+) skipped\)", r.stdout)
    assert m, r.stdout
    # the maps of the --n-filter 0 run through the binding's stage, with the driver's neighbour lists (all of the view selection's
    # neighbours, best first) and its clamped view counts (SceneDensify.cpp:3014-3015)
    cams = [dict(K=v["K"], R=v["R"], C=v["C"]) for v in views]
    sizes = [(v["width"], v["height"]) for v in views]
    vlist = [(x["X"], [j for j, _ in x["views"]]) for x in verts]
    off = os.path.join(tmp, "off")
    raws = _files(off)
    dms = [mvsio.read_dmap(os.path.join(off, "depth%04d.dmap" % i)) for i in range(N)]
    neighbors = {}
    ctx = binding.Context(0)
    try:
        for i, v in enumerate(views):
            g8 = np.clip(np.rint(v["gray"] * 255), 0, 255).astype(np.uint8)
            ctx.upload_view(i, SF.driver_gray(g8), v["K"], v["R"], v["C"], bgr=np.stack([g8] * 3, -1).copy())
            sel = SV.select(cams, sizes, vlist, i, number_views=3)
            neighbors[i] = [nb["id"] for nb in sel["neighbors"]][:31]
            ctx.set_depthmap(i, dms[i]["depth"], dms[i]["normal"], dms[i]["conf"], dms[i]["d_min"], dms[i]["d_max"])
            ctx.set_neighbors(i, neighbors[i])
        st = ctx.filter_sequence(range(N), max_neighbors=8, adjust=mode == 1, n_min_views=min(2, N - 1), n_min_views_adjust=min(1, N - 1))
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) == (st["n_filtered"], st["n_discarded"], st["n_processed"], st["n_skipped"])
        assert st["n_filtered"] == N and 0 < st["n_discarded"] < st["n_processed"]
        got = _files(work)
        for i in range(N):
            d, c = ctx.get_depthmap(i)
            assert not np.array_equal(d, dms[i]["depth"])
            assert got[i] == _with_maps(raws[i], dms[i], d, c), "depth%04d.dmap is not the filtered map of the --n-filter 0 run" % i
        order = sorted(range(N), key=lambda i: -len(neighbors[i]))
        cloud = ctx.fuse(order, W * H * N // 2 + 16)
    finally:
        ctx.close()
    ply = mvsio.read_ply(os.path.join(work, "dense.ply"))
    xyz = np.stack([ply["x"], ply["y"], ply["z"]], -1)
    assert len(xyz) == cloud["n_points"] > 1000 and np.array_equal(xyz, cloud["xyz"])
    assert got[N] != raws[N]
    # two contexts on one device: the stage runs on the first, after the gather; the same files
    two = os.path.join(tmp, "two%d" % mode)
    _run(scene, two, "--n-filter", str(mode), "--devices", "0,0")
    assert _files(two) == got

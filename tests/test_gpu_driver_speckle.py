"""DensifyPointCloud --speckle-size 100 (files in, files out): the final .dmap files are the maps of the run without the option put
through the numpy statement of the speckle filter (tests/speckle_ref.py), bit for bit; the printed counts are the statement's;
--speckle-size 0 is the run without the option.  The fused point counts of both runs are printed."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import speckle_ref as R
import test_gpu_schedule as GS

pytestmark = pytest.mark.gpu
mvsio = importlib.import_module("hc-mvs_amd.mvsio")

EXE = GS.EXE
N, W, H = 4, 160, 120


def _run(scene, work, *extra):
    os.makedirs(work, exist_ok=True)
    r = subprocess.run([EXE, "-i", scene, "-w", work, "-o", os.path.join(work, "dense.mvs"), "--resolution-level", "0", "--min-resolution", "64",
                        "--number-views", "3", "--n-nOptimize", "0", "--n-EstimationIters", "2", "--n-EstimationIters-external", "2", "--n-adapthalfwin", "5",
                        "--min-views-trust-point", "1", "--seed", "11", "-v", "2"] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _maps(work):
    return [mvsio.read_dmap(os.path.join(work, "depth%04d.dmap" % i)) for i in range(N)]


def _points(work):
    return len(mvsio.read_ply(os.path.join(work, "dense.ply"))["x"])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path_factory.mktemp("speckle_driver"))
    views, verts, scene = GS._driver_scene(tmp, n=N, w=W, h=H)
    r = _run(scene, os.path.join(tmp, "off"))
    assert "Speckle filter" not in r.stdout
    return tmp, scene


def test_speckle_size_0_is_the_run_without_the_option(plain):
    tmp, scene = plain
    r = _run(scene, os.path.join(tmp, "zero"), "--speckle-size", "0")
    assert "Speckle filter" not in r.stdout
    for name in ["depth%04d.dmap" % i for i in range(N)] + ["dense.ply"]:
        assert open(os.path.join(tmp, "zero", name), "rb").read() == open(os.path.join(tmp, "off", name), "rb").read(), name


@pytest.mark.parametrize("extra", [(), ("--speckle-diff", "0.02"), ("--devices", "0,0"), ("--batch", "3")], ids=["default", "diff", "two_contexts", "batch3"])
def test_driver_speckle_filter(plain, extra):
    tmp, scene = plain
    work = os.path.join(tmp, "on_" + "_".join(e.strip("-").replace(",", "") for e in extra))
    r = _run(scene, work, "--speckle-size", "100", *extra)
    m = re.search(r"Speckle filter \(segments below 100 pixels, depth difference below ([^)]*)\): (\d+) segments, (\d+) small, (\d+) of (\d+) pixels removed", r.stdout)
    assert m, r.stdout
    assert len(re.findall(r"Speckle filter", r.stdout)) == 1                                     # one line per run
    thr = np.float32(0.02) if "--speckle-diff" in extra else R.THR
    total = dict(n_segments=0, n_small=0, n_removed=0, n_valid=0)
    for i, (off, on) in enumerate(zip(_maps(os.path.join(tmp, "off")), _maps(work))):
        want = R.remove_speckles(off["depth"], off["normal"], off["conf"], thr, 100)
        for key in ("depth", "normal", "conf"):
            assert R.same_bits(on[key], want[key]), "depth%04d.dmap: %s is not the filtered map of the run without the option" % (i, key)
        assert (on["d_min"], on["d_max"]) == (off["d_min"], off["d_max"])
        for k in total:
            total[k] += want["stats"][k]
    assert total["n_removed"] > 0
    assert (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))) == (total["n_segments"], total["n_small"], total["n_removed"], total["n_valid"])
    print("fused points: %d without the filter, %d with --speckle-size 100 %s (%d of %d valid pixels removed)" %
          (_points(os.path.join(tmp, "off")), _points(work), " ".join(extra), total["n_removed"], total["n_valid"]))


def test_later_stages_see_the_filtered_maps(plain):
    """--fusion-mode 1 (the maps are the result) writes the filtered maps too, and a --resume 1 run takes them as they are"""
    tmp, scene = plain
    work = os.path.join(tmp, "maps_only")
    _run(scene, work, "--speckle-size", "100", "--fusion-mode", "1")
    first = [open(os.path.join(work, "depth%04d.dmap" % i), "rb").read() for i in range(N)]
    for off, on in zip(_maps(os.path.join(tmp, "off")), _maps(work)):
        assert R.same_bits(on["depth"], R.remove_speckles(off["depth"], thr=R.THR, speckle_size=100)["depth"])
    _run(scene, work, "--speckle-size", "100", "--fusion-mode", "1", "--resume", "1")
    assert [open(os.path.join(work, "depth%04d.dmap" % i), "rb").read() for i in range(N)] == first

"""--ignore-mask-label through the DensifyPointCloud driver: label images found by the fork's rule (<folder>/seman/<stem>.quad, read as
binary PGM / PPM), 8- and 16-bit, one image without a label file.  Bit-exactness of the masked estimate is pinned at the binding level
(test_gpu_mask.py); here: what the maps hold on ignored pixels after the estimate, the unmasked image, and --devices."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import oracle_mask_lib as M
import scene_files as SF

synth = importlib.import_module("hc-mvs_amd.synth")
mvsio = importlib.import_module("hc-mvs_amd.mvsio")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hc-mvs_amd", "DensifyPointCloud")
W, H = 160, 120


def _write_pgm16(path, lab):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (lab.shape[1], lab.shape[0]))
        f.write(np.ascontiguousarray(lab, ">u2").tobytes())


def _scene(tmp):
    views = synth.make_views(W, H, 180.0, 3, seed=6, baseline=(0.04, 0.09))
    verts = SF.sparse_vertices(views, 120)
    path = SF.write_scene(tmp, views, verts, "pgm")
    os.makedirs(os.path.join(tmp, "seman"), exist_ok=True)
    yy, xx = np.mgrid[:H // 2, :W // 2]
    lab0 = np.zeros((H // 2, W // 2), np.uint8)               # 8-bit, half the size: enlarged on the device
    lab0[(yy - 20) ** 2 + (xx - 30) ** 2 < 150] = 3
    lab0[:, 55] = 3                                            # a one-pixel line (two pixels wide once enlarged)
    mvsio.write_pgm(os.path.join(tmp, "seman", "view000.quad.pgm"), lab0)
    lab1 = np.zeros((H, W), np.uint16)                         # 16-bit, labels above 255
    lab1[:30, :] = 300; lab1[60:, 100] = 300; lab1[70:90, 20:40] = 7
    _write_pgm16(os.path.join(tmp, "seman", "view001.quad.pgm"), lab1)
    lab3 = np.zeros((H, W, 3), np.uint8)                       # colour: cv::cvtColor BGR2GRAY of (3, 3, 3) is 3
    lab3[H // 2:, :W // 3] = 3
    mvsio.write_ppm(os.path.join(tmp, "seman", "view003.quad.ppm"), lab3)
    return path, {0: lab0, 1: lab1, 3: lab3[..., 0]}          # (view002 has no label file)


def _run(scene, work, *extra):
    os.makedirs(work, exist_ok=True)
    r = subprocess.run([EXE, "-i", scene, "-w", work, "-o", os.path.join(work, "dense.mvs"), "--resolution-level", "0", "--number-views", "3",
                        "--fusion-mode", "1", "--n-nOptimize", "0", "--n-EstimationIters", "2", "--n-EstimationIters-external", "2",
                        "-v", "2"] + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _maps(work, i):
    return open(os.path.join(work, "depth%04d.dmap" % i), "rb").read(), mvsio.read_dmap(os.path.join(work, "depth%04d.dmap" % i))


@pytest.mark.gpu
def test_driver_ignore_mask(tmp_path):
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    tmp = str(tmp_path)
    scene, labels = _scene(tmp)
    ignore = M.parse_labels("3,300")
    r = _run(scene, os.path.join(tmp, "masked"), "--ignore-mask-label", "3,300")
    assert "Ignore mask (labels 3,300): 3 of " in r.stdout
    assert "view002.quad.png" in r.stderr and "view002.quad.pgm" in r.stderr  # the warning names the fork's path and the sibling tried
    _run(scene, os.path.join(tmp, "plain"))
    for i in range(4):
        raw, dm = _maps(os.path.join(tmp, "masked"), i)
        if i not in labels:
            assert raw == _maps(os.path.join(tmp, "plain"), i)[0]  # no label file: exactly the unmasked run
            continue
        keep = M.keep_mask(labels[i], ignore, W, H)
        ign = keep == 0
        assert ign.any() and not ign.all()
        assert (dm["normal"][ign] == 0).all() and (dm["conf"][ign] == 0).all()
        # a positive depth on an ignored pixel only where the median window holds at least five values of estimated pixels
        kept_in_window = M.median3_window_valid(keep, np.ones((H, W), np.float32))
        assert (dm["depth"][ign & (kept_in_window < 5)] == 0).all()
        assert (dm["depth"][~ign] > 0).mean() > 0.05
    # two contexts on one device: the same files, byte for byte
    _run(scene, os.path.join(tmp, "two"), "--ignore-mask-label", "3,300", "--devices", "0,0")
    for i in range(4):
        assert _maps(os.path.join(tmp, "two"), i)[0] == _maps(os.path.join(tmp, "masked"), i)[0]

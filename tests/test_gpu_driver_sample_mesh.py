"""DensifyPointCloud --sample-mesh (files in, files out): the .ply the driver writes for a PLY mesh is the cloud of Context.sample_mesh
(pinned against the numpy reference in test_gpu_mesh_sample.py) in the dense cloud's file format, byte for byte; inputs the mode does not
read are refused with a message."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
mvsio = importlib.import_module("hc-mvs_amd.mvsio")
binding = importlib.import_module("hc-mvs_amd.binding")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hc-mvs_amd", "DensifyPointCloud")


def grid_mesh(n=12):
    """a bumpy height field of 2 n^2 triangles over [0, 4] x [0, 3], with texture coordinates over the whole texture"""
    r = np.random.default_rng(6)
    g = np.linspace(0, 1, n + 1, dtype=np.float32)
    u, v = np.meshgrid(g, g, indexing="xy")
    V = np.stack([4 * u, 3 * v, 0.3 * r.standard_normal(u.shape)], -1).reshape(-1, 3).astype(np.float32)
    uv = np.stack([u, v], -1).reshape(-1, 2).astype(np.float32)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    Fc = np.concatenate([np.stack([i, i + 1, i + n + 2], -1), np.stack([i, i + n + 2, i + n + 1], -1)]).astype(np.uint32)
    return V, Fc, uv[Fc]


def run(*args):
    return subprocess.run([EXE] + list(args), capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def ctx():
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    c = binding.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("sample, ascii", [(-5000.0, False), (0.5, True)], ids=["count", "density"])
def test_driver_writes_the_cloud_of_the_binding(ctx, tmp_path, sample, ascii):
    V, Fc, _ = grid_mesh()
    if sample > 0:
        V = V * np.float32(20)  # about 10 000 square units
    mesh = str(tmp_path / "mesh.ply")
    mvsio.write_ply_mesh(mesh, V, Fc, ascii=ascii)
    r = run("-i", mesh, "-o", str(tmp_path / "cloud.mvs"), "--sample-mesh", repr(sample), "--seed", "7", "-v", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    xyz, fid, bgr, st = ctx.sample_mesh(V, Fc, sample, seed=7)
    assert bgr is None and 4500 < len(xyz) < 6500
    m = re.search(r"Sample mesh completed: (\d+) points \(", r.stdout)
    assert m and int(m.group(1)) == len(xyz), r.stdout
    want = str(tmp_path / "want.ply")
    mvsio.write_ply(want, xyz)
    assert open(str(tmp_path / "cloud.ply"), "rb").read() == open(want, "rb").read()
    # another seed, another cloud; no --seed is the driver's default seed
    r = run("-i", mesh, "-o", str(tmp_path / "other.mvs"), "--sample-mesh", repr(sample), "-v", "0")
    assert r.returncode == 0 and r.stdout == "", r.stdout + r.stderr
    mvsio.write_ply(want, ctx.sample_mesh(V, Fc, sample, seed=1234)[0])
    assert open(str(tmp_path / "other.ply"), "rb").read() == open(want, "rb").read()


def test_driver_colours_a_textured_mesh(ctx, tmp_path):
    V, Fc, tc = grid_mesh()
    rgb = np.random.default_rng(8).integers(0, 256, (16, 24, 3)).astype(np.uint8)
    mvsio.write_ppm(str(tmp_path / "skin.ppm"), rgb)
    mesh = str(tmp_path / "mesh.ply")
    mvsio.write_ply_mesh(mesh, V, Fc, texcoords=tc, texture_file="skin.ppm")
    r = run("-i", mesh, "-o", str(tmp_path / "cloud.mvs"), "--sample-mesh", "-5000", "--seed", "7", "-v", "2")
    assert r.returncode == 0 and "Sample mesh completed:" in r.stdout, r.stdout + r.stderr
    xyz, fid, bgr, st = ctx.sample_mesh(V, Fc, -5000, seed=7, texcoords=tc, texture_bgr=rgb[:, :, ::-1])
    want = str(tmp_path / "want.ply")
    mvsio.write_ply(want, xyz, bgr=bgr)
    assert open(str(tmp_path / "cloud.ply"), "rb").read() == open(want, "rb").read()
    # the texture is not a binary PPM: positions only, and a note
    mvsio.write_ply_mesh(mesh, V, Fc, texcoords=tc, texture_file="skin.png")
    r = run("-i", mesh, "-o", str(tmp_path / "plain.mvs"), "--sample-mesh", "-5000", "--seed", "7", "-v", "2")
    assert r.returncode == 0 and "positions only" in r.stderr, r.stdout + r.stderr
    mvsio.write_ply(want, xyz)
    assert open(str(tmp_path / "plain.ply"), "rb").read() == open(want, "rb").read()


def test_inputs_the_mode_does_not_read(tmp_path):
    assert os.path.exists(EXE), "build the driver first: make -C hc-mvs_amd/csrc"
    obj = str(tmp_path / "mesh.obj")
    with open(obj, "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    r = run("-i", obj, "-o", str(tmp_path / "a.mvs"), "--sample-mesh", "-100")
    assert r.returncode != 0 and "OBJ" in r.stderr and "not supported" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "a.ply"))
    quad = str(tmp_path / "quad.ply")
    with open(quad, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                b"property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    r = run("-i", quad, "-o", str(tmp_path / "b.mvs"), "--sample-mesh", "-100")
    assert r.returncode != 0 and "face 0 has 4 vertices" in r.stderr and "triangles" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "b.ply"))

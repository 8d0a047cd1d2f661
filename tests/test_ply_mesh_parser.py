"""The driver's PLY mesh reader (hc-mvs_amd/host/ply_mesh.h, DensifyPointCloud --sample-mesh) on good and on broken files.
tests/ply_mesh_shim.cpp is compiled with g++ -fsanitize=address,undefined into a program of its own and run as a child process: a bad
file must give an error message and exit code 1 -- no crash, no sanitizer report.  Nothing is loaded into Python."""
import importlib
import os
import subprocess

import numpy as np
import pytest

mvsio = importlib.import_module("hc-mvs_amd.mvsio")
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ply_mesh_shim.cpp")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ply_mesh_shim") / "ply_mesh_shim")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def run(exe, path):
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert r.returncode in (0, 1), (r.returncode, r.stdout, r.stderr)   # a crash or a sanitizer abort is neither
    assert r.stdout.startswith("ok " if r.returncode == 0 else "error: "), r.stdout
    return r.returncode, r.stdout.strip()


def mesh(n_v=30, n_f=50, seed=2):
    r = np.random.default_rng(seed)
    return (r.standard_normal((n_v, 3)) * 10).astype(np.float32), r.integers(0, n_v, (n_f, 3)).astype(np.uint32), r.random((n_f, 3, 2)).astype(np.float32)


def checksum(V, Fc, T=None):
    s = 0
    parts = [V.ravel().view(np.uint32), Fc.ravel()] + ([] if T is None else [T.ravel().view(np.uint32)])
    for v in np.concatenate(parts).tolist():
        s = (s * 1099511628211 + v) & ((1 << 64) - 1)
    return s


@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
def test_good_files(shim, tmp_path, ascii):
    V, Fc, T = mesh()
    p = str(tmp_path / "m.ply")
    mvsio.write_ply_mesh(p, V, Fc, ascii=ascii)
    assert run(shim, p) == (0, "ok 30 50 0 %d" % checksum(V, Fc))
    mvsio.write_ply_mesh(p, V, Fc, texcoords=T, texture_file="skin.ppm", ascii=ascii, index_type="uint", list_name="vertex_index")
    assert run(shim, p) == (0, "ok 30 50 50 %d skin.ppm" % checksum(V, Fc, T))


def test_extra_properties_and_elements_are_skipped(shim, tmp_path):
    p = str(tmp_path / "m.ply")
    with open(p, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                b"element face 1\nproperty list uchar int vertex_indices\nproperty int flags\nelement edge 1\nproperty int a\nproperty int b\nend_header\n"
                b"0 0 0 255\n1 0 0 255\n0 1 0 7\n3 0 1 2 9\n0 1\n")
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    assert run(shim, p) == (0, "ok 3 1 0 %d" % checksum(V, np.array([0, 1, 2], np.uint32)))


@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
def test_truncated_files(shim, tmp_path, ascii):
    V, Fc, T = mesh()
    good = str(tmp_path / "good.ply")
    mvsio.write_ply_mesh(good, V, Fc, texcoords=T, texture_file="skin.ppm", ascii=ascii)
    data = open(good, "rb").read()
    body = data.index(b"end_header\n") + 11
    p = str(tmp_path / "cut.ply")
    # inside the header, at the start of the data, inside the vertices, inside the faces, one byte short (binary: in ascii a shortened last number is still a number)
    for cut in [0, 3, 20, body - 5, body, body + 7, body + (len(data) - body) // 3, len(data) - 40] + ([] if ascii else [len(data) - 1]):
        with open(p, "wb") as f:
            f.write(data[:cut])
        rc, out = run(shim, p)
        assert rc == 1, (cut, out)


def test_a_face_that_is_not_a_triangle(shim, tmp_path):
    p = str(tmp_path / "quad.ply")
    with open(p, "wb") as f:
        f.write(b"ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 2\n"
                b"property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n3 0 1 2\n4 0 1 2 3\n")
    rc, out = run(shim, p)
    assert rc == 1 and "face 1 has 4 vertices" in out and "triangles" in out
    V, Fc, _ = mesh()
    rec = np.zeros(len(Fc), np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    rec["n"] = 3; rec["i"] = Fc
    rec["n"][17] = 200  # a binary face that claims 200 indices
    with open(p, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 30\nproperty float x\nproperty float y\nproperty float z\nelement face 50\n"
                b"property list uchar int vertex_indices\nend_header\n" + V.tobytes() + rec.tobytes())
    rc, out = run(shim, p)
    assert rc == 1 and "face 17 has 200 vertices" in out


@pytest.mark.parametrize("bad", [30, 2 ** 31 - 1, -1, 2 ** 32 - 1], ids=["n", "intmax", "minus1", "u32max"])
def test_an_index_out_of_range(shim, tmp_path, bad):
    V, Fc, _ = mesh()
    p = str(tmp_path / "idx.ply")
    F2 = Fc.astype(np.int64); F2[33, 1] = bad
    mvsio.write_ply_mesh(p, V, F2.astype(np.uint32) if bad > 0 else F2.astype(np.int32), index_type="uint" if bad > 0 else "int")
    rc, out = run(shim, p)
    assert rc == 1 and "face 33 names vertex" in out and "of 30" in out
    if bad < 2 ** 31:
        mvsio.write_ply_mesh(p, V, F2, ascii=True)
        rc, out = run(shim, p)
        assert rc == 1 and "face 33 names vertex" in out


@pytest.mark.parametrize("count", [51, 10 ** 6, 2 ** 32 - 1, 2 ** 40, 2 ** 64 - 1], ids=str)
@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
def test_a_face_count_larger_than_the_file(shim, tmp_path, ascii, count):
    V, Fc, _ = mesh()
    good = str(tmp_path / "good.ply")
    mvsio.write_ply_mesh(good, V, Fc, ascii=ascii)
    data = open(good, "rb").read().replace(b"element face 50\n", b"element face %d\n" % count)
    p = str(tmp_path / "lie.ply")
    with open(p, "wb") as f:
        f.write(data)
    rc, out = run(shim, p)
    assert rc == 1 and ("claims more rows" in out or "the file ends" in out or "more than 2^32" in out), out
    # the same lie about the vertices
    with open(p, "wb") as f:
        f.write(open(good, "rb").read().replace(b"element vertex 30\n", b"element vertex %d\n" % count))
    rc, out = run(shim, p)
    assert rc == 1, out


def test_garbage_headers(shim, tmp_path):
    p = str(tmp_path / "g.ply")
    for data in [b"", b"ply", b"plx\n", b"ply\nformat binary_big_endian 1.0\nend_header\n", b"ply\nformat ascii 1.0\nproperty float x\nend_header\n",
                 b"ply\nformat ascii 1.0\nelement vertex -3\nend_header\n", b"ply\nformat ascii 1.0\nelement vertex 1\nproperty quux x\nend_header\n",
                 b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nend_header\n0 0 0\n",
                 b"ply\nformat ascii 1.0\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n3 0 0 0\n",
                 b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list float int vertex_indices\nend_header\n",
                 b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\n"
                 b"end_header\n0 0 zero\n3 0 0 0\n",
                 b"ply\nformat ascii 1.0\nelement vertex 99999999999999999999999\nend_header\n", b"ply\n" + bytes(range(256)) * 8]:
        with open(p, "wb") as f:
            f.write(data)
        rc, out = run(shim, p)
        assert rc == 1, (data[:60], out)

"""The numpy reference of hcmvs_sample_mesh (tests/mesh_sample_ref.py) against the rule of Mesh::SamplePoints (Mesh.cpp:3444-3527) and
against what a uniform sample must look like, with fixed seeds; and the PLY mesh files of mvsio.  No GPU."""
import importlib
import math

import numpy as np
import pytest

import mesh_sample_ref as MR

mvsio = importlib.import_module("hc-mvs_amd.mvsio")
SEEDS = [1, 2, 3, 7, 11]


def random_triangles(n, seed, scale=1.0):
    r = np.random.default_rng(seed)
    V = (r.standard_normal((3 * n, 3)) * scale).astype(np.float32)
    return V, np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def test_the_draws_are_the_stated_construction():
    """splitmix64's first outputs from state 0 (the published test vector), and one draw spelled out with Python integers"""
    M = (1 << 64) - 1
    assert int(MR.mix(0)) == 0xE220A8397B1DCDAF and int(MR.mix(0x9E3779B97F4A7C15)) == 0x6E789E6AA1B965F4

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    for s, f, k in [(0, 0, 0), (7, 5, 3), (M, 123456789, 1 << 40), (11, (1 << 32) - 2, 141001)]:
        z = mix((mix(s ^ mix(f)) + k * 0xD1B54A32D192ED03) & M)
        u = float(MR.draw(s, np.uint64(f), np.uint64(k)))
        assert u == (z >> 11) * 2.0 ** -53 and 0.0 <= u < 1.0


@pytest.mark.parametrize("seed", SEEDS)
def test_counts_and_points_follow_the_rule(seed):
    V, Fc = random_triangles(300, seed)
    out = MR.sample_mesh(V, Fc, 37.5, seed)
    _, area_d = MR.face_areas(V, Fc)
    fl = np.floor(area_d * 37.5).astype(np.uint64)
    assert np.all((out["counts"] == fl) | (out["counts"] == fl + 1)) and (out["counts"] == fl).any() and (out["counts"] == fl + 1).any()
    assert len(out["xyz"]) == out["counts"].sum() and np.array_equal(out["face"], np.repeat(np.arange(300), out["counts"].astype(np.int64)))
    x, y = out["x"], out["y"]
    assert x.min() >= 0 and y.min() >= 0 and x.max() <= 1 and y.max() <= 1 and (x + y).max() <= 1
    # every point reconstructs from its face: solve P = O + x u + y v in double and compare with the barycentrics it was made from
    O, u, v = (a.astype(np.float64)[out["face"]] for a in MR.edges(V, Fc))
    P = out["xyz"].astype(np.float64) - O
    uu, uv, vv, pu, pv = (u * u).sum(1), (u * v).sum(1), (v * v).sum(1), (P * u).sum(1), (P * v).sum(1)
    det = uu * vv - uv * uv
    bx, by = (pu * vv - pv * uv) / det, (pv * uu - pu * uv) / det
    ok = det > 1e-3 * uu * vv  # well-shaped faces: float32 rounding of the point stays far below the tolerance
    assert ok.mean() > 0.9
    assert np.abs(bx - x)[ok].max() < 1e-3 and np.abs(by - y)[ok].max() < 1e-3
    assert bx[ok].min() > -1e-3 and by[ok].min() > -1e-3 and (bx + by)[ok].max() < 1 + 1e-3


@pytest.mark.parametrize("seed", SEEDS)
def test_negative_form_hits_the_number_of_points(seed):
    V, Fc = random_triangles(1000, 100 + seed)
    N = 20000
    out = MR.sample_mesh(V, Fc, -N, seed)
    area_f, area_d = MR.face_areas(V, Fc)
    assert out["area"] == MR.total_area(area_f) and out["density"] == N / out["area"]
    fp = area_d * out["density"]
    frac = fp - np.floor(fp)
    # the floors are fixed, every face adds a Bernoulli(frac) point: variance sum frac (1 - frac)
    n = len(out["xyz"])
    assert abs(n - N) <= 6 * math.sqrt((frac * (1 - frac)).sum()), (n, N)
    for b in (out["x"], out["y"]):  # a uniform point of the triangle: mean 1/3, variance 1/18
        assert abs(b.mean() - 1 / 3) <= 6 * math.sqrt(1 / (18 * n))


@pytest.mark.parametrize("seed", SEEDS)
def test_points_are_uniform_on_one_triangle(seed):
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    out = MR.sample_mesh(V, [[0, 1, 2]], -200000, seed)
    n = len(out["xyz"])
    assert abs(n - 200000) <= 1
    x, y = out["x"], out["y"]
    # the four congruent sub-triangles the midpoints cut
    cls = np.where(x >= 0.5, 0, np.where(y >= 0.5, 1, np.where(x + y <= 0.5, 2, 3)))
    obs = np.bincount(cls, minlength=4)
    chi2 = ((obs - n / 4) ** 2 / (n / 4)).sum()
    assert chi2 < 16.27, (chi2, obs)  # 0.999 quantile, 3 degrees of freedom


def test_zero_area_and_tiny_meshes():
    V = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], np.float32)
    out = MR.sample_mesh(V, [[0, 0, 3], [0, 1, 2], [0, 1, 3]], 1000.0, 5)
    assert list(out["counts"][:2]) == [0, 0] and out["counts"][2] in (500, 501)
    tiny = MR.sample_mesh(V * np.float32(1e-3), [[0, 1, 3]], -100, 5)  # area 5e-7 < ZEROTOLERANCE<float>(): an empty cloud
    assert len(tiny["xyz"]) == 0 and tiny["area"] < MR.ZEROTOLERANCE_F
    assert len(MR.sample_mesh(V * np.float32(0.02), [[0, 1, 3]], -100, 5)["xyz"]) in (99, 100, 101)  # area 2e-4: sampled


def test_texture_sample_is_the_bilinear_form_with_clamped_pixels():
    tex = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3) * 4
    px = np.array([0.0, 1.5, 4.0, 5.0, 2.25], np.float32); py = np.array([0.0, 2.5, 3.0, 4.0, 0.5], np.float32)
    got = MR.sample_texture(tex, px, py)
    assert np.array_equal(got[0], tex[0, 0]) and np.array_equal(got[2], tex[3, 4]) and np.array_equal(got[3], tex[3, 4])
    t = tex.astype(np.float64)
    want = 0.25 * (t[2, 1] + t[2, 2] + t[3, 1] + t[3, 2])
    assert np.abs(got[1] - want).max() <= 2  # each of the three truncations back to 8 bits loses less than one
    want = 0.5 * (0.75 * t[0, 2] + 0.25 * t[0, 3]) + 0.5 * (0.75 * t[1, 2] + 0.25 * t[1, 3])
    assert np.abs(got[4] - want).max() <= 4


@pytest.mark.parametrize("ascii", [False, True], ids=["binary", "ascii"])
@pytest.mark.parametrize("textured", [False, True], ids=["plain", "textured"])
def test_ply_mesh_round_trip(tmp_path, ascii, textured):
    r = np.random.default_rng(3)
    V = (r.standard_normal((40, 3)) * 1e3).astype(np.float32)
    V[0] = [np.float32(1 / 3), np.float32(-1e-30), np.float32(16777217.0)]
    Fc = r.integers(0, 40, (70, 3)).astype(np.uint32)
    T = r.random((70, 3, 2)).astype(np.float32) if textured else None
    path = str(tmp_path / "mesh.ply")
    mvsio.write_ply_mesh(path, V, Fc, texcoords=T, texture_file="tex 1.ppm" if textured else None, ascii=ascii)
    m = mvsio.read_ply_mesh(path)
    assert m["vertices"].dtype == np.float32 and m["faces"].dtype == np.uint32
    assert np.array_equal(m["vertices"], V) and np.array_equal(m["faces"], Fc)
    if textured:
        assert np.array_equal(m["texcoords"], T) and m["texture_file"] == "tex 1.ppm"
    else:
        assert m["texcoords"] is None and m["texture_file"] is None
    # the other spellings a mesh file comes in
    mvsio.write_ply_mesh(path, V, Fc, texcoords=T, ascii=ascii, index_type="uint", list_name="vertex_index")
    m = mvsio.read_ply_mesh(path)
    assert np.array_equal(m["vertices"], V) and np.array_equal(m["faces"], Fc)

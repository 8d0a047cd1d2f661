"""hcmvs_sample_mesh (mesh_kernels.hip: one thread per face, a scan of the counts, one thread per point) against the numpy restatement
of Mesh::SamplePoints with the counter-based draws of DESIGN.md section 5, D11 (tests/mesh_sample_ref.py, itself checked on the CPU by
tests/test_mesh_sample_ref.py): positions, face indices, counts and colours bit for bit."""
import importlib

import numpy as np
import pytest

import mesh_sample_ref as MR

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")

QUAD_V = np.array([[0, 0, 0], [2, 0, 0], [2, 1.5, 0.25], [0, 1.5, 0.25]], np.float32)
QUAD_F = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def mixed_mesh():
    """1500 faces around (1000, -1000, 1000): 1496 ordinary ones (about 50 points each at density 2000), face 3 with a repeated vertex,
    face 700 collinear, faces 100-139 so small that area * density < 1, face 1201 large enough for more than 70 000 points"""
    r = np.random.default_rng(12)
    n = 1500
    centre = np.array([1000.0, -1000.0, 1000.0]) + r.uniform(-5, 5, (n, 1, 3))
    V = centre + r.uniform(-0.2, 0.2, (n, 3, 3))
    V[100:140] = centre[100:140] + r.uniform(-0.01, 0.01, (40, 3, 3))
    V[1201] = centre[1201] + np.array([[0, 0, 0], [9.0, 0, 0.5], [0.5, 8.5, 0]])
    V = V.reshape(-1, 3).astype(np.float32)
    Fc = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    Fc[3] = [9, 10, 9]
    V[3 * 700 + 2] = V[3 * 700] + (V[3 * 700 + 1] - V[3 * 700]) * np.float32(2)  # exactly on the line: the float32 cross product is 0
    return V, Fc


@pytest.fixture(scope="module")
def mixed():
    V, Fc = mixed_mesh()
    return V, Fc, MR.sample_mesh(V, Fc, 2000.0, 9)


def same_cloud(got, want):
    xyz, fid, bgr, st = got
    assert st["n_points"] == len(want["xyz"]) == len(xyz)
    assert np.array_equal(fid, want["face"])
    assert np.array_equal(xyz.view(np.uint32), want["xyz"].view(np.uint32))
    assert st["area"] == want["area"] and st["density"] == want["density"]
    if want["bgr"] is not None:
        assert np.array_equal(bgr, want["bgr"])


def test_quad(ctx):
    want = MR.sample_mesh(QUAD_V, QUAD_F, 1650.0, 4)
    assert 4500 < len(want["xyz"]) < 5500
    got = ctx.sample_mesh(QUAD_V, QUAD_F, 1650.0, seed=4)
    same_cloud(got, want)
    assert got[2] is None and got[3]["n_faces"] == 2 and got[3]["n_zero_area_faces"] == 0 and got[3]["device_bytes"] > 0


def test_mixed_mesh(ctx, mixed):
    V, Fc, want = mixed
    c = want["counts"]
    assert 140000 < len(want["xyz"]) < 160000
    assert c[3] == 0 and c[700] == 0 and c[1201] > 70000 and c[100:140].max() <= 1 and c[100:140].min() == 0
    _, area_d = MR.face_areas(V, Fc)
    assert area_d[3] == 0 and area_d[700] == 0 and (area_d[100:140] * 2000 < 1).all() and (area_d[100:140] > 0).all()
    got = ctx.sample_mesh(V, Fc, 2000.0, seed=9)
    same_cloud(got, want)
    assert got[3]["n_zero_area_faces"] == 2 and got[3]["n_faces"] == 1500


def test_negative_form(ctx, mixed):
    V, Fc, _ = mixed
    want = MR.sample_mesh(V, Fc, -30000, 21)
    assert abs(len(want["xyz"]) - 30000) < 300
    same_cloud(ctx.sample_mesh(V, Fc, -30000, seed=21), want)
    # half a point rounds up (ROUND2INT, in float): -4999.5 asks for 5000 points, and -8388609 (odd, above 2^23, where x + .5f ties to even)
    # for 8388610, as the reference's Round2Int(float) does
    assert MR.density_of(QUAD_V, QUAD_F, -8388609.0)[0] == 8388610 / MR.total_area(MR.face_areas(QUAD_V, QUAD_F)[0])
    st = ctx.sample_mesh(QUAD_V, QUAD_F, -8388609.0, seed=2, count_only=True)[3]
    assert st["density"] == MR.density_of(QUAD_V, QUAD_F, -8388609.0)[0] and abs(st["n_points"] - 8388610) <= 6
    same_cloud(ctx.sample_mesh(QUAD_V, QUAD_F, -4999.5, seed=2), MR.sample_mesh(QUAD_V, QUAD_F, -4999.5, 2))
    assert MR.sample_mesh(QUAD_V, QUAD_F, -4999.5, 2)["density"] == 5000 / MR.sample_mesh(QUAD_V, QUAD_F, -5000, 2)["area"]
    # total area below ZEROTOLERANCE<float>(): an empty cloud, and success
    tiny = QUAD_V * np.float32(0.004)
    assert 0 < MR.total_area(MR.face_areas(tiny, QUAD_F)[0]) < MR.ZEROTOLERANCE_F
    xyz, fid, bgr, st = ctx.sample_mesh(tiny, QUAD_F, -1000, seed=1)
    assert len(xyz) == 0 and len(fid) == 0 and st["n_points"] == 0 and st["area"] == MR.total_area(MR.face_areas(tiny, QUAD_F)[0])
    assert len(ctx.sample_mesh(tiny, QUAD_F, 1e-3, seed=1)[0]) == 0  # a density that leaves no point: zero points is success too


def test_count_only_capacity_and_seeds(ctx):
    import ctypes as C
    a = ctx.sample_mesh(QUAD_V, QUAD_F, 1650.0, seed=4)
    none = ctx.sample_mesh(QUAD_V, QUAD_F, 1650.0, seed=4, count_only=True)
    assert none[0] is None and none[3]["n_points"] == len(a[0])
    b = ctx.sample_mesh(QUAD_V, QUAD_F, 1650.0, seed=4)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = ctx.sample_mesh(QUAD_V, QUAD_F, 1650.0, seed=5)
    assert len(c[0]) != len(a[0]) or not np.array_equal(c[0], a[0])
    assert not np.array_equal(c[0][:1000], a[0][:1000])
    # too small a capacity: refused, and the size needed comes back
    n = C.c_uint64(0)
    need = len(a[0])
    xyz = np.full((need, 3), 7, np.float32)
    fp, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = binding.lib().hcmvs_sample_mesh(ctx._h, 4, QUAD_V.ctypes.data_as(fp), 2, QUAD_F.ctypes.data_as(u32), None, None, 0, 0, C.c_float(1650.0), 4, need - 1,
                                         xyz.ctypes.data_as(fp), None, None, C.byref(n), None)
    assert rc == binding.ERR_INVALID and n.value == need and (xyz == 7).all()
    assert b"needed" in binding.lib().hcmvs_last_error(ctx._h)
    rc = binding.lib().hcmvs_sample_mesh(ctx._h, 4, QUAD_V.ctypes.data_as(fp), 2, QUAD_F.ctypes.data_as(u32), None, None, 0, 0, C.c_float(1650.0), 4, need,
                                         xyz.ctypes.data_as(fp), None, None, C.byref(n), None)
    assert rc == binding.OK and n.value == need and np.array_equal(xyz, a[0])
    # a cloud of 2^32 points or more is refused (the reference's unsigned would wrap), in the counting call already
    with pytest.raises(binding.HcmvsError) as e:
        ctx.sample_mesh(QUAD_V, QUAD_F, 2e9, seed=4, count_only=True)
    assert e.value.code == binding.ERR_INVALID and "2^32 points or more" in str(e.value)
    with pytest.raises(binding.HcmvsError) as e:
        ctx.sample_mesh(QUAD_V, QUAD_F, 3e38, seed=4)  # more than 2^32 on one face
    assert e.value.code == binding.ERR_INVALID and "2^32 points or more" in str(e.value)
    assert ctx.sample_mesh(QUAD_V, QUAD_F, 1650.0, seed=4)[0].tobytes() == a[0].tobytes()


def test_refused_inputs(ctx):
    tex = np.zeros((8, 8, 3), np.uint8); tc = np.zeros((2, 3, 2), np.float32)
    bad_v = QUAD_V.copy(); bad_v[2, 1] = np.nan
    inf_v = QUAD_V.copy(); inf_v[3, 0] = -np.inf
    bad_f = QUAD_F.copy(); bad_f[1, 2] = 4
    nan_tc = tc.copy(); nan_tc[1, 2, 0] = np.nan
    cases = [(dict(vertices=bad_v), "vertex 2"), (dict(vertices=inf_v), "vertex 3"), (dict(faces=bad_f), "face 1 names vertex 4 of 4"),
             (dict(faces=np.zeros((0, 3), np.uint32)), "no faces"), (dict(sample=0.0), "sample"), (dict(sample=float("nan")), "sample"),
             (dict(texture_bgr=tex), "without texture coordinates"), (dict(texcoords=tc), "without a texture"),
             (dict(texcoords=nan_tc, texture_bgr=tex), "face 1")]
    for kw, needle in cases:
        args = dict(vertices=QUAD_V, faces=QUAD_F, sample=1650.0, seed=4)
        args.update(kw)
        with pytest.raises(binding.HcmvsError) as e:
            ctx.sample_mesh(**args)
        assert e.value.code == binding.ERR_INVALID and needle in str(e.value), (needle, str(e.value))
    # the context is still usable
    same_cloud(ctx.sample_mesh(QUAD_V, QUAD_F, 1650.0, seed=4), MR.sample_mesh(QUAD_V, QUAD_F, 1650.0, 4))


def test_textured(ctx):
    r = np.random.default_rng(5)
    tex = r.integers(0, 256, (8, 8, 3)).astype(np.uint8)
    # the quad spans the whole texture, corners at exactly 0 and 1: samples reach all four borders; two more faces inside it
    V = np.concatenate([QUAD_V, QUAD_V + np.float32(3)])
    Fc = np.concatenate([QUAD_F, QUAD_F + 4]).astype(np.uint32)
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    tc = np.concatenate([uv[QUAD_F], (uv * np.float32(0.37) + np.float32(0.21))[QUAD_F]]).astype(np.float32)
    want = MR.sample_mesh(V, Fc, 900.0, 3, texcoords=tc, texture_bgr=tex)
    assert 5000 < len(want["xyz"]) < 6000 and len(np.unique(want["bgr"], axis=0)) > 1000
    got = ctx.sample_mesh(V, Fc, 900.0, seed=3, texcoords=tc, texture_bgr=tex)
    same_cloud(got, want)
    # a face whose three corners sit on one texel corner: every point gets that border pixel (coordinate = width: clamped)
    corner = np.ones((1, 3, 2), np.float32) * np.array([1, 0], np.float32)
    xyz, fid, bgr, _ = ctx.sample_mesh(QUAD_V, QUAD_F[:1], 100.0, seed=3, texcoords=corner, texture_bgr=tex)
    assert len(bgr) > 100 and (bgr == tex[7, 7]).all()
    # texture coordinates far outside [0, 1], where D11 defines what the reference's casts leave undefined: sample positions below zero
    # and beyond int32 (saturated, pixel clamped), weights whose products leave [0, 256) (the low byte of the saturated int) and, with
    # coordinates near the float range, infinite positions whose weights make NaN products (0)
    far = np.array([[[-3, -2.5], [4.75, 0.5], [0.25, 7]], [[1e12, -1e12], [0.5, 0.5], [-1e12, 3e9]], [[3e38, -3e38], [-3e38, 0.25], [0.5, 3e38]]], np.float32)
    Ff = np.array([[0, 1, 2], [0, 2, 3], [1, 2, 3]], np.uint32)
    want = MR.sample_mesh(QUAD_V, Ff, 700.0, 6, texcoords=far, texture_bgr=tex)
    assert len(want["xyz"]) > 2500 and len(np.unique(want["bgr"][want["face"] == 0], axis=0)) > 100 and all((want["face"] == f).sum() > 500 for f in range(3))
    same_cloud(ctx.sample_mesh(QUAD_V, Ff, 700.0, seed=6, texcoords=far, texture_bgr=tex), want)
    # a non-square texture: width and height are not mixed up
    tex2 = r.integers(0, 256, (5, 11, 3)).astype(np.uint8)
    same_cloud(ctx.sample_mesh(V, Fc, 200.0, seed=8, texcoords=tc, texture_bgr=tex2), MR.sample_mesh(V, Fc, 200.0, 8, texcoords=tc, texture_bgr=tex2))

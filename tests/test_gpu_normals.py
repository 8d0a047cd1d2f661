"""hcmvs_estimate_point_normals (cloud_kernels.hip: exact k-nearest search through a Morton-sorted grid and an octree climb, then a
double-precision Jacobi PCA, then the flip towards the first view) against the brute-force float64 reference of tests/normals_ref.py, on
the clouds of tests/normals_clouds.py: EVERY point the reference does not exclude, to 2^-23 per component, sign included.

The tolerance: both sides are float32 roundings of float64 unit vectors that, under the conditioning mask, differ by about
eps * l2 / (l1 - l0) <= 2.2e-12; two such values round at most one float32 ulp apart, <= 2^-24 below 1; the factor 2 is margin.  What
the masks exclude and why is in normals_ref.py; that they exclude next to nothing on these clouds, and that one wrong neighbour moves the
reference by more than 100 times the tolerance, is checked on the CPU in test_normals_ref.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import normals_clouds as NC

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    K = np.array([[20.0, 0, 7.5], [0, 20.0, 7.5], [0, 0, 1]])
    for i, centre in enumerate(NC.CENTRES):                  # only the centres are read
        c.upload_view(i, np.zeros((16, 16), np.float32), K, np.eye(3), centre)
    yield c
    c.close()


def normals(ctx, xyz, first, k):
    return ctx.estimate_point_normals(xyz, np.ones(len(xyz), np.uint32), first, k)


def assert_finite_unit(gn):
    assert np.isfinite(gn).all()
    assert np.abs(np.linalg.norm(gn.astype(np.float64), axis=1) - 1).max() < 1e-6


def compare(name, k, gn):
    """every comparable point within 2^-23; every point finite and of unit length.  Returns the number of points compared"""
    ref = NC.reference(name, k)
    assert_finite_unit(gn)
    ok = NC.comparable(ref)
    diff = np.abs(gn.astype(np.float64) - ref["normal"].astype(np.float64)).max(1)
    worst = int(np.argmax(np.where(ok, diff, -1))) if ok.any() else -1
    print("normals %s k=%d: n=%d compared=%d near_tie=%d ill_conditioned=%d grazing=%d max diff=%.3g (2^-23 = %.3g), above: %d" % (
        name, k, len(gn), ok.sum(), ref["near_tie"].sum(), ref["ill_conditioned"].sum(), ref["grazing"].sum(),
        diff[ok].max() if ok.any() else 0.0, NC.TOL, (diff[ok] > NC.TOL).sum()))
    assert (diff[ok] <= NC.TOL).all(), "%d of %d points differ, worst point %d: device %s reference %s" % (
        (diff[ok] > NC.TOL).sum(), ok.sum(), worst, gn[worst], ref["normal"][worst])
    return int(ok.sum())


COMPARED = [(name, k) for name, k in NC.CASES if name not in ("h", "i1", "i2")]


@pytest.mark.parametrize("name,k", COMPARED)
def test_normals_equal_the_reference(ctx, name, k):
    """a: the sheet at k on both sides of the two kernel instances (<= 16, <= 32); b: outliers and a far cluster of five (the climb over
    several levels, fewer than k candidates in the low ones, blocks cut at the faces of the grid); c: a dense patch beside a sparse one;
    d, d2: the whole sheet in one cell, a lone point that climbs to the top (d2: with the cell enlarged to keep 20 bits per axis); e: exact
    ties at the k-th distance, decided by the original index; f: 100 copies of one point; g: a flat box; i<n>: n = k - 1, k, k + 1 points"""
    xyz, first = NC.cloud(name)
    gn = normals(ctx, xyz, first, k)
    compared = compare(name, k, gn)
    n = len(xyz)
    assert compared >= n - 1 - int(NC.CAP_ILL * n)
    if name == "g":                                          # the plane z = 0.5 seen from above
        assert np.abs(gn - np.array([0, 0, 1], np.float32)).max() <= NC.TOL


def test_order_independence(ctx):
    """the sheet in another input order: the same normals, bit for bit, at the permuted places.  No point of it has two equal distances
    among its k + 1 nearest (test_normals_ref.py), so neighbours are summed in the order of their distances whatever their indices: pins
    the sort, the index <-> position maps and the scatter of the results"""
    xyz, first = NC.cloud("a")
    perm = np.random.RandomState(11).permutation(len(xyz))
    assert (perm != np.arange(len(xyz))).mean() > 0.99
    for k in (3, 16, 32):
        gn = normals(ctx, xyz, first, k)
        gp = normals(ctx, xyz[perm], first[perm], k)
        assert np.array_equal(gp.view(np.uint32), gn[perm].view(np.uint32)), k
        assert np.array_equal(normals(ctx, xyz, first, k).view(np.uint32), gn.view(np.uint32))   # and the same twice


def test_collinear(ctx):
    """500 exactly collinear points: no plane is determined; a finite unit normal, perpendicular to the line"""
    xyz, first = NC.cloud("h")
    gn = normals(ctx, xyz, first, 8)
    assert_finite_unit(gn)
    assert np.abs(gn.astype(np.float64) @ NC.LINE_DIR).max() < 1e-6


@pytest.mark.parametrize("k", NC.TINY_K)
def test_one_and_two_points(ctx, k):
    xyz, first = NC.cloud("i1")
    assert_finite_unit(normals(ctx, xyz, first, k))
    xyz, first = NC.cloud("i2")
    gn = normals(ctx, xyz, first, k)
    assert_finite_unit(gn)
    d = xyz[1].astype(np.float64) - xyz[0].astype(np.float64)
    assert np.abs(gn.astype(np.float64) @ (d / np.linalg.norm(d))).max() < 1e-6


def test_refusals(ctx):
    xyz, first = NC.cloud("i17")
    ones = np.ones(len(xyz), np.uint32)

    def refused(x, nv, vi, k, word):
        with pytest.raises(binding.HcmvsError) as e:
            ctx.estimate_point_normals(x, nv, vi, k)
        assert e.value.code == binding.ERR_INVALID and word in str(e.value), str(e.value)

    refused(xyz, ones, first, 2, "3 <= k <= 32")
    refused(xyz, ones, first, 33, "3 <= k <= 32")
    nv = ones.copy(); nv[6] = 0
    refused(xyz, nv, np.delete(first, 6), 16, "point 6 has no view")
    vi = first.copy(); vi[4] = 9
    refused(xyz, ones, vi, 16, "unknown view 9")
    # a coordinate that is not finite never reaches the device: refused on the host, naming the first such point
    for bad in (np.nan, np.inf, -np.inf):
        for q in range(3):
            x = xyz.copy(); x[5, q] = bad; x[11, 0] = np.nan
            refused(x, ones, first, 16, "point 5 ")
    # no points: success, and the output is not written
    out = np.full(3, 7.0, np.float32)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = binding.lib().hcmvs_estimate_point_normals(ctx._h, 0, xyz.ctypes.data_as(f32p), ones.ctypes.data_as(u32p), first.ctypes.data_as(u32p),
                                                    16, out.ctypes.data_as(f32p))
    assert rc == binding.OK and (out == 7.0).all()
    # the context is as good as before
    compare("i17", 16, normals(ctx, xyz, first, 16))

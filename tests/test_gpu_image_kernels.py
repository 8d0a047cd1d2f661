"""The small kernels that prepare a view's image, pinned at their branches through the C-ABI: resize_area_fast_kernel,
resize_area_kernel and resize_cubic_kernel (hcmvs_rescale_view), gray_to_u8_kernel, bgr_to_u8_kernel and gradient_kernel
(hcmvs_get_gradient_map), point_colors_kernel (hcmvs_estimate_point_colors).

Every device result is compared twice: with the CPU oracle, bit for bit, and with the plain numpy statement of image_ref.py -- equal
for the integer kernels, inside the derived float32 bound (T + 2) * 2**-24 * mag64 for the resizes (test_image_ref.py holds the oracle
to the same statements on the CPU).  All pixels are compared: nothing is sampled or masked.  The inputs are image_cases.py's; each
test asserts on its own input, with numpy, that the branch it is named for is reached.

Not tested: |g * 255| of 2**31 and more in the 8-bit conversion.  There OpenCV's saturate_cast, the oracle's (int)lrintf and the
device's cast are three different things, and no image gets there: every input here stays far below."""
import importlib

import numpy as np
import pytest

import image_cases as IC
import image_ref as IR
import oracle_lib as O

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")

F32 = np.float32
K0 = np.array([[120.0, 0, 64.5], [0, 118.0, 47.0], [0, 0, 1]])


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


# ---- D1: hcmvs_rescale_view -----------------------------------------------------------------------------

def check_rescale(ctx, g, scale, path, dsize=None):
    h, w = g.shape
    out, mag, T, p = IR.resize_gray(g, scale)
    assert p == path and (dsize is None or out.shape == dsize)                   # the case is on the branch it is named for
    ctx.upload_view(0, g, K0, np.eye(3), np.zeros(3))
    got, K2 = ctx.rescale_view(0, 1, scale)
    want = O.resize_gray(g, scale)
    assert got.shape == want.shape == out.shape
    err, bound = np.abs(got.astype(np.float64) - out), IR.resize_bound(mag, T)
    print("rescale %dx%d @ %g (%s): T %d, worst |device - out64| / bound %.3f, device == oracle on %d of %d pixels"
          % (h, w, scale, path, T, (err / np.maximum(bound, 1e-300)).max(), (got == want).sum(), got.size))
    assert np.array_equal(got, want)
    assert (err <= bound).all()
    f = max(got.shape) / max(w, h)                                               # Image::GetCamera: normalised K times max(w', h')
    assert np.allclose(K2, np.array([[120.0 * f, 0, 64.5 * f], [0, 118.0 * f, 47.0 * f], [0, 0, 1]]), rtol=1e-12)


@pytest.mark.parametrize("case", IC.RESIZE_CASES, ids=IC.case_id)
def test_rescale_matches_oracle_and_statement(ctx, case):
    h, w, scale, path, dsize = case
    check_rescale(ctx, IC.noise_image(h, w, scale), scale, path, dsize)


@pytest.mark.parametrize("case", IC.IMPULSE_CASES, ids=IC.case_id)
def test_rescale_impulses(ctx, case):
    h, w, scale, path = case
    g = IC.impulse_image(h, w)
    mag = IR.resize_gray(g, scale)[1]
    assert (mag > 0).sum() >= 4 and (mag == 0).any()                             # isolated responses: a tap off by one shows
    check_rescale(ctx, g, scale, path)


def test_scale_within_15_percent_is_refused(ctx):
    ctx.upload_view(0, np.zeros((64, 64), F32), np.eye(3), np.eye(3), np.zeros(3))
    for s in IC.REFUSED_SCALES:
        assert abs(F32(s) - F32(1)) < F32(0.15)
        with pytest.raises(binding.HcmvsError):
            ctx.rescale_view(0, 1, s)


# ---- D2: the 8-bit conversion and the gradient map ------------------------------------------------------

SIZES = pytest.mark.parametrize("size", IC.GRADIENT_SIZES, ids=lambda s: "%dx%d" % s)


def device_gradient(ctx, gray, bgr=None):
    ctx.upload_view(2, gray, K0, np.eye(3), np.zeros(3), bgr=bgr)
    return ctx.gradient_map(2)


def check_gradient_of_gray(ctx, g):
    g8 = IR.gray_to_u8(g)
    got = device_gradient(ctx, g)
    assert np.array_equal(got, O.gradient_map(g))
    assert np.array_equal(got, IR.gradient_u8(g8))
    return g8


@SIZES
def test_gradient_noise_saturates_and_rounds_both_ways(ctx, size):
    g = IC.gradient_noise(*size)
    assert ((g < 0) | (g > 1)).sum() > 0 and np.abs(g).max() * 255 < 2 ** 31     # out of range: the conversion saturates
    b = IR.gradient_branches(check_gradient_of_gray(ctx, g))
    assert b["clamped"] > 0 and b["up"] > 0 and b["down"] > 0


@SIZES
def test_gradient_ties_of_the_conversion(ctx, size):
    g, tie, k = IC.gradient_ties(*size)
    p = (g * F32(255)).astype(np.float64)
    assert tie.sum() > 0 and np.array_equal(p[tie], k[tie] + 0.5) and (k[tie] % 2 == 0).any() and (k[tie] % 2 == 1).any()
    g8 = check_gradient_of_gray(ctx, g)
    ax, ay = IR.sobel_abs(g8)
    assert ax.max() < 255 and ay.max() < 255                                     # unsaturated: a tie rounded the wrong way changes the map
    assert np.array_equal(g8[tie], (k + (k & 1))[tie])


@SIZES
def test_gradient_blocks(ctx, size):
    b = IR.gradient_branches(check_gradient_of_gray(ctx, IC.gradient_blocks(*size)))
    assert b["clamped"] > 0 and b["up"] > 0


@SIZES
def test_gradient_constant(ctx, size):
    g8 = check_gradient_of_gray(ctx, np.full(size, 0.3, F32))
    assert not IR.gradient_u8(g8).any()                                          # the reflected border adds nothing


@SIZES
def test_gradient_from_colour(ctx, size):
    """(e) a fuse-only view (no gray image) and (f) a view with both: the gradient comes from the colour image (ensure_gradient)"""
    bgr = IC.gradient_bgr(*size)
    b8 = IR.bgr_to_u8(bgr)
    want = IR.gradient_u8(b8)
    assert np.array_equal(O.gradient_u8(O.bgr2gray_u8(bgr)), want)
    b = IR.gradient_branches(b8)
    assert b["clamped"] > 0 and b["up"] > 0 and b["down"] > 0
    assert np.array_equal(device_gradient(ctx, None, bgr), want)
    other = IC.gradient_noise(*size)
    assert not np.array_equal(IR.gradient_u8(IR.gray_to_u8(other)), want)
    assert np.array_equal(device_gradient(ctx, other, bgr), want)


# ---- D3: hcmvs_estimate_point_colors --------------------------------------------------------------------

def test_point_colors_match_oracle_and_statement(ctx):
    views = IC.color_views()
    xyz, nv, ids, tags = IC.color_points(views)
    detail = []
    want = IR.point_colors(views, xyz, nv, ids, detail)
    IC.check_color_scene(views, tags, detail, want)
    for i, v in enumerate(views):
        ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"], bgr=v["bgr"])
    got = ctx.estimate_point_colors(xyz, nv, ids)
    maps = [dict(K=v["K"], R=v["R"], C=v["C"], depth=np.zeros((v["h"], v["w"]), F32), conf=np.zeros((v["h"], v["w"]), F32), bgr=v["bgr"],
                 neighbors=[]) for v in views]
    ora = O.estimate_point_colors(maps, xyz, nv, ids)
    for name, ref in (("oracle", ora), ("statement", want)):
        bad = np.flatnonzero((got != ref).any(1))
        assert len(bad) == 0, (name, [(int(i), tags[i], got[i].tolist(), ref[i].tolist()) for i in bad[:5]])

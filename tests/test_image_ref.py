"""The CPU oracle's image pieces (hcor_resize_gray, hcor_gray_f32_to_u8, hcor_bgr2gray_u8, hcor_gradient_map,
hcor_estimate_point_colors) against the plain numpy statements of image_ref.py, over the case tables the device tests use
(image_cases.py), and literal known answers that keep the numpy statements themselves honest.

The integer kernels must be EQUAL.  A resize is a float32 sum of products against the float64 sum of the same products: per pixel
|oracle - out64| <= (T + 2) * 2**-24 * mag64, the standard bound of a length-T sum (T = the terms of the largest table product for
INTER_AREA, 16 for INTER_CUBIC; mag64 = the same sum over absolute values).  The bound is derived, not measured."""
import numpy as np
import pytest

import image_cases as IC
import image_ref as IR
import oracle_lib as O

F32 = np.float32


# ---- known answers of the numpy statements ---------------------------------------------------------------

def test_known_answers_area():
    blk = np.tile(np.array([[1, 2], [3, 4]], F32), (8, 8))                       # a 2 x 2 block: every mean is 2.5
    out, mag, taps, path = IR.resize_area(blk, 0.5)
    assert path == "fast" and taps == 4 and out.shape == (8, 8) and np.array_equal(out, np.full((8, 8), 2.5)) and np.array_equal(mag, out)
    imp = np.zeros((8, 8), F32); imp[5, 2] = -8                                  # an impulse: one destination pixel, a quarter of it
    out, mag, _, _ = IR.resize_area(imp, 0.5)
    want = np.zeros((4, 4)); want[2, 1] = -2
    assert np.array_equal(out, want) and np.array_equal(mag, -want)
    # factor 1.6 on a ramp: cell 0 = [0, 1.6) = pixel 0 + 0.6 of pixel 1; cell 1 = [1.6, 3.2) = 0.4 of pixel 1 + pixel 2 + 0.2 of pixel 3
    ramp = np.arange(16, dtype=F32).reshape(1, 16).repeat(8, 0)
    out, _, taps, path = IR.resize_area(ramp, 0.625)
    assert path == "general" and out.shape == (5, 10) and taps == 9
    assert out[0, 0] == pytest.approx(0.6 / 1.6, rel=1e-6) and out[0, 1] == pytest.approx((0.4 + 2 + 0.6) / 1.6, rel=1e-6)
    assert np.allclose(out, out[0][None, :], rtol=1e-6)
    # the 1e-3 cut: factor 1 / float32(1 / 3) is 3 - 9e-8; cell d starts d * 9e-8 before pixel 3 d, and that leading sliver is dropped:
    # two whole pixels and a trailing one of all but a sliver, never a fourth entry
    tab = IR.area_tab(78, 26, 1.0 / float(F32(1.0 / 3.0)))
    assert [[s for s, _ in e] for e in tab] == [[3 * d, 3 * d + 1, 3 * d + 2] for d in range(26)]
    # a factor above 16 needs more than 16 entries per axis
    assert max(len(e) for e in IR.area_tab(280, 17, 1.0 / float(F32(0.06)))) == 18


def test_known_answers_cubic():
    # Keys kernel, A = -0.75, t = 0.25 (exact in float32)
    assert IR.cubic_weights(np.array([0.25], F32))[0].tolist() == [-0.10546875, 0.87890625, 0.26171875, -0.03515625]
    assert IR.cubic_weights(np.array([0.0], F32))[0].tolist() == [0, 1, 0, 0]
    imp = np.zeros((9, 9), F32); imp[4, 4] = 1
    out, mag = IR.resize_cubic(imp, 2.0)                                         # destination 9: fx = 4.25 -> taps 3 .. 6, the impulse is tap 1
    assert out.shape == (18, 18) and out[9, 9] == 0.87890625 ** 2 and out[9, 7] == 0.87890625 * 0.26171875 and out[9, 5] == 0.87890625 * -0.03515625
    assert mag[9, 5] == -out[9, 5] and out[9, 2] == 0
    # a ramp: A = -0.75 does not reproduce it; at t = 0.25 the taps -1, 0, 1, 2 weigh to w2 + 2 w3 - w0 = 0.296875, at 0.75 to 0.703125
    ramp = np.tile(np.arange(32, dtype=F32), (16, 1))
    out, _ = IR.resize_cubic(ramp, 2.0)
    fx = (np.arange(64) + 0.5) / 2 - 0.5
    want = np.floor(fx) + np.where(fx - np.floor(fx) == 0.25, 0.296875, 0.703125)
    assert np.array_equal(out[:, 4:-4], np.tile(want[4:-4], (32, 1)))


def test_known_answers_u8_and_gradient():
    assert IR.gray_to_u8(np.array([[-1.0, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.999, 1.0, 7.0]], F32)).tolist() == [[0, 0, 0, 2, 2, 255, 255, 255]]
    assert IR.bgr_to_u8(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30]]], np.uint8)).tolist() == [[255, 0, 29, 150, 76, 22]]
    step = np.zeros((5, 6), np.uint8); step[:, 3:] = 255                         # a vertical edge: |gx| = 1020 -> 255, gy = 0: 127.5 -> 128
    assert IR.gradient_u8(step).tolist() == [[0, 0, 128, 128, 0, 0]] * 5
    g = np.zeros((5, 5), np.uint8); g[2, 2] = 3
    # around a single 3: its diagonal neighbours have |gx| = |gy| = 3, its edge neighbours 6 and 0, itself 0 and 0
    assert IR.gradient_u8(g).tolist() == [[0] * 5, [0, 3, 3, 3, 0], [0, 3, 0, 3, 0], [0, 3, 3, 3, 0], [0] * 5]
    g = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 254]], np.uint8)                  # reflect-101: the corner pixel's neighbours mirror, its own gx = gy = 0
    ax, ay = IR.sobel_abs(g)
    assert ax[2, 2] == 0 and ay[2, 2] == 0 and ax[1, 1] == 254 and ax[2, 1] == 508 and ay[1, 2] == 508
    s = np.arange(0, 511)                                                       # half of a sum, ties to even: as float64's rint does it
    assert np.array_equal((s + ((s >> 1) & 1)) >> 1, np.rint(s / 2.0).astype(int))


def test_known_answers_colors():
    img = np.zeros((4, 4, 3), np.uint8)
    img[1, 1] = (255, 200, 1); img[1, 2] = (0, 100, 255); img[2, 1] = (0, 50, 255); img[2, 2] = (255, 10, 255)
    # x = y = 0.5, channel 0: top = trunc(127.5) + 0 = 127, bottom = 0 + 127, each halved and truncated: 63 + 63; channel 1:
    # (100 + 50) / 2 + (25 + 5) / 2; channel 2: top = 0 + 127, bottom = 127 + 127 -> 63 + 127
    assert IR.sample_u8(img, F32(1.5), F32(1.5)) == [126, 90, 190]
    assert IR.sample_u8(img, F32(1.0), F32(1.0)) == [255, 200, 1] and IR.sample_u8(img, F32(2.0), F32(1.0)) == [0, 100, 255]
    # 255 * 0.25 + 255 * 0.75 truncates to 63 + 191 = 254, not 255
    assert IR.sample_u8(img, F32(1.75), F32(2.0))[2] == 254
    view = dict(K=np.array([[64.0, 0, 2], [0, 64, 2], [0, 0, 1]]), R=np.eye(3), C=np.zeros(3), bgr=img)
    xyz = np.array([[-0.5, -0.5, 64], [-1.0, -1.0, 64], [-1.03125, -1.0, 64], [0, 0, 64], [0.015625, 0, 64]], F32)   # (1.5, 1.5), (1, 1), (0.97, 1), (2, 2), (2.02, 2)
    got = IR.point_colors([view], xyz, [1] * 5, [0] * 5)
    assert got.tolist() == [[126, 90, 190], [255, 200, 1], [255, 255, 255], [255, 10, 255], [255, 255, 255]]


def test_tie_values_are_exact_ties():
    k = np.arange(255)
    t = np.array([IC.tie_value(int(i)) for i in k], F32)
    p = t * F32(255)
    assert p.dtype == np.float32 and np.array_equal(p.astype(np.float64), k + 0.5)
    assert np.array_equal(IR.gray_to_u8(t[None, :])[0], k + (k & 1))             # to even: up for an odd k


# ---- the oracle against the statements -------------------------------------------------------------------

@pytest.mark.parametrize("case", IC.RESIZE_CASES, ids=IC.case_id)
def test_oracle_resize_within_the_bound(case):
    h, w, scale, path, dsize = case
    g = IC.noise_image(h, w, scale)
    out, mag, T, p = IR.resize_gray(g, scale)
    assert p == path and out.shape == dsize                                      # the table cannot drift off its branch
    got = O.resize_gray(g, scale)
    assert got.shape == dsize
    err, bound = np.abs(got.astype(np.float64) - out), IR.resize_bound(mag, T)
    print("resize %s: T %d, worst |oracle - out64| / bound %.3f" % (IC.case_id(case), T, (err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("case", IC.IMPULSE_CASES, ids=IC.case_id)
def test_oracle_resize_impulses(case):
    h, w, scale, path = case
    g = IC.impulse_image(h, w)
    out, mag, T, p = IR.resize_gray(g, scale)
    assert p == path and (mag > 0).sum() >= 4 and (mag == 0).any()
    got = O.resize_gray(g, scale)
    assert (np.abs(got.astype(np.float64) - out) <= IR.resize_bound(mag, T)).all()   # exactly 0 where no tap meets an impulse


def test_case_table_covers_the_launch_edges():
    dh = {c[4][0] for c in IC.AREA_CASES}
    dw = {c[4][1] for c in IC.AREA_CASES if c[3] == "fast"}
    assert {16, 17, 18, 19} <= dh and {63, 64, 65} <= dw


def gradient_inputs(h, w):
    return [IC.gradient_noise(h, w), IC.gradient_ties(h, w)[0], IC.gradient_blocks(h, w), np.full((h, w), 0.3, F32)]


@pytest.mark.parametrize("size", IC.GRADIENT_SIZES + [(37, 81), (5, 7)], ids=lambda s: "%dx%d" % s)
def test_oracle_u8_and_gradient_equal(size):
    h, w = size
    for g in gradient_inputs(h, w):
        g8 = IR.gray_to_u8(g)
        assert np.array_equal(O.gray_f32_to_u8(g), g8)
        assert np.array_equal(O.gradient_u8(g8), IR.gradient_u8(g8))
        assert np.array_equal(O.gradient_map(g), IR.gradient_u8(g8))
    bgr = IC.gradient_bgr(h, w)
    b8 = IR.bgr_to_u8(bgr)
    assert np.array_equal(O.bgr2gray_u8(bgr), b8) and np.array_equal(O.gradient_u8(b8), IR.gradient_u8(b8))


def test_gradient_inputs_reach_their_branches():
    g = IC.gradient_noise(37, 81)
    ax, ay = IR.sobel_abs(IR.gray_to_u8(g))
    assert (ax > 255).sum() > 1000 and (ay > 255).sum() > 1000                   # the noise saturates most of the image
    for h, w in IC.GRADIENT_SIZES:
        g = IC.gradient_noise(h, w)
        b = IR.gradient_branches(IR.gray_to_u8(g))
        assert b["clamped"] > 0 and b["up"] > 0 and b["down"] > 0 and ((g < 0) | (g > 1)).sum() > 0
        g, tie, k = IC.gradient_ties(h, w)
        p = (g * F32(255)).astype(np.float64)
        assert np.array_equal(p[tie], k[tie] + 0.5) and (k[tie] % 2 == 0).any() and (k[tie] % 2 == 1).any()
        ax, ay = IR.sobel_abs(IR.gray_to_u8(g))
        assert ax.max() < 255 and ay.max() < 255                                 # nothing saturates around the ties
        b = IR.gradient_branches(IR.gray_to_u8(IC.gradient_blocks(h, w)))
        assert b["clamped"] > 0 and b["up"] > 0


def test_oracle_point_colors_equal():
    views = IC.color_views()
    xyz, nv, ids, tags = IC.color_points(views)
    detail = []
    want = IR.point_colors(views, xyz, nv, ids, detail)
    maps = [dict(K=v["K"], R=v["R"], C=v["C"], depth=np.zeros((v["h"], v["w"]), F32), conf=np.zeros((v["h"], v["w"]), F32), bgr=v["bgr"],
                 neighbors=[]) for v in views]
    got = O.estimate_point_colors(maps, xyz, nv, ids)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, [(int(i), tags[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    IC.check_color_scene(views, tags, detail, want)

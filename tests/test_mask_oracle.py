"""--ignore-mask-label on the CPU: the label parse and resizeNN restatements against hand-worked cases, and the oracle's masked estimate
(hcor_params.keep) against the unmasked one and against itself in both visiting orders."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_lib as O  # noqa: E402
import oracle_mask_lib as M  # noqa: E402

synth = importlib.import_module("hc-mvs_amd.synth")


# ---- label list --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arg,labels", [
    ("", None), ("3", [3]), ("3,7", [3, 7]), ("3,", [3, 0]), (",3", [0, 3]), ("-1", [-1]), ("70000", [70000]),
    ("  5,x,12abc", [5, 0, 12]), ("1,,2", [1, 0, 2]),
])
def test_parse_labels(arg, labels):
    assert M.parse_labels(arg) == labels


def test_labels_outside_16_bits_never_match():
    lab = np.array([[0, 1], [65535, 4464]], np.uint16)
    assert M.keep_mask(lab, [-1], 2, 2).all()
    assert M.keep_mask(lab, [70000], 2, 2).all()
    assert M.keep_mask(lab, [65536 + 1], 2, 2).all()  # (4464 + 65536 = 70000 does not wrap either)
    assert (M.keep_mask(lab, [65535, 0], 2, 2) == np.array([[0, 1], [0, 1]])).all()
    assert (M.keep_mask(lab, M.parse_labels("3,"), 2, 2) == np.array([[0, 1], [1, 1]])).all()  # "3," ignores label 0 too


# ---- resizeNN ----------------------------------------------------------------------------------------------------------------

def test_resize_nn_enlarge_by_two():
    lab = np.array([[1, 2], [3, 4]], np.uint16)
    assert (M.resize_nn(lab, 4, 4) == np.array([[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]])).all()


def test_resize_nn_shrink_by_two():
    lab = np.arange(16, dtype=np.uint16).reshape(4, 4)
    assert (M.resize_nn(lab, 2, 2) == np.array([[0, 2], [8, 10]])).all()  # sx = floor(x * 2)


def test_resize_nn_non_integer_factors():
    # 3 -> 5 columns: ifx = 1 / (5 / 3) = 0.6 -> sx = floor(0, 0.6, 1.2, 1.8, 2.4) = 0 0 1 1 2
    lab = np.array([[10, 20, 30]], np.uint16)
    assert (M.resize_nn(lab, 5, 1) == np.array([[10, 10, 20, 20, 30]])).all()
    # 5 -> 3 columns: ifx = 1 / (3 / 5) = 1.6666... -> sx = floor(0, 1.67, 3.33) = 0 1 3
    lab = np.array([[10, 20, 30, 40, 50]], np.uint16)
    assert (M.resize_nn(lab, 3, 1) == np.array([[10, 20, 40]])).all()
    # 7 rows -> 3 rows: ify = 1 / (3 / 7) = 2.333... -> sy = 0 2 4
    lab = np.arange(7, dtype=np.uint16).reshape(7, 1)
    assert (M.resize_nn(lab, 1, 3).ravel() == np.array([0, 2, 4])).all()


def test_resize_nn_last_row_and_column():
    # 2 -> 3: ifx = 1 / 1.5 = 0.666... -> sx = floor(0, 0.67, 1.33) = 0 0 1: the last column is the last source column, never beyond
    lab = np.array([[1, 2], [3, 4]], np.uint16)
    assert (M.resize_nn(lab, 3, 3) == np.array([[1, 1, 2], [1, 1, 2], [3, 3, 4]])).all()
    # 1 x 1 -> anything: the clamp min(sx, sw - 1)
    assert (M.resize_nn(np.array([[9]], np.uint16), 4, 3) == 9).all()
    # 10 -> 7: floor(6 * 10 / 7) = 8 (not 9: the last source column is skipped)
    lab = np.arange(10, dtype=np.uint16).reshape(1, 10)
    assert M.resize_nn(lab, 7, 1)[0, -1] == 8


def test_resize_nn_same_size_is_identity():
    lab = np.random.default_rng(0).integers(0, 65536, (13, 17)).astype(np.uint16)
    assert (M.resize_nn(lab, 17, 13) == lab).all()


# ---- the oracle's masked estimate ----------------------------------------------------------------------------------------

def _scene(w=72, h=60, nsrc=2, seed=5, iters=2, **kw):
    views = synth.make_views(w, h, 90.0, nsrc, seed=seed)
    pts = synth.sparse_points(views, 50)
    d0, n0, dmin, dmax = _splat(views, pts)
    p = O.default_params(adapthalfwin=5, n_estimation_iters=iters, arith_mode=O.ARITH_DEVICE, **kw)
    return views, p, d0, n0, dmin, dmax


def _splat(views, pts):
    L = O.lib()
    v = O.make_view(views[0])
    h, w = views[0]["gray"].shape
    d = np.zeros((h, w), np.float32); n = np.zeros((h, w, 3), np.float32)
    import ctypes as C
    dmin = C.c_float(); dmax = C.c_float()
    p = np.ascontiguousarray(pts, np.float32)
    L.hcor_splat_init(C.byref(v), O.fptr(p), len(p), O.fptr(d), O.fptr(n), C.byref(dmin), C.byref(dmax))
    return d, n, dmin.value, dmax.value


def _blobs(h, w, seed=1):
    rng = np.random.default_rng(seed)
    keep = np.ones((h, w), np.uint8)
    for _ in range(6):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(3, 10)
        yy, xx = np.mgrid[:h, :w]
        keep[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 0
    return keep


@pytest.mark.parametrize("order", [O.ORDER_ZIGZAG, O.ORDER_ROWS])
def test_mask_keeping_everything_is_the_unmasked_estimate(order):
    views, p, d0, n0, dmin, dmax = _scene(order=order, n_threads=3)
    h, w = d0.shape
    ref = O.estimate(views, p, dmin, dmax, d0, n0)
    for keep in (None, np.ones((h, w), np.uint8), M.keep_mask(np.full((h // 2, w // 3), 4, np.uint16), [3, 5, -1], w, h)):
        got = O.estimate(views, p, dmin, dmax, d0, n0, keep=keep)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b)


def test_zigzag_equals_rows_under_masks():
    views, p, d0, n0, dmin, dmax = _scene()
    h, w = d0.shape
    line = np.ones((h, w), np.uint8); line[:, w // 2] = 0
    for keep in (_blobs(h, w), line):
        pz = O.default_params(adapthalfwin=5, n_estimation_iters=2, arith_mode=O.ARITH_DEVICE, order=O.ORDER_ZIGZAG)
        pr = O.default_params(adapthalfwin=5, n_estimation_iters=2, arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=4)
        a = O.estimate(views, pz, dmin, dmax, d0, n0, keep=keep)
        b = O.estimate(views, pr, dmin, dmax, d0, n0, keep=keep)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert 0 < a[3] < O.estimate(views, pz, dmin, dmax, d0, n0)[3]  # masked pixels cost no evaluation


@pytest.mark.parametrize("last", [True, False])
def test_ignored_pixels_hold_applied_then_median(last):
    views, p, d0, n0, dmin, dmax = _scene()
    h, w = d0.shape
    # a dense initial map, so that the median gives a one-pixel masked line a positive depth
    d0 = np.where(d0 > 0, d0, np.float32(0.5 * (dmin + dmax))).astype(np.float32)
    keep = _blobs(h, w, seed=3); keep[:, 20] = 0; keep[: 3, :] = 0
    p.it_external = 0; p.n_external_iters = 1 if last else 2
    d, n, c, ev = O.estimate(views, p, dmin, dmax, d0, n0, keep=keep)
    applied = np.where(keep != 0, d0, 0).astype(np.float32)
    med = np.empty_like(applied)
    O.lib().hcor_median3(O.fptr(applied), w, h, O.fptr(med))
    ign = keep == 0
    assert np.array_equal(d[ign], med[ign])
    assert (n[ign] == 0).all() and (c[ign] == 0).all()
    valid = M.median3_window_valid(keep, d0)
    line = np.zeros((h, w), bool); line[5: h - 5, 20] = True
    assert (d[line & ign & (valid >= 5)] > 0).any()  # the median quirk: a positive depth with a zero normal
    assert (d[ign & (valid < 5)] == 0).all()

"""Small depth maps on which a connected-component labelling goes wrong, for the speckle filter: shared by
test_speckle_ref.py (CPU) and test_gpu_speckle.py.  The device form works on 64 x 16 tiles; the shapes are no multiples of that.
case = dict(name, depth (h, w) float32, speckle_size[, thr])."""
import numpy as np

import speckle_ref as R

TILE_W, TILE_H = 64, 16


def serpentine(w, h, depth=2.0, gap=0.0):
    """a 1-pixel path: the even rows in full, joined by one pixel at alternating ends of the odd rows; the rest of the odd rows holds gap"""
    d = np.full((h, w), gap, np.float32)
    d[0::2, :] = depth
    for k, y in enumerate(range(1, h, 2)):
        d[y, w - 1 if k % 2 == 0 else 0] = depth
    return d


def comb(w, h, depth=3.0):
    """teeth in the even columns hanging down to a spine in the last row: the canonical label, 0, is far from where the teeth meet"""
    d = np.zeros((h, w), np.float32)
    d[:, 0::2] = depth
    d[h - 1, :] = depth
    return d


def checkerboard(w, h):
    """all valid, 4-neighbours never similar (diagonals are): every pixel is a segment of its own"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x + y) % 2 == 0, 1.0, 2.0).astype(np.float32)


def ramp(w, h, step=1.005):
    """neighbours along x differ by 0.5 % (joined), the ends by far more: one segment all the same"""
    return np.tile((np.float32(1.0) * np.float32(step) ** np.arange(w)).astype(np.float32), (h, 1))


def asymmetric_band(w, h, seed):
    """neighbours are equal or apart by a factor inside the band where |dp - dq| / dp < thr <= |dp - dq| / dq: the one-sided test of the
    reference would join such a pair from one side only; the symmetric rule never does"""
    rng = np.random.default_rng(seed)
    d = (np.float32(2.0) * (np.float32(1) + np.float32(0.00702) * rng.integers(0, 2, (h, w)).astype(np.float32))).astype(np.float32)
    return d


def count_in_band(d, thr=R.THR):
    n = 0
    for a, b in ((d[:, :-1], d[:, 1:]), (d[:-1, :], d[1:, :])):
        with np.errstate(all="ignore"):
            diff = np.abs(a - b)
            n += int(((diff / a < thr) != (diff / b < thr)).sum())
    return n


def blobs(w, h, seed, levels=4, holes=0.08):
    """piecewise-constant regions of a smoothed random field, pierced by invalid pixels: segments of every size across the tile borders"""
    rng = np.random.default_rng(seed)
    f = rng.random((h + 8, w + 8))
    k = np.ones(9) / 9
    f = np.apply_along_axis(lambda r: np.convolve(r, k, "valid"), 1, f)
    f = np.apply_along_axis(lambda c: np.convolve(c, k, "valid"), 0, f)
    f = (f - f.min()) / (f.max() - f.min())
    d = (1.0 + 0.5 * np.floor(f * levels)).astype(np.float32)
    d[rng.random((h, w)) < holes] = 0
    return d


def special_values():
    d = np.full((12, 20), 2.0, np.float32)
    d[1, 1] = np.nan
    d.view(np.uint32)[1, 3] = 0x7FC12345                        # a NaN with a payload
    d[2, 5] = np.inf; d[2, 6] = np.inf; d[3, 5] = np.inf      # valid, similar to nothing, each other included
    d[4, 8] = -np.inf
    d[5, 10] = -1.0
    d[6, 12] = -0.0
    d[7, 14] = 0.0
    d[9:12, :] = 0
    d[10, 2:5] = np.inf                                          # a row of infinite depths in the open: three singletons
    d[10, 10] = 1e-38; d[10, 11] = 1e-38                         # denormal-adjacent depths join like any other
    d[11, 19] = 3.4e38
    return d


def sized_blobs():
    """two rectangles of 99 and of 100 pixels: speckle_size 100 removes the first and keeps the second"""
    d = np.zeros((30, 40), np.float32)
    d[2:13, 3:12] = 1.25      # 11 x 9 = 99
    d[15:25, 20:30] = 1.25    # 10 x 10 = 100
    return d


def _cases():
    out = []

    def add(name, depth, speckle_size, thr=None):
        c = dict(name=name, depth=np.ascontiguousarray(depth, np.float32), speckle_size=speckle_size)
        if thr is not None:
            c["thr"] = thr
        out.append(c)

    s = serpentine(64, 48)
    add("serpentine_64x48", s, 100)
    add("serpentine_64x48_removed", s, int((s > 0).sum()) + 1)
    add("serpentine_517x259", serpentine(517, 259, 2.0, 5.0), 517)   # the gaps are segments of 516 pixels, one per odd row: removed
    add("comb_131x37", comb(131, 37), 100)
    add("checkerboard_70x33", checkerboard(70, 33), 2)
    full = np.full((35, 67), 1.5, np.float32)
    add("full_67x35", full, 100)
    add("full_67x35_exact", full, 67 * 35)
    add("full_67x35_one_more", full, 67 * 35 + 1)
    add("sized_99_100", sized_blobs(), 100)
    add("row_1xN", blobs(150, 1, 11, holes=0.05), 10)
    add("column_Nx1", blobs(1, 150, 12, holes=0.05), 10)
    add("one_pixel_valid", np.full((1, 1), 4.0, np.float32), 100)
    add("one_pixel_valid_kept", np.full((1, 1), 4.0, np.float32), 1)
    add("one_pixel_invalid", np.zeros((1, 1), np.float32), 100)
    add("ramp_300x1", ramp(300, 1), 100)
    add("ramp_80x20", ramp(80, 20), 100)
    band = asymmetric_band(66, 18, 5)
    assert count_in_band(band) > 100
    add("asymmetric_band_66x18", band, 4)
    add("special_values", special_values(), 2)
    add("special_values_size0", special_values(), 0)
    add("special_values_size1", special_values(), 1)
    add("blobs_200x50", blobs(200, 50, 1), 100)
    add("blobs_130x70", blobs(130, 70, 2, levels=6, holes=0.15), 30)
    add("blobs_65x17_wide_thr", blobs(65, 17, 3, levels=3), 20, thr=0.4)   # a threshold of the caller's: 1.5 and 2.0 join, 1.0 and 1.5 do not
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]
BATCH = ("blobs_200x50", "special_values", "serpentine_64x48")   # three maps of different sizes in one call


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def aux(depth, seed=0):
    """a normal map and a confidence map to go with a depth map: no zeros, so that a cleared pixel shows"""
    rng = np.random.default_rng(1000 + seed)
    h, w = depth.shape
    n = (rng.random((h, w, 3)) + 0.25).astype(np.float32)
    c = (rng.random((h, w)) + 0.25).astype(np.float32)
    return n, c


def thr_of(case):
    return np.float32(case.get("thr", R.THR))

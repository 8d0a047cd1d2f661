"""helper: the batches that pin the MASK, SPREAD and MASK + SPREAD sweep-kernel instances (--ignore-mask-label, --n-viewspread 1) to the
oracle, in every launch shape -- the 16 classes, sizes, view counts, sweeps, seed offsets and knob grid of tests/sweep_matrix.py with a
FLAVOUR on top: `mask`, `spread`, `mask+spread`.  test_sweep_matrix_flavours_plan.py shows on the CPU which instances and shapes they
launch; test_gpu_sweep_matrix_flavours.py runs them against the oracle.

Items 0 and 2 of a batch carry the flavour; item 1 carries no mask and its source views offer no maps, so the MASK instance also runs an
item without a keep-mask (c.keep == nullptr: it reads a gradient byte it ignores) and the SPREAD instance an item without spreading views
(c.spread == nullptr).

The masks put the edges of the sweep worker's masked-pixel path -- a masked pixel is not evaluated: its stored state enters the row's ring
and its column is published at once -- into every row direction and onto the borders of stretches of 32 columns:
  item 0 (label image of the image's size): blobs; in the upper half of the inside rows whole columns at the first and last column of a
    row and at the last and first column of a stretch of either direction; two adjacent inside rows (stretches without any evaluation; the
    row below waits on a row that only publishes); the last inside row (row 0 of a right-to-left sweep, which waits on no row); the
    rows above the inside (border pixels, never visited);
  item 2 (label image of HALF the image's size: the device resamples it): blobs; the label row that maps onto inside row 0.
With view spread the estimate is outer iteration 1 of 2 (spread is on and the restore hint legal) and starts from the oracle's outer
iteration 0; every source view of item 0 offers maps, every second one of item 2 -- in the classes with 9..16 views the lanes of the
second view set then hold both kinds."""
import functools
import itertools

import numpy as np

import oracle_lib as O
import oracle_mask_lib as OM
import sweep_matrix as M
import sweep_plan_lib as P

FLAVOURS = ("mask", "spread", "mask+spread")
IGNORE = (3, 4)                           # label 5 of the blobs is NOT ignored
SPREAD_KW = dict(it_external=1, n_external_iters=2, propagate_halfwin=5, propagate_step=4)


def has_mask(fl):
    return "mask" in fl


def has_spread(fl):
    return "spread" in fl


def flavoured(i):
    """items 0 and 2 carry the flavour, item 1 stays plain"""
    return i != 1


def params(fl, cls):
    return dict(M.params(cls), **(SPREAD_KW if has_spread(fl) else {}))


def plan_items(fl, cls):
    b = M.border(M.adapthalfwin(cls))
    return [P.image(w, h, v, b, hint=M.has_hint(cls, i), mask=has_mask(fl) and flavoured(i), spread=has_spread(fl) and flavoured(i))
            for i, ((w, h), v) in enumerate(zip(M.SIZES, M.VIEWS[cls[1:3]]))]


def class_plan(lib, fl, cls, launches, segment, waves, n_sweeps=M.N_SWEEPS):
    return P.plan(lib, plan_items(fl, cls), n_sweeps, bool(cls[0]), 256, M.LAUNCH_KNOB[launches], segment, waves)


def configs(lib, fl, cls):
    """the (launches, segment, waves) of the knob grid whose resolved plan differs from that of every earlier one of the flavour's class (a
    spread launch resolves 4 waves to 3, a big-patch launch 3 and 4 to 2)"""
    seen, out = [], []
    for launches, segment, waves in itertools.product(M.LAUNCHES, M.SEGMENTS, M.WAVES):
        pl = class_plan(lib, fl, cls, launches, segment, waves)
        if pl not in seen:
            seen.append(pl)
            out.append((launches, segment, waves))
    return out


def want_key(fl, cls, i):
    """the key of item i's oracle result in sweep_matrix_run.want: the plain item 1 is the plain matrix's in the `mask` flavour and the
    same estimate in the two flavours with view spread"""
    if flavoured(i):
        return ("flavour", fl, cls, i)
    return ("flavour", "spread", cls, i) if has_spread(fl) else ("class", cls, i)


# ---- the masks ---------------------------------------------------------------------------------------------------------------------------

def blobs(h, w, seed, radii=(3, 12)):
    """eight discs of radius 3..11 with labels 3, 4, 5 in turn"""
    rng = np.random.default_rng(seed)
    lab = np.zeros((h, w), np.uint16)
    yy, xx = np.mgrid[:h, :w]
    for k in range(8):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(*radii)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 3 + (k % 3)
    return lab


def edge_columns(ncols):
    """inside columns q: the first and last of a row, and the last and first of a stretch of 32 in a left-to-right sweep (31, 32) and in a
    right-to-left one, which counts from the other end"""
    return (0, 31, 32, ncols - 33, ncols - 32, ncols - 1)


def blank_rows(nrows):
    """the two adjacent inside rows that are masked over the whole width (in the lower half: the masked columns end above them)"""
    return (nrows // 2 + 3, nrows // 2 + 4)


def labels_full(w, h, b, seed):
    """item 0's label image, of the image's own size"""
    nrows, ncols = h - 2 * b, w - 2 * b
    lab = blobs(h, w, seed)
    for q in edge_columns(ncols):
        lab[b:b + nrows // 2, b + q] = 3
    for r in blank_rows(nrows):
        lab[b + r, :] = 4
    lab[h - 1 - b, :] = 3
    lab[:b, :] = 4
    return lab


def labels_half(w, h, b, seed):
    """item 2's label image, of half the image's size (its discs have half the radius: resampled, they cover what item 0's do): label row
    b // 2 is the one INTER_NEAREST maps onto image row b, inside row 0"""
    lab = blobs(h // 2, w // 2, seed, radii=(2, 6))
    lab[b // 2, :] = 3
    return lab


def masked(sc, lab):
    """the scene with the label image and the keep-mask the oracle gets"""
    h, w = sc["views"][0]["gray"].shape
    return dict(sc, labels=lab, ignore=list(IGNORE), keep=OM.keep_mask(lab, IGNORE, w, h))


def kept_share(keep, b):
    return float(keep[b:-b, b:-b].mean())


def positive_share(depth, keep, b):
    """the share of the kept inside pixels on which `depth` is positive"""
    k = keep[b:-b, b:-b] != 0
    return float((depth[b:-b, b:-b][k] > 0).mean())


# ---- the offered maps and the maps an estimate with view spread starts from -------------------------------------------------------------

def offered(views, seed, every=1, holes=0.1):
    """what the source views offer: their analytic maps with holes (depth 0) and scores on both sides of the keep threshold; only every
    `every`-th view offers (the others: None)"""
    rng = np.random.default_rng(seed)
    out = []
    for k, v in enumerate(views[1:]):
        d = v["depth"].copy()
        d[rng.uniform(size=d.shape) < holes] = 0
        m = (d, np.ascontiguousarray(v["normal"], np.float32), rng.uniform(0.0, 0.75, d.shape).astype(np.float32))
        out.append(m if k % every == 0 else None)
    return out


def started(sc, ahw):
    """the scene with the maps outer iteration 1 starts from: outer iteration 0 of the plain estimate on the CPU, one sweep from the splat"""
    p0 = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, it_external=0, n_external_iters=2, adapthalfwin=ahw,
                          n_estimation_iters=1)
    d, n, _, _ = O.estimate(sc["views"], p0, sc["dmin"], sc["dmax"], sc["d0"], sc["n0"])
    return dict(sc, d0=d, n0=n, spread=True)


@functools.lru_cache(maxsize=None)
def _started_class(cls):
    return tuple(started(sc, M.adapthalfwin(cls)) for sc in M.class_scenes(cls))


@functools.lru_cache(maxsize=None)
def class_scenes(fl, cls):
    """the three items of the flavour's class (the views, hints and seed offsets are those of the plain class)"""
    b = M.border(M.adapthalfwin(cls))
    out = []
    for i, sc in enumerate(_started_class(cls) if has_spread(fl) else M.class_scenes(cls)):
        if flavoured(i):
            h, w = sc["views"][0]["gray"].shape
            if has_mask(fl):
                sc = masked(sc, labels_full(w, h, b, 40 + i) if i == 0 else labels_half(w, h, b, 40 + i))
            if has_spread(fl):
                sc = dict(sc, maps=offered(sc["views"], 10 * M.CLASSES.index(cls) + i, every=1 if i == 0 else 2))
        out.append(sc)
    return tuple(out)


# ---- the batch of many small images ------------------------------------------------------------------------------------------------------

def many_masked(i):
    return i % 3 == 0


def many_offers(i):
    return i % 2 == 0


def many_params():
    return dict(adapthalfwin=M.MANY_AHW, n_estimation_iters=M.N_SWEEPS, seed=M.SEED, **SPREAD_KW)


def many_plan_items(n=M.MANY):
    return [P.image(*M.many_size(i), M.MANY_VIEWS, M.border(M.MANY_AHW), mask=many_masked(i), spread=many_offers(i)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def many_scene(i):
    """image i of sweep_matrix.many_scene in the mask+spread flavour: every third one masked (as item 0 of a class), the source views of
    every second one offer maps"""
    sc = started(M.many_scene(i), M.MANY_AHW)
    w, h = M.many_size(i)
    if many_masked(i):
        sc = masked(sc, labels_full(w, h, M.border(M.MANY_AHW), 60 + i))
    if many_offers(i):
        sc = dict(sc, maps=offered(sc["views"], 500 + i))
    return sc


# ---- a batch whose middle item is masked everywhere --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def blank_middle_scenes(cls):
    """the plain class's three items, the middle one with every label ignored: its rows only publish"""
    out = list(M.class_scenes(cls))
    h, w = out[1]["views"][0]["gray"].shape
    out[1] = masked(out[1], np.full((h, w), IGNORE[0], np.uint16))
    return tuple(out)


def blank_middle_plan_items(cls):
    items = M.plan_items(cls)
    items[1] = items[1][:4] + (1, 0)
    return items

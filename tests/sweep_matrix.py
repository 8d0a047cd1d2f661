"""helper: the batches and knob settings that pin every plain sweep-kernel instance (MASK = SPREAD = false) and every launch shape to the
oracle -- test_sweep_matrix_plan.py shows on the CPU, through the plan shim, WHICH instances and shapes they launch;
test_gpu_sweep_matrix.py runs them against the oracle.

16 classes, one per combination of big (patches beyond 64 taps), two (9..16 source views), pack (view counts that leave view groups idle)
and hint (the `restore` variant's extra hypothesis in the last sweep).  A class is a batch of three items of DIFFERENT sizes: their row
counts differ, so in one launch for all sweeps the short image enters its next sweep while the tall ones are still in the previous one, and
in stretches of 32 columns their rows have 3, 2 and 3 stretches, the last one shorter than the others."""
import functools
import importlib
import itertools

import numpy as np

import sweep_plan_lib as P

SIZES = ((88, 72), (72, 88), (104, 56))   # w x h; inside the border of 7: 74 x 58, 58 x 74, 90 x 42; of 10: 68 x 52, 52 x 68, 84 x 36
VIEWS = {(0, 1): (3, 5, 2),               # (two, pack) -> source views per item
         (0, 0): (8, 7, 8),               # V % 8 in {0, 7} for every item: no item's count packs
         (1, 1): (10, 12, 9),
         (1, 0): (16, 15, 16)}
SEED_OFFSETS = (0, 3, 11)
N_SWEEPS = 3                              # sweep 1 runs right-to-left; with a hint the first launch of the one-launch plan still holds two sweeps
SEED = 2024
FOCAL = 90.0

CLASSES = tuple(itertools.product((0, 1), repeat=4))        # (big, two, pack, hint)
WAVES = (1, 2, 3, 4)
LAUNCHES = ("per-sweep", "one")
SEGMENTS = (0, 32)
LAUNCH_KNOB = {"per-sweep": P.PER_SWEEP, "one": P.ONE}


def class_id(cls):
    return "".join(n for n, on in zip(("big", "two", "pack", "hint"), cls) if on) or "plain"


def adapthalfwin(cls):
    return 10 if cls[0] else 6


def border(ahw):
    return max(ahw, 7)


def has_hint(cls, i):
    """items 0 and 2 of a hint class carry a hint, item 1 none: the HINT instance also runs items without one"""
    return bool(cls[3]) and i != 1


def params(cls):
    return dict(adapthalfwin=adapthalfwin(cls), n_estimation_iters=N_SWEEPS, seed=SEED)


def plan_items(cls):
    b = border(adapthalfwin(cls))
    return [P.image(w, h, v, b, hint=has_hint(cls, i)) for i, ((w, h), v) in enumerate(zip(SIZES, VIEWS[cls[1:3]]))]


def class_plan(lib, cls, launches, segment, waves, n_sweeps=N_SWEEPS):
    return P.plan(lib, plan_items(cls), n_sweeps, bool(cls[0]), 256, LAUNCH_KNOB[launches], segment, waves)


def configs(lib, cls):
    """the (launches, segment, waves) of the knob grid whose resolved plan differs from that of every earlier one of the class (a big-patch
    launch resolves 3 and 4 waves to 2)"""
    seen, out = [], []
    for launches, segment, waves in itertools.product(LAUNCHES, SEGMENTS, WAVES):
        pl = class_plan(lib, cls, launches, segment, waves)
        if pl not in seen:
            seen.append(pl)
            out.append((launches, segment, waves))
    return out


# ---- the scenes (rendered once per process; the arrays are shared, nobody writes to them) -----------------------------------------------

def render(w, h, n_src, seed, hint=False):
    """one item: views (0 = the reference), the splat initialisation of the CPU oracle, and with `hint` the ground-truth depth with 0.4 %
    noise and 20 % holes plus the ground-truth normal"""
    import scene_oracle as SO
    synth = importlib.import_module("hc-mvs_amd.synth")
    views = synth.make_views(w, h, FOCAL, n_src, seed=seed)
    d0, n0, dmin, dmax = SO.splat(views[0], synth.sparse_points(views, 80))
    item = dict(views=views, d0=d0, n0=n0, dmin=dmin, dmax=dmax, hint=None)
    if hint:
        rng = np.random.RandomState(seed)
        hd = (views[0]["depth"] * (1 + 0.004 * rng.normal(size=(h, w)))).astype(np.float32)
        hd[rng.uniform(size=(h, w)) < 0.2] = 0
        item["hint"] = (hd, np.ascontiguousarray(views[0]["normal"], np.float32))
    return item


@functools.lru_cache(maxsize=None)
def class_scenes(cls):
    """a tuple of the class's three items; seed offsets are SEED_OFFSETS"""
    key = 100 + 10 * CLASSES.index(cls)
    return tuple(render(w, h, v, key + i, has_hint(cls, i)) for i, ((w, h), v) in enumerate(zip(SIZES, VIEWS[cls[1:3]])))


# ---- the batch of many small images (edges outside the matrix) --------------------------------------------------------------------------

MANY = 17
MANY_AHW = 5
MANY_VIEWS = 3


def many_size(i):
    return (72, 80, 88)[i % 3], 56 + 4 * (i % 7)       # three alternating widths, heights 56 .. 80


def many_seed_offset(i):
    return 5 * i


def many_plan_items(n=MANY):
    return [P.image(*many_size(i), MANY_VIEWS, border(MANY_AHW)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def many_scene(i):
    return render(*many_size(i), MANY_VIEWS, 300 + i)

"""helper: the scenes of the post-filter chain tests (test_postfilter_chain_scenarios.py on the CPU, test_gpu_postfilter_chain.py on the
device), the chain run image after image through the oracle, and what happens between its fusions.

The device computes every fusion of a chain after the first incrementally (pf_kernels.hip) and exposes no owner map, so whether a chain
exercises the incremental paths at all -- estimates released, taken over by an earlier or a later pass, re-linked into the second bank of
the bidder lists -- is established here, on the oracle's owner maps (hcor_cloud::owner), independently of the code under test."""
import functools

import numpy as np

import oracle_lib as O
from fusion_scene import make_maps

FREE = 0xFFFF


def chain_maps(w=512, h=24, depth=5.0):
    """three views of a fronto-parallel plane from ONE camera position: A at full horizontal resolution, B and C at half of it, their
    pixel grids shifted by a quarter pixel either way, so that A's pixels 2j, 2j+1 land on B's pixel j and 2j-1, 2j on C's pixel j.
    With nMinViewsFuse = 3 a pixel of A becomes a point only when BOTH its targets are still free: x = 0 is one (it claims B0 and
    C0), so x = 1 (shares B0) is not, so C1 stays free and x = 2 is one ... -- the answer of every pixel of a row hangs on the answer
    of the pixel before it, over the whole row, and it ALTERNATES: the worst case for an iteration that starts from "every pixel is a
    point" (its changes travel one pixel per step)."""
    f = 300.0
    def view(width, fx, cx):
        K = np.array([[fx, 0, cx], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float64)
        d = np.full((h, width), depth, np.float32)
        n = np.zeros((h, width, 3), np.float32); n[..., 2] = -1
        g = np.full((h, width), 0.5, np.float32)
        g8 = np.full((h, width), 128, np.uint8)
        return dict(K=K, R=np.eye(3), C=np.zeros(3), gray=g, depth=d, normal=n, conf=np.full((h, width), 0.8, np.float32),
                    bgr=np.stack([g8, g8, g8], -1).copy(), d_min=1.0, d_max=10.0, neighbors=[])
    cxA = (w - 1) / 2.0
    A = view(w, f, cxA)
    B = view(w // 2 + 1, f / 2, cxA / 2 - 0.25)
    Cm = view(w // 2 + 1, f / 2, cxA / 2 + 0.25)
    A["neighbors"] = [1, 2]
    return [A, B, Cm], [0, 1, 2]


def _scores(maps):
    """between outer iterations conf holds the SCORE (as the post-filter tests of test_gpu_fuse.py set it up)"""
    for m in maps:
        m["conf"] = np.where(m["depth"] > 0, 1.3 - m["conf"], 0).astype(np.float32)
    return maps


def _ring(seq=None, order=None, **kw):
    maps, o = make_maps(**kw)
    order = o if order is None else order
    return _scores(maps), order, (order[::-1] if seq is None else seq)


def _r4b():
    """R4a's maps with thinned, emptied and padded neighbour lists: 7 is no view (nor an index of the oracle's map array)"""
    maps, _, _ = SCENES["R4a"]()
    maps[0]["neighbors"] = maps[0]["neighbors"][:2]
    maps[2]["neighbors"] = []
    maps[3]["neighbors"] = [7] + maps[3]["neighbors"][:3]
    return maps, [3, 1, 0, 2, 4], [0, 2, 4, 3]


R5_SIZES = [(50, 38), (75, 57), (33, 25), (50, 38), (61, 47)]


def _flip(w, h):
    """scene F: in the first fusion every row of A alternates point / no point from x = 0.  Image 2 (C) is post-filtered first; its column
    1 is empty and gets filled, which gives A's pixel 1 a second target ... and the alternation of every row flips phase, one pixel per
    settle step, inside an INCREMENTAL fusion"""
    maps, order = chain_maps(w, h)
    maps[2]["depth"][:, 1] = 0
    maps[2]["conf"][:, 1] = 0
    return _scores(maps), order, [2, 0, 1]


# name -> () -> (maps, order, seq); NMIN: the nMinViewsFuse values the scene is run with
SCENES = {
    "R1": lambda: _ring(w=64, h=48, f=60, n_views=5, noise=.004, outliers=.15, holes=.25, seed=5),
    "R2": lambda: _ring(w=48, h=40, f=45, n_views=4, noise=.004, outliers=.2, holes=.3, seed=6),
    "R3": lambda: _ring(w=72, h=56, f=66, n_views=6, noise=.006, outliers=.15, holes=.3, seed=7, far=1, far_factor=2.0),
    "R4a": lambda: _ring(w=50, h=38, f=46, n_views=5, noise=.004, outliers=.15, holes=.25, seed=9, order=[2, 0, 3, 1], seq=[4, 1, 3]),
    "R4b": _r4b,
    "R5": lambda: _ring(w=50, h=38, f=46, n_views=5, noise=.004, outliers=.15, holes=.25, seed=11, sizes=R5_SIZES, border=3,
                        order=[0, 1, 2, 3, 4], seq=[1, 2, 0, 4, 3]),
    "R6": lambda: _ring(w=40, h=32, f=37, n_views=18, noise=.004, outliers=.15, holes=.25, seed=10, seq=[3, 0, 9, 1, 17, 5]),
    "F512": lambda: _flip(512, 24),
    "F130": lambda: _flip(130, 17),   # (17 rows: hcmvs_upload_view takes no image under 16, the estimator's border on both sides + 2)
}
NMIN = {"R1": (2, 3), "R2": (2, 3), "R3": (2, 3), "R4a": (2,), "R4b": (2,), "R5": (2, 3), "R6": (3,), "F512": (3,), "F130": (3,)}
CASES = [(name, nmin) for name in SCENES for nmin in NMIN[name]]


@functools.lru_cache(maxsize=None)
def scene(name):
    """(maps, order, seq) of a scene, built once; nobody changes the arrays"""
    maps, order, seq = SCENES[name]()
    for m in maps:
        for a in m.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return maps, list(order), list(seq)


def gradient_of(m):
    """the u8 gradient map GapInterpolation reads, from the image the device takes it from: the colour image when the view has one
    (cv::cvtColor BGR2GRAY), its gray image otherwise"""
    L = O.lib()
    if m.get("bgr") is None:
        return O.gradient_map(np.ascontiguousarray(m["gray"], np.float32))
    b = np.ascontiguousarray(m["bgr"], np.uint8)
    h, w = b.shape[:2]
    g8 = np.empty((h, w), np.uint8); gra = np.empty((h, w), np.uint8)
    L.hcor_bgr2gray_u8(O.u8ptr(b), w, h, O.u8ptr(g8))
    L.hcor_gradient_map(O.u8ptr(g8), w, h, O.u8ptr(gra))
    return gra


def run_chain(maps, order, seq, n_min_views_fuse, **kw):
    """the chain image after image through O.postfilter (device-association transcendentals).  kw: thr, normal_deg, gap.  Returns one
    entry per image of seq: dict(depth, normal, conf: the maps of EVERY image after that image's post-filter; filled: pixels filled so
    far; filled_image: by this image; owners: per image the owner map of this image's fusion; before: the depth map of the post-filtered
    image as its fusion found it)"""
    cur = [dict(m) for m in maps]
    out = []
    total = 0
    for vid in seq:
        before = cur[vid]["depth"]
        dd, nd, cd, filled, own = O.postfilter(cur, vid, gradient_of(cur[vid]), order, mode=O.ARITH_DEVICE, n_min_views_fuse=n_min_views_fuse,
                                               owners=True, **kw)
        total += filled
        for i in range(len(cur)):
            cur[i]["depth"] = dd[i]
        cur[vid]["normal"] = nd; cur[vid]["conf"] = cd
        out.append(dict(depth=[m["depth"] for m in cur], normal=[m["normal"] for m in cur], conf=[m["conf"] for m in cur], filled=total,
                        filled_image=filled, owners=own, before=before))
    return out


@functools.lru_cache(maxsize=None)
def chain_of(name, n_min_views_fuse):
    """the oracle's chain of a scene at the default thresholds, computed once and shared by the tests"""
    maps, order, seq = scene(name)
    return run_chain(maps, order, seq, n_min_views_fuse)


def chain_stats(maps, order, seq, n_min_views_fuse, chain=None):
    """what happens between consecutive fusions of the chain, counted on the oracle's owner maps.  Returns dict of
      released, stolen, handed: one count per pair of consecutive fusions (k, k + 1), summed over all images --
        released: the estimate belonged to a point of fusion k and is free, with a depth > 0, after fusion k + 1
        stolen:   it belongs to a point in both, in fusion k + 1 to one of an EARLIER pass (owner index decreased)
        handed:   ... of a LATER pass (owner index increased)
      moved:  per post-filtered image (in seq order) the pixels whose depth was > 0 before its post-filter and is another value > 0 after
              it: a free estimate inside a gap that GapInterpolation filled over.  Every pair that projects from or onto such a pixel is
              linked again, into the second bank of the bidder lists
      filled: per post-filtered image the pixels GapInterpolation filled"""
    chain = run_chain(maps, order, seq, n_min_views_fuse) if chain is None else chain
    rel, sto, han = [], [], []
    for k in range(len(chain) - 1):
        a, b = chain[k], chain[k + 1]
        r = s = h = 0
        for i in range(len(maps)):
            oa, ob = a["owners"][i], b["owners"][i]
            r += int(((oa != FREE) & (ob == FREE) & (b["depth"][i] > 0)).sum())
            both = (oa != FREE) & (ob != FREE)
            s += int((both & (ob < oa)).sum())
            h += int((both & (ob > oa)).sum())
        rel.append(r); sto.append(s); han.append(h)
    moved = []
    for k, vid in enumerate(seq):
        d0, d1 = chain[k]["before"], chain[k]["depth"][vid]
        moved.append(int(((d0 > 0) & (d1 > 0) & (d0 != d1)).sum()))
    return dict(released=rel, stolen=sto, handed=han, moved=moved, filled=[c["filled_image"] for c in chain])

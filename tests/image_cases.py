"""The inputs of the image-kernel tests (test_image_ref.py on the CPU, test_gpu_image_kernels.py on the device): the case tables of
the resizes, the images of the gradient map and the scene of the point colours.  What is asserted of the kernels lives in the tests; check_color_scene asserts that the scene is what it claims to be."""
import numpy as np

F32 = np.float32

# (source h, source w, scale, path, destination (h, w)): every branch of launch_resize_gray's INTER_AREA side.  Widths sit on both
# sides of the 64-wide launch block, heights 16 .. 19 around the 4-high one; 16 is the smallest image a view may have.
AREA_CASES = [
    (48, 64, 0.5, "fast", (24, 32)),            # the plain integer factor
    (48, 126, 0.5, "fast", (24, 63)),           # destination width 63 / 64 / 65: the edge of the launch block
    (48, 128, 0.5, "fast", (24, 64)),
    (48, 129, 0.5, "fast", (24, 64)),           # 64.5 rounds to even; the last source column is unused
    (48, 130, 0.5, "fast", (24, 65)),
    (97, 131, 0.5, "general", (48, 66)),        # an integer factor that does not fit: 66 * 2 > 131
    (64, 68, 0.25, "fast", (16, 17)),           # the smallest height
    (68, 64, 0.25, "fast", (17, 16)),           # height 17
    (128, 136, 0.125, "fast", (16, 17)),        # 64 taps
    (256, 272, 0.0625, "fast", (16, 17)),       # 256 taps
    (257, 280, 0.0625, "general", (16, 18)),    # factor 16 on the tables, the last cell clamped to the image
    (270, 280, 0.06, "general", (16, 17)),      # factor 16.7: up to 18 table entries per axis
    (60, 78, 1.0 / 3.0, "general", (20, 26)),   # 1 / float32(1 / 3) is not 3: the 1e-3 cut drops the leading slivers
    (90, 85, 0.2, "general", (18, 17)),
    (95, 90, 0.2, "general", (19, 18)),         # height 19
    (112, 112, 1.0 / 7.0, "general", (16, 16)),
    (40, 70, 0.4995, "general", (20, 35)),      # factor 2.002: trailing cells of 0.002, 0.004, .. of a pixel, just above the 1e-3 cut
    (97, 131, 0.62, "general", (60, 81)),
    (97, 131, 0.8, "general", (78, 105)),
    (97, 131, 0.33, "general", (32, 43)),
    (97, 131, 0.25, "general", (24, 33)),       # 33 * 4 > 131
]
CUBIC_CASES = [
    (16, 16, 2.5, "cubic", (40, 40)),
    (17, 23, 1.2, "cubic", (20, 28)),
    (48, 63, 1.7, "cubic", (82, 107)),
    (16, 40, 4.0, "cubic", (64, 160)),
    (97, 131, 1.2, "cubic", (116, 157)),
    (97, 131, 1.7, "cubic", (165, 223)),
    (97, 131, 2.5, "cubic", (242, 328)),
]
RESIZE_CASES = AREA_CASES + CUBIC_CASES
IMPULSE_CASES = [(48, 130, 0.5, "fast"), (90, 85, 0.2, "general"), (270, 280, 0.06, "general"), (17, 23, 1.2, "cubic")]
REFUSED_SCALES = [1.0, 0.9, 1.14, 1.15, 0.85]   # within 15 % of 1 as floats: DepthMap.h:234 does not resample


def case_id(c):
    return "%dx%d@%.4g" % (c[0], c[1], c[2])


def noise_image(h, w, scale):
    seed = h * 1000003 + w * 1009 + int(scale * 10000)
    return np.random.default_rng(seed).uniform(-0.5, 1.5, (h, w)).astype(F32)


def impulse_image(h, w):
    """isolated impulses of both signs, in the corners, on the borders and inside: a tap off by one cannot average out"""
    g = np.zeros((h, w), F32)
    for k, (y, x) in enumerate([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2), (h // 3, w - 2), (h - 2, w // 3), (1, w // 2),
                                (h // 2 + 5, 1)]):
        g[y, x] = F32(1 + k) * (1 if k % 2 == 0 else -1)
    return g


# ---- the gradient map ------------------------------------------------------------------------------------

GRADIENT_SIZES = [(16, 16), (19, 63), (17, 64), (18, 65), (37, 129)]   # h x w: ragged right and bottom edges of the 64 x 4 launch block


def tie_value(k):
    """the float32 whose float32 product with 255 is exactly k + 0.5 (0 <= k < 255; test_image_ref checks all of them)"""
    return F32((2 * k + 1) / 510.0)


def gradient_noise(h, w):
    return np.random.default_rng(7 * h + w).uniform(-0.2, 1.2, (h, w)).astype(F32)


def gradient_ties(h, w):
    """a slow ramp of 8-bit levels k(y, x); two pixels of three hold the level itself, the third the tie k + 0.5.  Neighbouring
    levels differ by 1 or 2, so nothing saturates around a tie.  Returns (image, tie mask, k)"""
    y, x = np.mgrid[0:h, 0:w]
    k = (x + 2 * y) % 255
    tie = (7 * x + 3 * y) % 3 == 0
    g = (k / 255.0).astype(F32)
    g[tie] = ((2 * k[tie] + 1) / 510.0).astype(F32)
    return g, tie, k


def gradient_blocks(h, w):
    """0 / 1 blocks: edges along both axes, corners, and blocks that touch every image border"""
    y, x = np.mgrid[0:h, 0:w]
    return ((((x + 3) // 5) + ((y + 2) // 4)) % 2).astype(F32)


def gradient_bgr(h, w):
    return np.random.default_rng(11 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the point colours -----------------------------------------------------------------------------------

def color_views():
    """views 0 .. 2 carry a colour image, view 3 does not.  R = I, integer centres, f a power of two, integer principal points: every
    projection matrix is exact.  Views 1 and 2 sit at (cx, cy, .): at depth f a point's image position is its own x, y."""
    rng = np.random.default_rng(5)
    def view(w, h, f, cx, cy, C, color=True):   # noqa: E306
        return dict(K=np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]]), R=np.eye(3), C=np.array(C, np.float64), w=w, h=h,
                    gray=rng.uniform(0, 1, (h, w)).astype(F32), bgr=rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if color else None)
    return [view(64, 48, 64.0, 32, 24, (0, 0, 0)), view(64, 48, 64.0, 32, 24, (32, 24, -2)), view(65, 19, 32.0, 32, 9, (32, 9, 1)),
            view(64, 48, 64.0, 32, 24, (0, 0, 4), color=False)]


def color_points(views):
    """(xyz f32 (n, 3), n_views, view_ids, tags): tags[i] names what point i is there for"""
    rng = np.random.default_rng(9)
    pts, lists, tags = [], [], []
    def add(X, ids, tag):   # noqa: E306
        pts.append([F32(X[0]), F32(X[1]), F32(X[2])]); lists.append(list(ids)); tags.append(tag)
    def at(v, px, py, z=None):   # noqa: E306  the point that view v sees at (px, py) at depth z (default f: exact for views 1 and 2)
        V = views[v]
        f, cx, cy = V["K"][0, 0], V["K"][0, 2], V["K"][1, 2]
        z = f if z is None else z
        return (np.float64(px) - cx) * z / f + V["C"][0], (np.float64(py) - cy) * z / f + V["C"][1], z + V["C"][2]
    for v in (0, 1, 2):
        w, h = views[v]["w"], views[v]["h"]
        for _ in range(60):   # interior, random fractions, random depth (1 / z inexact)
            add(at(v, rng.uniform(1, w - 2), rng.uniform(1, h - 2), rng.uniform(20, 90)), [v], "interior")
        for _ in range(12):   # exact integer positions
            add(at(v, int(rng.integers(1, w - 1)), int(rng.integers(1, h - 1))), [v], "integer")
    one = F32(1)
    for v in (1, 2):          # the inclusive border and its float32 neighbours on both sides, on each axis
        w, h = views[v]["w"], views[v]["h"]
        for name, lo, hi in (("x", one, F32(w - 2)), ("y", one, F32(h - 2))):
            for edge, val in (("lo", lo), ("hi", hi)):
                for side, p in (("on", val), ("below", np.nextafter(val, F32(-1e9))), ("above", np.nextafter(val, F32(1e9)))):
                    for other in (F32(5.25), F32(7.0)):
                        add(at(v, p, other) if name == "x" else at(v, other, p), [v], "border-%s-%s-%s" % (name, edge, side))
        add(at(v, one, one), [v], "corner"); add(at(v, F32(w - 2), F32(h - 2)), [v], "corner")
    for v in (0,):            # the same borders through a camera whose principal point does not cancel (x = px - 32 is exact here too)
        for p in (1.0, 62.0, 0.5, 62.5):
            add(at(v, p, 10.5), [v], "v0-border-x")
        for p in (1.0, 46.0, 0.5, 46.5):
            add(at(v, 10.5, p), [v], "v0-border-y")
    add((1.0, 2.0, 50.0), [], "no-view")
    add(at(3, 20.5, 20.5), [3], "no-colour-view")
    add(at(0, 20.5, 21.25), [3, 0], "skip-no-colour")          # view 3 is closer (C z = 4) but has no colour image: view 0
    add(at(0, 20.5, 21.25), [0, 3], "skip-no-colour")
    for px, py in ((20.5, 21.25), (40.0, 30.75), (3.5, 3.5)):
        add(at(0, px, py, 40.0), [0, 1], "closest-of-two")       # depth 40 in view 0, 42 in view 1
        add(at(0, px, py, 40.0), [1, 0], "closest-of-two")
        add(at(1, px, py), [1, 1], "same-view-twice")
        add(at(2, px, 9.5), [2, 0, 1], "closest-of-three")
    # behind: depth -64 in view 0, +2 more in view 1 -> view 0 (the most negative) wins; its projection mirrors into the image
    for px, py in ((20.5, 21.25), (33.0, 24.0), (50.75, 40.5)):
        add(at(0, px, py, -64.0), [1, 0], "behind-inside")
    add((-200.0, 3.0, -64.0), [0, 1], "behind-outside")
    add((0.0, 0.0, 0.0), [0], "at-the-centre")                 # q = 0: 1 / 0, the inside test is false on the NaN
    for _ in range(20):       # outside the image
        add(at(0, rng.uniform(-40, 0.99), rng.uniform(-10, 60), rng.uniform(20, 90)), [0], "outside")
        add(at(2, rng.uniform(0, 64), rng.uniform(17.01, 30), rng.uniform(20, 90)), [2], "outside")
    xyz = np.array(pts, F32)
    nv = np.array([len(l) for l in lists], np.uint32)
    ids = np.array([i for l in lists for i in l], np.uint32)
    return xyz, nv, ids, tags


def check_color_scene(views, tags, detail, want):
    """the scene reaches what it is there for (shared with the device test)"""
    white = (want == 255).all(1)
    by = lambda t: [i for i, s in enumerate(tags) if s.startswith(t)]   # noqa: E731
    assert 200 < len(tags) < 1000 and white.any() and (~white).any()
    assert all(detail[i][3] for i in by("interior") + by("integer") + by("corner") + by("behind-inside") + by("same-view-twice"))
    assert not any(detail[i][3] for i in by("outside") + by("behind-outside") + by("at-the-centre") + by("no-view") + by("no-colour-view"))
    assert all(detail[i][0] == -1 for i in by("no-view") + by("no-colour-view")) and all(detail[i][0] == 0 for i in by("skip-no-colour") + by("behind"))
    assert all(detail[i][0] == 0 for i in by("closest-of-two")) and all(detail[i][0] == 2 for i in by("closest-of-three"))
    assert all(float(detail[i][1]) == int(detail[i][1]) and float(detail[i][2]) == int(detail[i][2]) for i in by("integer"))
    for i in by("border-"):
        _, axis, edge, side = tags[i].rsplit("-", 3)
        v, px, py, inside = detail[i]
        lim = F32(1) if edge == "lo" else F32((views[v]["w"] if axis == "x" else views[v]["h"]) - 2)
        p = px if axis == "x" else py
        assert {"on": p == lim, "below": p == np.nextafter(lim, F32(-1e9)), "above": p == np.nextafter(lim, F32(1e9))}[side], (tags[i], p)
        assert inside == (side == "on" or (side == "above") == (edge == "lo")), (tags[i], p)
    assert [detail[i][3] for i in by("v0-border-x")] == [True, True, False, False] == [detail[i][3] for i in by("v0-border-y")]

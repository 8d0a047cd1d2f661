"""The tables and the tiling the device initialisations are built on (hc-mvs_amd/csrc/init_plan.h, the set-up half of tri_init.cpp), on
the CPU through tests/init_plan_shim.cpp:
  - the tile lists name exactly the entries whose clamped box meets the tile, in strictly ascending order;
  - the face table is a complete statement of the raster: the host loop's rule (highest index wins, z > 0) evaluated over it in numpy
    gives binding.triangulate_points bit for bit, so the refactored host form and any other consumer of the table agree;
  - the same for the splat's table against hcmvs_splat_points."""
import ctypes as C
import importlib

import numpy as np
import pytest

import init_plan_lib as IP

binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")

SIZES = [(97, 131, 120.0), (160, 120, 150.0), (320, 200, 300.0)]


def scene(w, h, f, n, seed):
    views = synth.make_views(w, h, f, 1, seed=seed)
    return views[0], synth.sparse_points(views, n, seed=seed + 3)


def check_tiling(w, h, boxes):
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    tw, th = IP.tile_shape()
    tx, ty, first, items = IP.bin_tiles(w, h, boxes)
    assert (tx, ty) == ((w + tw - 1) // tw, (h + th - 1) // th)
    assert first[0] == 0 and first[-1] == len(items) and np.all(np.diff(first.astype(np.int64)) >= 0)
    listed = np.zeros((len(boxes), ty, tx), bool)      # listed[i, tile]: the tile's list names entry i
    for t in range(tx * ty):
        lst = items[first[t]:first[t + 1]].astype(np.int64)
        assert np.all(np.diff(lst) > 0), "tile %d: list not strictly ascending" % t
        assert lst.size == 0 or (lst[0] >= 0 and lst[-1] < len(boxes))
        listed[lst, t // tx, t % tx] = True
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        # every pixel lies in exactly one tile (the tiles partition the image): upsample the entry's tiles to pixels
        px = np.repeat(np.repeat(listed[i], th, 0), tw, 1)[:h, :w]
        inside = np.zeros((h, w), bool)
        if x0 < x1 and y0 < y1:
            inside[y0:y1, x0:x1] = True
        assert px[inside].all(), "entry %d: a pixel of its box lies in a tile that does not list it" % i
        for t_y, t_x in zip(*np.nonzero(listed[i])):      # no list names an entry whose box misses the tile
            assert inside[t_y * th:(t_y + 1) * th, t_x * tw:(t_x + 1) * tw].any(), "entry %d listed by tile (%d, %d) its box misses" % (i, t_x, t_y)
    return len(items)


@pytest.mark.parametrize("w,h,f", SIZES)
@pytest.mark.parametrize("n", [4, 25, 400])
@pytest.mark.parametrize("add_corners", [0, 1])
def test_tiling_of_triangulations(w, h, f, n, add_corners):
    v, pts = scene(w, h, f, n, seed=n + w)
    tab = IP.tri_table(w, h, v["K"], v["R"], v["C"], pts, add_corners=bool(add_corners))
    assert tab is not None and len(tab["faces"]) >= 1
    faces = tab["faces"]
    assert np.all(np.diff(faces["index"]) > 0)          # the host loop's order
    boxes = IP.face_boxes(faces)
    assert (boxes[:, 0] >= 0).all() and (boxes[:, 1] >= 0).all() and (boxes[:, 2] <= w).all() and (boxes[:, 3] <= h).all()
    assert check_tiling(w, h, boxes) >= 1


@pytest.mark.parametrize("w,h,f", SIZES)
def test_tiling_of_one_face_over_the_whole_image(w, h, f):
    tw, th = IP.tile_shape()
    n = check_tiling(w, h, [[0, 0, w, h]])
    assert n == ((w + tw - 1) // tw) * ((h + th - 1) // th)
    # with an empty box and a one-pixel box in the last corner next to it
    assert check_tiling(w, h, [[0, 0, w, h], [5, 5, 5, 9], [w - 1, h - 1, w, h]]) == n + 1


def test_layout_keeps_the_counters_first_and_the_pieces_apart():
    for tb, nt, ne in ((0, 1, 0), (120 * 7, 18, 40), (20 * 2004, 300, 51000)):
        counters, table, first, items, total = IP.layout(tb, nt, ne)
        assert counters == 0 and table >= 16 and first >= table + tb and items >= first + 4 * (nt + 1) and total >= items + 4 * ne
        assert all(o % 256 == 0 for o in (table, first, items, total))


@pytest.mark.parametrize("w,h,f,n,seed", [(160, 120, 150.0, 60, 1), (320, 200, 300.0, 400, 2), (97, 131, 120.0, 25, 3)])
@pytest.mark.parametrize("add_corners", [1, 0])
def test_face_table_states_the_host_raster(w, h, f, n, seed, add_corners):
    v, pts = scene(w, h, f, n, seed)        # the three scenes of test_triangulate_init.py
    d, nm, lo, hi = binding.triangulate_points(w, h, v["K"], v["R"], v["C"], pts, add_corners=bool(add_corners))
    tab = IP.tri_table(w, h, v["K"], v["R"], v["C"], pts, add_corners=bool(add_corners))
    td, tn, hits = IP.raster_faces(tab, w, h)
    assert np.array_equal(td, d) and np.array_equal(tn, nm)
    assert lo == tab["lo"] * np.float32(0.9) and hi == tab["hi"] * np.float32(1.1)
    assert hits >= (d > 0).sum() > 0
    assert tab["n_used"] <= n


def splat_points_host(w, h, v, pts):
    pts = np.ascontiguousarray(pts, np.float32)
    d = np.full((h, w), 7.0, np.float32); nm = np.zeros((h, w, 3), np.float32)
    lo, hi = C.c_float(), C.c_float()
    fp = C.POINTER(C.c_float)
    arrs = [np.ascontiguousarray(v[k], np.float64) for k in ("K", "R", "C")]
    rc = binding.lib().hcmvs_splat_points(w, h, *[a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs], pts.ctypes.data_as(fp), len(pts),
                                          d.ctypes.data_as(fp), nm.ctypes.data_as(fp), C.byref(lo), C.byref(hi))
    assert rc == 0
    return d, nm, lo.value, hi.value


@pytest.mark.parametrize("w,h,f,n,seed", [(160, 120, 150.0, 300, 1), (97, 131, 120.0, 40, 2), (320, 200, 300.0, 400, 3)])
def test_splat_table_states_the_host_splat_and_tiles(w, h, f, n, seed):
    v, pts = scene(w, h, f, n, seed)
    extra = []                               # blocks clamped at the border, and one wholly outside
    for (x, y, z) in ((-1.0, 5.0, 9.0), (w + 0.4, h - 1.0, 11.0), (1.0, 1.0, 8.5), (w - 2.0, 0.0, 12.0), (w + 40.0, -30.0, 10.0)):
        Xc = np.array([(x - v["K"][0, 2]) * z / v["K"][0, 0], (y - v["K"][1, 2]) * z / v["K"][1, 1], z])
        extra.append(Xc @ v["R"] + v["C"])
    pts = np.vstack([pts, np.asarray(extra, np.float32)]).astype(np.float32)
    d, nm, lo, hi = splat_points_host(w, h, v, pts)
    tab = IP.splat_table(w, h, v["K"], v["R"], v["C"], pts)
    td, hits = IP.raster_splats(tab, w, h)
    assert np.array_equal(td, d) and not nm.any()
    assert lo == tab["lo"] * np.float32(0.9) and hi == tab["hi"] * np.float32(1.1)
    assert (tab["box"][-1] == 0).all()       # the point outside covers nothing
    assert hits > (d > 0).sum()
    assert check_tiling(w, h, tab["box"]) >= len(pts) - 1

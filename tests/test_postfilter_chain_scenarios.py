"""Conditions on the INPUTS of test_gpu_postfilter_chain.py, met by the oracle alone (no device): every chain the device is compared on
does, between its fusions, what the incremental path of pf_kernels.hip has special code for -- estimates released, taken over by an earlier
pass (stolen) or a later one (handed on), free estimates filled over (moved: the pair is linked again, into the second bank of the bidder
lists), an image that is a target only, unregistered neighbour ids, more than 16 neighbours, and a change that travels one pixel per settle
step over a whole row.  Without them the device tests could pass on chains in which nothing incremental happens.

Counted on the owner maps of the oracle's fusion (hcor_cloud::owner); measured (released, stolen, handed) per pair of fusions:
  R1 nMinViewsFuse 2: (2,2,0) (5,4,0) (11,118,0) (45,411,6), moved 83 .. 259 per image;  R1 / 3: (40,76,5) (44,83,3) (46,85,2) (65,378,2)
  R2 / 2: (0,2,0) (2,1,0) (20,182,0);  R2 / 3: (13,25,1) (16,24,2) (31,29,0)
  R3 / 2: (5,3,0) (5,2,0) (27,223,1) (86,800,2) (4,20,6);  R3 / 3: (65,118,5) (52,106,2) (74,166,4) (93,765,2) (11,33,6)
  R4a: (2,2,0) (3,0,0), image 4 filled 336;  R4b: (11,36,0) (3,4,0) (1,1,0)
  R5 / 2: (101,72,0) (2,3,0) (304,815,1) (2,3,0);  R5 / 3: (187,120,1) (21,14,0) (264,483,9) (123,96,2)
  R6: (2,54,0) (53,1301,33) (0,0,0) (1,16,7) (0,0,0)
  F512: 6144 released by the second fusion (h * w/2: every point of the first), none after it;  F130 (130 x 17): 1105."""
import numpy as np
import pytest

import chain_scenes as S
import oracle_lib as O


def stats(name, nmin):
    maps, order, seq = S.scene(name)
    return S.chain_stats(maps, order, seq, nmin, chain=S.chain_of(name, nmin))


def test_owner_output_is_optional_and_consistent():
    """the owner maps change nothing else; an estimate has an owner iff it is in the mask RemoveSmallSegments keeps (a valid depth after the
    fusion, in a point); owners are positions in the fusion order"""
    maps, order, seq = S.scene("R4b")
    vid = seq[0]
    gra = S.gradient_of(maps[vid])
    plain = O.postfilter(maps, vid, gra, order, mode=O.ARITH_DEVICE)
    dd, nd, cd, filled, own = O.postfilter(maps, vid, gra, order, mode=O.ARITH_DEVICE, owners=True)
    assert filled == plain[3] and np.array_equal(nd, plain[1]) and np.array_equal(cd, plain[2])
    assert all(np.array_equal(a, b) for a, b in zip(dd, plain[0]))
    pos = {img: i for i, img in enumerate(order)}
    n_owned = 0
    for i, m in enumerate(maps):
        owned = own[i] != S.FREE
        n_owned += int(owned.sum())
        assert own[i].shape == m["depth"].shape and (own[i][owned] < len(order)).all()
        assert (m["depth"][owned] > 0).all()                     # only estimates belong to points ...
        if i != vid:
            assert (dd[i][owned] > 0).all()                      # ... and a point's estimates are not invalidated
        if i not in pos:
            assert i not in [order[k] for k in np.unique(own[i][owned])]   # an image that is no seed is merged into other images' points
    assert n_owned > 1000
    # the mask of the post-filtered image: unowned estimates are gaps to GapInterpolation, owned ones keep their value
    owned = own[vid] != S.FREE
    assert np.array_equal(dd[vid][owned], maps[vid]["depth"][owned])
    # a fusion without a request for owners (the cloud's pointer is NULL) is the fusion of every existing caller
    a = O.fuse_depthmaps(maps, order, 20000)
    assert a["n_points"] > 500


@pytest.mark.parametrize("name,nmin", [c for c in S.CASES if c[0] in ("R1", "R2", "R3", "R5")])
def test_rings_release_and_steal(name, nmin):
    st = stats(name, nmin)
    need = {"R1": (10, 10), "R2": (10, 10), "R3": (50, 100), "R5": (100, 80)}[name]
    print(name, nmin, st)
    assert any(r >= need[0] and s >= need[1] for r, s in zip(st["released"], st["stolen"])), st      # in one and the same fusion
    if name == "R1":
        assert max(st["handed"]) >= 1, st
        assert min(st["moved"]) >= 50, st


def test_target_only_image_and_odd_pixel_count():
    """R4a: 1900 pixels per image (not a multiple of 64: the padded tail of the delta scan); image 4 is post-filtered but is no seed of the
    fusion order, so all it has is the target side of the chain state"""
    maps, order, seq = S.scene("R4a")
    assert maps[0]["depth"].size == 1900 and 1900 % 64 != 0 and 4 in seq and 4 not in order
    st = stats("R4a", 2)
    print(st)
    assert st["filled"][seq.index(4)] > 100 and max(st["released"]) >= 1, st


def test_thinned_lists_and_an_unregistered_neighbour():
    """R4b: a neighbour id that is no view heads a list, one list is empty, one is cut short"""
    maps, order, seq = S.scene("R4b")
    assert maps[3]["neighbors"][0] == 7 and len(maps) == 5 and maps[2]["neighbors"] == [] and len(maps[0]["neighbors"]) == 2
    st = stats("R4b", 2)
    print(st)
    assert any(r >= 4 and s >= 4 for r, s in zip(st["released"], st["stolen"])), st
    # the oracle passes id 7 over: the chain equals that of the list without it
    bare = [dict(m) for m in maps]
    bare[3]["neighbors"] = maps[3]["neighbors"][1:]
    a, b = S.chain_of("R4b", 2), S.run_chain(bare, order, seq, 2)
    for x, y in zip(a, b):
        assert x["filled"] == y["filled"] and all(np.array_equal(p, q) for p, q in zip(x["depth"], y["depth"]))


def test_many_neighbours():
    """R6: 17 neighbours per image, bits 16 and above of the merge / in-front masks"""
    maps, order, seq = S.scene("R6")
    assert all(len(m["neighbors"]) == 17 for m in maps)
    st = stats("R6", 3)
    print(st)
    assert max(st["stolen"]) >= 1000, st


def test_sizes_differ():
    """R5: every neighbour list names images of other sizes, larger and smaller than the image itself"""
    maps, order, seq = S.scene("R5")
    assert [m["depth"].shape[::-1] for m in maps] == S.R5_SIZES
    for m, (w, h) in zip(maps, S.R5_SIZES):
        assert m["K"][0, 2] == (w - 1) / 2.0 and m["K"][1, 2] == (h - 1) / 2.0 and m["K"][0, 0] == m["K"][1, 1] == 46 * w / 50.0
        assert (m["depth"][3:-3, 3:-3] > 0).mean() > 0.5 and not m["depth"][:3].any() and not m["depth"][:, -3:].any()


@pytest.mark.parametrize("name", ["F512", "F130"])
def test_phase_flip_of_every_row(name):
    """scene F: the gap interpolation of image 2 fills one pixel per row; in the second fusion the alternation of every row of image 0 flips
    phase.  With C's column 1 empty the first fusion's points are x = 0 (B0, C0), then x = 3 (B1, C2), 5, 7 ... w - 1; once it is filled
    they are x = 0, 2, 4 ... w - 2.  The targets in B and C change hands within the pass (pixels 2j and 2j + 1 share B's pixel j), so what is
    released per row are the w/2 - 1 odd pixels of image 0 and the last pixel of C: h * w/2 estimates.  The third fusion changes nothing."""
    maps, order, seq = S.scene(name)
    h, w = maps[0]["depth"].shape
    st = stats(name, 3)
    print(st)
    assert st["filled"][0] == h
    assert st["released"][0] == h * (w // 2), st
    own0, own1 = (S.chain_of(name, 3)[k]["owners"][0] for k in (0, 1))
    assert (own0[:, 0] == 0).all() and (own0[:, 3::2] == 0).all() and (own0[:, 1:3] == S.FREE).all() and (own0[:, 2::2] == S.FREE).all()
    assert (own1[:, 0::2] == 0).all() and (own1[:, 1::2] == S.FREE).all()          # every pixel of every row from x = 2 on changed
    assert st["released"][1:] == [0] * (len(seq) - 2) and st["stolen"][1:] == [0] * (len(seq) - 2) and st["handed"][1:] == [0] * (len(seq) - 2), st

"""The hand-off between two pyramid levels on the host (hcmvs_handoff_maps: the rule of include/hcmvs_hip.h in a plain loop, the form the
device kernels are pinned to) against three independent statements of it: tests/handoff_ref.py (numpy float32, written from the rule),
the stand-alone driver's own code (sceneio::resize_cubic + its clean-up loop, through tests/handoff_shim.cpp) and, for the enlarging of
hint mode, the oracle's resize_area_up.  And the HIP-free plan of the device form (handoff_plan.h): every refusal, and the prefix table.
No GPU."""
import importlib

import numpy as np
import pytest

import handoff_ref as R
import oracle_lib as O

binding = importlib.import_module("hc-mvs_amd.binding")
F = np.float32

HINT_RANGES = {"mixed": (2.0, 7.0), "clean": (0.5, 20.0), "nan_last": (2.0, 7.0), "empty": (3.0, 4.0)}


def host(mode, d, n, dw, dh, **rng):
    return binding.handoff_maps([dict(depth=d, normal=n, dst_w=dw, dst_h=dh, **rng)], mode)[0]


def same_result(got, want, given=(0.0, 0.0)):
    """maps, range, status and counters; an empty init item leaves the range as it was given"""
    ok = R.same_bits(got["depth"], want["depth"]) and R.same_bits(got["normal"], want["normal"]) and got["status"] == want["status"]
    ok = ok and all(got[k] == want[k] for k in ("n_valid", "n_clamped", "n_rescaled"))
    lo, hi = (given if want["d_min"] is None else (want["d_min"], want["d_max"]))
    return ok and R.same_bits(F(got["d_min"]), F(lo)) and R.same_bits(F(got["d_max"]), F(hi))


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("src,dst", R.INIT_SHAPES)
def test_init_mode_equals_the_numpy_statement_and_the_driver(src, dst, content):
    d, n = R.make_maps(*src, content)
    want = R.handoff_init(d, n, *dst)
    got = host("init", d, n, *dst, d_min=-5.0, d_max=-6.0)
    assert same_result(got, want, given=(-5.0, -6.0))
    assert not np.isnan(got["depth"]).any() and (got["depth"] >= 0).all()
    # the code the stand-alone driver runs today
    rc, dd, dn, lo, hi = R.driver_hand_over(d, n, *dst)
    assert R.same_bits(dd, got["depth"]) and R.same_bits(dn, got["normal"])
    empty = not (want["depth"] > 0).any()
    assert (rc == 3) == (got["status"] == binding.HANDOFF_EMPTY) == empty and (content != "empty" or empty)
    if rc == 0:
        assert R.same_bits(F(lo), F(got["d_min"])) and R.same_bits(F(hi), F(got["d_max"]))
        assert got["d_min"] == 0.0 or (got["depth"] > 0).all()       # a map with holes: the range starts at 0
        k = got["depth"] > 0
        ln = np.linalg.norm(got["normal"][k].astype(np.float64), axis=-1)
        assert np.all((np.abs(ln[~np.isnan(ln)] - 1) < 1e-6) | (ln[~np.isnan(ln)] == 0))


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("src,dst", R.HINT_SHAPES)
def test_hint_mode_equals_the_numpy_statement_and_the_oracle_resize(src, dst, content):
    d, n = R.make_maps(*src, content, hint=True)
    lo, hi = HINT_RANGES[content]
    want = R.handoff_hint(d, n, *dst, lo, hi)
    got = host("hint", d, n, *dst, d_min=lo, d_max=hi)
    assert same_result(got, want)
    assert got["status"] == binding.HANDOFF_OK and not np.isnan(got["depth"]).any()
    # the enlarged values before the clean-up are cv::resize INTER_AREA's, as the oracle restates it
    assert R.same_bits(want["raw"], O.resize_area_up(d, *dst)) and R.same_bits(R.area_up(n, *dst)[0], O.resize_area_up(n, *dst))
    k = got["depth"] > 0
    assert R.same_bits(got["depth"][k], O.resize_area_up(d, *dst)[k])
    assert R.same_bits(got["normal"][~k], O.resize_area_up(n, *dst)[~k])          # no hint there: the normal stays as enlarged
    assert got["d_min"] >= 0 and (np.isnan(got["d_max"]) or got["d_max"] >= hi)
    if content == "nan_last":
        assert np.isnan(got["d_max"])        # the last pixel is a NaN: it replaces hi and nothing follows
    if content == "clean":
        assert (got["d_min"], got["d_max"]) == (0.0 if (want["raw"] == 0).any() else F(lo), F(hi))     # every depth lies inside 0.5 .. 20
    if content == "empty":
        assert got["n_valid"] == 0 and (got["d_min"], got["d_max"]) == (0.0, F(hi))


def test_the_step_beside_a_hole_is_clamped_and_a_nan_behind_hi_is_forgotten():
    d, n = R.make_maps(37, 29, "mixed")
    want = R.handoff_init(d, n, 74, 58)
    assert want["n_negative"] >= 1           # the cubic kernel undershoots between the 9 and the hole: the case proves something
    x, y = R.STEP_AT
    assert (want["raw"][2 * y - 2:2 * y + 3, 2 * x + 4:2 * x + 12] < 0).any()
    got = host("init", d, n, 74, 58)
    assert got["n_clamped"] == want["n_clamped"] >= want["n_negative"] and (got["depth"] >= 0).all()
    assert np.isnan(want["raw"]).any() and np.isnan(got["normal"]).any()         # the NaN depth and the NaN normals reached the result
    # hint mode: a NaN in the middle replaces hi, the depths behind it take over again; the negative depth reaches lo and is cut at 0
    d, n = R.make_maps(37, 29, "mixed", hint=True)
    want = R.handoff_hint(d, n, 74, 58, 2.0, 50.0)
    raw = want["raw"].reshape(-1)
    last = np.flatnonzero(np.isnan(raw))[-1]
    assert want["n_negative"] >= 1 and 0 < last < len(raw) - 1
    assert want["d_max"] == raw[last + 1:].max() < 50.0        # the 50 taken in came before the NaN
    got = host("hint", d, n, 74, 58, d_min=2.0, d_max=50.0)
    assert same_result(got, want) and got["d_min"] == 0.0


def test_a_batch_of_mixed_sizes_equals_the_single_calls():
    maps = []
    for (src, dst), content in zip(R.INIT_SHAPES[:5], ["mixed", "clean", "empty", "mixed", "clean"]):
        d, n = R.make_maps(*src, content, seed=7)
        maps.append(dict(depth=d, normal=n, dst_w=dst[0], dst_h=dst[1], d_min=1.0, d_max=2.0))
    batch = binding.handoff_maps(maps, "init")
    assert [b["status"] for b in batch] == [0, 0, 1, 0, 0]
    for m, b in zip(maps, batch):
        one = binding.handoff_maps([m], "init")[0]
        assert R.same_bits(one["depth"], b["depth"]) and R.same_bits(one["normal"], b["normal"])
        assert {k: v for k, v in one.items() if k not in ("depth", "normal")} == {k: v for k, v in b.items() if k not in ("depth", "normal")}
    assert (batch[2]["d_min"], batch[2]["d_max"]) == (1.0, 2.0) and not batch[2]["depth"].any()     # untouched; the maps written all the same


# ---- the plan: refusals and the prefix table -------------------------------------------------------------------------------------------

def test_every_refusal_of_the_plan_and_of_the_host_form():
    cases, keep = R.refusals()
    assert len(cases) >= 25
    for name, items, mode, n in cases:
        refused, why = R.plan_check(items, mode, n)
        assert refused and why, name
        if items is not None and n is None:
            rc, res = binding.handoff_maps_raw(items, mode)
            assert rc == binding.ERR_INVALID and all(r["status"] == -1 for r in res), name
    # the same items, mended, pass; sources may be shared between items
    a, bufs = R.good_item()
    b, bufs2 = R.good_item()
    for mode in (0, 1):
        assert R.plan_check([a, dict(b, src_depth=a["src_depth"], src_normal=a["src_normal"])], mode) == (False, "")
    assert R.plan_check([R.good_item(8, 6, 8, 6)[0]], 1) == (False, "")       # a hint of equal size
    assert R.plan_check([R.good_item(8, 6, 5, 3)[0]], 0) == (False, "")       # init mode shrinks
    assert binding.handoff_maps_raw([a], 0)[0] == binding.OK
    full = [R.good_item() for _ in range(64)]
    assert R.plan_check([it for it, _ in full], 0) == (False, "")


def test_prefix_table_every_pixel_belongs_to_one_workgroup_of_one_item():
    sizes = [(74, 58), (61, 47), (5, 3), (200, 3), (300, 211)]     # 300 x 211 = 63 300 pixels: 31 workgroups, the last one partly filled
    items = [R.good_item(4, 3, w, h)[0] for w, h in sizes]
    first = R.plan_first(items)
    chunk, block = R.shim().layout["chunk"], R.shim().layout["block"]
    assert chunk % block == 0 and first[0] == 0 and (np.diff(first) >= 1).all()
    owner = [np.zeros(w * h, np.int32) for w, h in sizes]
    for blk in range(first[-1]):
        q = int(np.searchsorted(first, blk, side="right")) - 1          # the last entry <= blk: the kernel's bisection
        assert 0 <= q < len(sizes)
        base = (blk - first[q]) * chunk
        n = sizes[q][0] * sizes[q][1]
        assert base < n                                                 # no workgroup without a pixel
        for k in range(chunk // block):
            lo = base + k * block
            owner[q][lo:min(lo + block, n)] += 1
    assert all((o == 1).all() for o in owner)
    assert first[-1] == sum(-(-w * h // chunk) for w, h in sizes)

"""The plan of the speckle filter (hc-mvs_amd/csrc/speckle_plan.h through tests/speckle_plan_shim.cpp, g++ alone): what a call refuses before
any work, the tile table of a batch and the layout of the one scratch buffer."""
import importlib

import numpy as np
import pytest

import speckle_lib as SL
import speckle_ref as R

binding = importlib.import_module("hc-mvs_amd.binding")

THR = float(R.THR)
D, N, Cf, Lb = 0x10000000, 0x20000000, 0x30000000, 0x40000000   # four addresses far apart


def test_constants_and_default_threshold():
    k = SL.constants()
    assert (k["tile_w"], k["tile_h"], k["block"], k["max_items"], k["scratch_per_pixel"]) == (64, 16, 256, 64, 8)
    assert k["args_bytes"] == SL.ARGS.itemsize
    assert np.float32(SL.lib().ss_default_threshold()) == R.THR == np.float32(0.01) * np.float32(0.7)
    assert np.float32(binding.SPECKLE_DIFF) == R.THR


def test_a_plain_call_may_run():
    assert SL.check([(D, N, Cf, Lb, 96, 80)], THR) == ""
    assert SL.check([(D, 0, 0, 0, 96, 80)], THR) == ""
    assert SL.check([(D + i * 0x1000000, 0, 0, 0, 1920, 1080) for i in range(64)], THR) == ""
    assert SL.check([(D, 0, 0, 0, 46340, 46340)], THR) == ""            # 46340^2 < 2^31


@pytest.mark.parametrize("items, n, thr, word", [
    (None, 1, THR, "null items"),
    ([(D, 0, 0, 0, 8, 8)], 0, THR, "n_items"),
    ([(D, 0, 0, 0, 8, 8)], -3, THR, "n_items"),
    ([(D, 0, 0, 0, 8, 8)], 65, THR, "n_items"),
    ([(D, 0, 0, 0, 0, 8)], None, THR, "size below 1"),
    ([(D, 0, 0, 0, 8, -1)], None, THR, "size below 1"),
    ([(D, 0, 0, 0, 46341, 46341)], None, THR, "2^31"),
    ([(D, 0, 0, 0, 65536, 32768)], None, THR, "2^31"),
    ([(0, N, Cf, Lb, 8, 8)], None, THR, "null depth"),
    ([(D, 0, 0, 0, 8, 8), (0, 0, 0, 0, 8, 8)], None, THR, "item 1: null depth"),
    ([(D, 0, 0, 0, 8, 8)], None, 0.0, "threshold"),
    ([(D, 0, 0, 0, 8, 8)], None, -0.007, "threshold"),
    ([(D, 0, 0, 0, 8, 8)], None, float("nan"), "threshold"),
    ([(D, 0, 0, 0, 8, 8)], None, float("inf"), "threshold"),
    ([(D, D, 0, 0, 8, 8)], None, THR, "overlaps"),
    ([(D, D + 8 * 8 * 4 - 1, 0, 0, 8, 8)], None, THR, "overlaps"),                       # the last byte of the depth
    ([(D, 0, D - 8 * 8 * 4 + 4, 0, 8, 8)], None, THR, "overlaps"),
    ([(D, N, Cf, N + 8 * 8 * 12 - 4, 8, 8)], None, THR, "the normal of item 0 overlaps the labels of item 0"),
    ([(D, 0, 0, 0, 8, 8), (N, 0, 0, D + 4, 8, 8)], None, THR, "the depth of item 0 overlaps the labels of item 1"),
    ([(D, 0, 0, 0, 8, 8), (D, 0, 0, 0, 8, 8)], None, THR, "overlaps"),
])
def test_refusals(items, n, thr, word):
    why = SL.check(items, thr, n)
    assert word in why, why


def test_buffers_that_touch_do_not_overlap():
    assert SL.check([(D, D + 8 * 8 * 4, D + 8 * 8 * 16, D + 8 * 8 * 20, 8, 8)], THR) == ""


def test_tile_table():
    sizes = [(1, 1), (64, 16), (65, 16), (64, 17), (517, 259), (1920, 1080), (1, 300), (300, 1)]
    items = [(D + i * 0x1000000, 0, 0, 0, w, h) for i, (w, h) in enumerate(sizes)]
    first, pixel0, fits = SL.tiles(items)
    assert fits and first[0] == 0 and pixel0[0] == 0
    for i, (w, h) in enumerate(sizes):
        assert first[i + 1] - first[i] == -(-w // 64) * -(-h // 16)
        assert pixel0[i + 1] - pixel0[i] == w * h
    assert list(np.diff(first)) == [1, 1, 2, 2, 9 * 17, 30 * 68, 19, 5]
    # 64 maps of 46340 x 46340 would need more tiles than a launch has workgroups
    big = [(D, 0, 0, 0, 46340, 46340)] * 64
    first, pixel0, fits = SL.tiles(big)
    assert first[-1] == 64 * 725 * 2897 and pixel0[-1] == 64 * 46340 * 46340 and fits
    assert SL.tiles([(D, 0, 0, 0, 1, 2 ** 30)] * 32)[2] is False         # 2^26 tiles each: 2^31 in all


def test_layout():
    k = SL.constants()
    n, n_tiles, n_pixels = 3, 1000, 640 * 480 + 96 * 80 + 1
    l = SL.layout(n, n_tiles, n_pixels)
    order = ["result", "items", "first", "partials", "labels", "sizes"]
    need = [k["result_bytes"], n * k["item_bytes"], (n + 1) * 4, n_tiles * k["partial_bytes"], n_pixels * 4, n_pixels * 4]
    at = 0
    for name, bytes_ in zip(order, need):
        assert l[name] == at and at % 256 == 0, name
        if name == "partials":
            assert l["staged"] == at                                          # what travels through the staging ends where the partials begin
        at += (bytes_ + 255) // 256 * 256
    assert l["bytes"] == at
    # 8 B per pixel of the batch, and a little
    big = SL.layout(32, 32 * 30 * 68, 32 * 1920 * 1080)
    assert 0 <= big["bytes"] - 8 * 32 * 1920 * 1080 < (1 << 21)


def test_host_entry_refuses_like_the_plan():
    d = np.ones((8, 8), np.float32); before = d.copy()
    for w, h, dp, np_, thr in ((0, 8, d.ctypes.data, 0, THR), (8, 8, 0, 0, THR), (8, 8, d.ctypes.data, 0, float("nan")), (8, 8, d.ctypes.data, 0, 0.0),
                               (8, 8, d.ctypes.data, d.ctypes.data, THR)):
        rc, _ = binding.remove_speckles_raw(w, h, dp, np_, 0, 0, thr, 100)
        assert rc == binding.ERR_INVALID
    assert np.array_equal(d, before)
    out = binding.remove_speckles(d, speckle_size=65)
    assert out["stats"]["n_removed"] == 64 and not out["depth"].any() and np.array_equal(d, before)

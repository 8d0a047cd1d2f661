"""The sweep launch plan (hc-mvs_amd/csrc/sweep_plan.h) on the CPU: which kernel instance, how many launches, what a ticket is, for
batches whose answers follow by hand from the rules.  tests/sweep_plan_shim.cpp is compiled with g++ alone: no HIP, no library."""
import itertools

import pytest

import sweep_plan_lib
from sweep_plan_lib import AUTO, FLAGS, ONE, PER_SWEEP, image, plan, resolve  # noqa: F401


@pytest.fixture(scope="module")
def lib():
    return sweep_plan_lib.load()


def check(pl, n_launches, count, nw, segLen, tickets, grid, **flags):
    """every launch of pl: `count` sweeps with the given instance and tickets; the launches follow each other"""
    assert len(pl) == n_launches
    for i, l in enumerate(pl):
        assert l["first"] == i * count and l["count"] == count
        assert (l["nw"], l["segLen"], l["tickets"], l["grid"]) == (nw, segLen, tickets, grid), l
        for f in FLAGS:
            assert l[f] == flags.get(f, False), (f, l)
        assert l["exists"]


HD = image(1920, 1080)  # 1066 rows, 1906 columns: 8 stretches of 256


def test_rows_of_the_test_images():
    assert HD[:2] == (1066, 1906) and image(3840, 2160)[:2] == (2146, 3826)


@pytest.mark.parametrize("n, nw, tickets", [(1, 3, 8528), (2, 2, 17056), (3, 2, 25584), (4, 1, 34112), (11, 1, 93808)])
def test_few_images_one_launch_per_sweep_in_stretches(lib, n, nw, tickets):
    check(plan(lib, [HD] * n), 8, 1, nw, 256, tickets, 8192)


def test_twelve_images_one_launch(lib):
    check(plan(lib, [HD] * 12), 1, 8, 1, 0, 12792, 8192)
    check(plan(lib, [HD] * 12, launches=PER_SWEEP), 8, 1, 1, 0, 12792, 8192)


def test_three_images_forced_into_one_launch(lib):
    check(plan(lib, [HD] * 3, launches=ONE), 1, 8, 2, 0, 3198, 3198)


def test_one_4k_image(lib):
    check(plan(lib, [image(3840, 2160)]), 8, 1, 2, 256, 2146 * 15, 8192)


def test_hint_in_the_last_sweep_one_image(lib):
    """three waves requested: the hint sweep runs two, and still in stretches (the rule counts the requested waves)"""
    pl = plan(lib, [image(1920, 1080, hint=True)])
    check(pl[:7], 7, 1, 3, 256, 8528, 8192)
    last = pl[7:]
    assert len(last) == 1 and (last[0]["first"], last[0]["count"]) == (7, 1)
    last[0]["first"] = 0
    check(last, 1, 1, 2, 256, 8528, 8192, hint=True)


def test_hint_in_the_last_sweep_twelve_images(lib):
    pl = plan(lib, [HD] * 11 + [image(1920, 1080, hint=True)])
    assert len(pl) == 2 and (pl[1]["first"], pl[1]["count"]) == (7, 1)
    check(pl[:1], 1, 7, 1, 0, 12792, 8192)
    pl[1]["first"] = 0
    check(pl[1:], 1, 1, 1, 0, 12792, 8192, hint=True)
    check(plan(lib, [image(1920, 1080, hint=True)] * 12, n_sweeps=1), 1, 1, 1, 0, 12792, 8192, hint=True)


def test_mixed_sizes_and_view_counts(lib):
    items = [image(136, 72, 8), image(88, 104, 3), image(120, 80, 8)]  # adapthalfwin 6: border 7
    assert [i[:2] for i in items] == [(58, 122), (90, 74), (66, 106)]
    kw = dict(n_sweeps=3, launches=PER_SWEEP, waves=2)
    check(plan(lib, items, segment=40, **kw), 3, 1, 2, 40, 58 * 4 + 90 * 2 + 66 * 3, 610, pack=True)
    check(plan(lib, items, segment=5, **kw), 3, 1, 2, 32, 58 * 4 + 90 * 3 + 66 * 4, 766, pack=True)


def test_flags_of_any_item_select_the_instance(lib):
    items = [HD, image(1920, 1080, mask=True), image(1920, 1080, spread=True)]
    check(plan(lib, items), 8, 1, 2, 256, 25584, 8192, mask=True, spread=True)
    # the big patch: border 10 (1060 rows, 1900 columns), 2048 workers -> two waves, 2 * 1060 > 2048 -> stretches
    check(plan(lib, [image(1920, 1080, 12, border=10)], big=True), 8, 1, 2, 256, 1060 * 8, 8192, big=True, two=True, pack=True)


def test_selecting_view_count(lib):
    """the n_src of the LAST item whose count packs, else of item 0"""
    def sel(*vs):
        return plan(lib, [image(1920, 1080, v) for v in vs], n_sweeps=1)[0]
    assert sel(8, 6, 8)["pack"] and not sel(8, 7)["pack"] and not sel(7, 8)["pack"]
    assert sel(16, 12, 9)["pack"] and sel(16, 12, 9)["two"] and not sel(16, 15)["pack"] and sel(16, 15)["two"]


def test_resolve_sweep_variant(lib):
    for V in range(1, 17):
        v = resolve(lib, 1, V)
        assert v["pack"] == (V not in (7, 8, 15, 16)) and v["two"] == (V >= 9)
        assert lib.sp_segments_for(V) == (8 if V <= 8 else 4)
    for mask in (False, True):
        assert [resolve(lib, r, 8, mask=mask)["nw"] for r in (1, 2, 3, 4)] == [1, 2, 3, 4]
        assert [resolve(lib, r, 8, mask=mask, spread=True)["nw"] for r in (1, 2, 3, 4)] == [1, 2, 3, 3]
        for spread in (False, True):
            for big, hint in ((True, False), (False, True), (True, True)):
                assert [resolve(lib, r, 8, big, hint, mask, spread)["nw"] for r in (1, 2, 3, 4)] == [1, 2, 2, 2]
    for r in (-1, 0, 5, 6, 64):  # (the knobs cannot produce one; the rule is kept)
        for big, hint, spread in itertools.product((False, True), repeat=3):
            assert resolve(lib, r, 8, big, hint, False, spread)["nw"] == (1 if r < 2 and (big or hint) else 2)
    v = resolve(lib, 3, 12, big=True, hint=True, mask=True, spread=True)
    assert all(v[f] for f in ("big", "two", "hint", "mask", "spread", "pack", "exists"))


def test_instance_set(lib):
    """nw 1..4; at most 2 with big or hint; at most 3 with spread: 152 of the 256 combinations (and nothing outside 1..4 waves)"""
    n = 0
    for nw in range(0, 6):
        for big, two, pack, hint, mask, spread in itertools.product((0, 1), repeat=6):
            want = 1 <= nw <= 4 and (nw <= 2 or not (big or hint)) and (nw <= 3 or not spread)
            assert bool(lib.sp_exists(nw, big, two, pack, hint, mask, spread)) == want
            n += want
    assert n == 152


def test_every_plan_the_knobs_allow(lib):
    """1..32 items of a few sizes, both view classes, all flag combinations, the three launch modes, waves automatic and 1..4: every
    planned instance exists, the launches tile [0, nSweeps) in order, a hint launch is one sweep and the last, no sweeps: no launch"""
    sizes = [(1920, 1080), (3840, 2160), (640, 480), (96, 80)]
    n_plans = 0
    for n in (1, 2, 3, 4, 5, 8, 11, 12, 16, 31, 32):
        for si, views in itertools.product(range(len(sizes)), ((8, 3, 7), (16, 12, 15))):
            for big, hint, mask, spread in itertools.product((False, True), repeat=4):
                border = 10 if big else 7
                items = [image(*sizes[(si + i % 2) % len(sizes)], views[i % 3], border, hint and i == n - 1, mask and i == 0, spread and i == n // 2)
                         for i in range(n)]
                for launches, waves, segment, n_sweeps in itertools.product((AUTO, PER_SWEEP, ONE), range(5), (-1, 0, 100), (0, 1, 2, 8)):
                    pl = plan(lib, items, n_sweeps, big, 256, launches, segment, waves)
                    n_plans += 1
                    assert (n_sweeps == 0) == (len(pl) == 0)
                    at = 0
                    for i, l in enumerate(pl):
                        assert l["exists"] and l["first"] == at and l["count"] >= 1
                        assert (l["big"], l["mask"], l["spread"], l["two"]) == (big, mask, spread, views[0] > 8)
                        assert l["hint"] == (hint and i == len(pl) - 1) and (not l["hint"] or l["count"] == 1)
                        assert 1 <= l["grid"] == min(l["tickets"], 8192)
                        at += l["count"]
                    assert at == n_sweeps
    assert n_plans > 10000

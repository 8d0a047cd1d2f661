"""The ledger of tests/sweep_matrix.py, on the CPU: which sweep-kernel instances and launch shapes the matrix of
test_gpu_sweep_matrix.py launches, read from the launch plan (hc-mvs_amd/csrc/sweep_plan.h through tests/sweep_plan_shim.cpp, g++ alone).
It must be EVERY plain instance the library holds (MASK = SPREAD = false: 40 of the 152) in every shape plan_sweeps can give it, so that a
later change to plan_sweeps or to the matrix cannot silently drop an instance from the GPU's oracle coverage.  The other 112 (MASK, SPREAD,
MASK + SPREAD) have the same ledger in test_sweep_matrix_flavours_plan.py, which also asserts that the four together are all 152: every
instance the library holds is pinned to the oracle."""
import itertools

import pytest

import sweep_matrix as M
import sweep_plan_lib as P


@pytest.fixture(scope="module")
def lib():
    return P.load()


def shape(l):
    return (l["nw"], l["big"], l["two"], l["pack"], l["hint"], l["count"] >= 2, l["segLen"] > 0)


def test_the_sizes_are_what_the_matrix_is_built_on(lib):
    assert [i[:2] for i in M.plan_items((0, 0, 1, 0))] == [(58, 74), (74, 58), (42, 90)]
    assert [i[:2] for i in M.plan_items((1, 0, 1, 0))] == [(52, 68), (68, 52), (36, 84)]
    for cls in M.CLASSES:
        items = M.plan_items(cls)
        assert [-(-i[1] // 32) for i in items] == [3, 2, 3] and all(i[1] % 32 for i in items)     # stretches per row; the last one is shorter
        assert len({i[0] for i in items}) == 3                                                    # three row counts
        assert [bool(i[3]) for i in items] == [bool(cls[3]), False, bool(cls[3])]                 # item 1 never carries a hint
        assert all((i[2] > 8) == bool(cls[1]) for i in items)
        assert any(i[2] % 8 not in (0, 7) for i in items) == bool(cls[2])      # view_count_packs of some item


def test_the_matrix_launches_every_plain_instance_in_every_shape(lib):
    seen = set()
    n_configs = 0
    for cls in M.CLASSES:
        big, two, pack, hint = (bool(x) for x in cls)
        cfgs = M.configs(lib, cls)
        assert len(cfgs) == (8 if big else 16), (cls, cfgs)       # a big-patch launch resolves 3 and 4 waves to 2
        assert len(set(cfgs)) == len(cfgs)
        n_configs += len(cfgs)
        for launches, segment, waves in cfgs:
            pl = M.class_plan(lib, cls, launches, segment, waves)
            at = 0
            for l in pl:
                assert l["exists"], (cls, launches, segment, waves, l)
                assert not l["mask"] and not l["spread"] and (l["big"], l["two"], l["pack"]) == (big, two, pack)
                assert l["first"] == at and (l["segLen"] > 0) == (segment > 0)
                at += l["count"]
                seen.add(shape(l))
            assert at == M.N_SWEEPS
            assert [l["hint"] for l in pl] == [False] * (len(pl) - 1) + [hint]
            if launches == "per-sweep":
                assert [l["count"] for l in pl] == [1] * M.N_SWEEPS
            elif hint:     # sweeps 0-1 without the hint, sweep 2 with it
                assert [(l["first"], l["count"], l["hint"]) for l in pl] == [(0, 2, False), (2, 1, True)]
            else:
                assert [(l["first"], l["count"]) for l in pl] == [(0, M.N_SWEEPS)]
    assert n_configs == 192
    want = set()
    n_instances = 0
    for nw, big, two, pack, hint in itertools.product(range(0, 6), *[(False, True)] * 4):
        if not lib.sp_exists(nw, big, two, pack, hint, 0, 0):
            continue
        n_instances += 1
        for several, stretches in itertools.product((False, True), repeat=2):
            if not (hint and several):                     # a hint launch always holds one sweep
                want.add((nw, big, two, pack, hint, several, stretches))
    assert n_instances == 40 and len(want) == 24 * 4 + 16 * 2 == 128
    assert seen == want, "missing %s, extra %s" % (sorted(want - seen), sorted(seen - want))


def test_the_batch_of_many_small_images_has_more_tickets_than_the_chip_holds_workgroups(lib):
    """256 CUs x 12 sweep workers is plan_sweeps' own model of what is resident (`slots`); nobody has measured it"""
    for launches, waves in itertools.product(M.LAUNCHES, (3, 4)):
        pl = P.plan(lib, M.many_plan_items(), M.N_SWEEPS, False, 256, M.LAUNCH_KNOB[launches], 32, waves)
        assert len(pl) == (3 if launches == "per-sweep" else 1)
        for l in pl:
            assert l["exists"] and l["nw"] == waves and l["segLen"] == 32 and l["tickets"] * l["nw"] > 256 * 12
    assert len({M.many_size(i) for i in range(M.MANY)}) == M.MANY and M.MANY <= 64

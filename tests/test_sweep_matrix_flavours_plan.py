"""The ledger of tests/sweep_matrix_flavours.py, on the CPU: which MASK, SPREAD and MASK + SPREAD sweep-kernel instances and launch
shapes the matrix of test_gpu_sweep_matrix_flavours.py launches, read from the launch plan through the shim as test_sweep_matrix_plan.py
reads the plain ones.  It must be every one of the 112 such instances in every shape plan_sweeps can give it; with the 40 plain ones of
test_sweep_matrix_plan.py that is ALL 152 instances the library holds.

It also holds what makes the masked batches tests of estimation and not of empty maps: each mask keeps at least half of the inside
pixels and the oracle's depth is positive on more than 0.3 of the kept ones (the plain matrix's own bar); and that in the classes with
9..16 views the second view set of item 2 holds views that offer maps and views that do not."""
import itertools

import numpy as np
import pytest

import sweep_matrix as M
import sweep_matrix_flavours as F
import sweep_plan_lib as P
from sweep_matrix_run import want

N_CONFIGS = {"mask": 192, "spread": 160, "mask+spread": 160}      # a spread launch resolves 4 waves to 3
N_INSTANCES = {"mask": 40, "spread": 36, "mask+spread": 36}
N_SHAPES = {"mask": 128, "spread": 112, "mask+spread": 112}


@pytest.fixture(scope="module")
def lib():
    return P.load()


def shape(l):
    return (l["nw"], l["big"], l["two"], l["pack"], l["hint"], l["count"] >= 2, l["segLen"] > 0)


def instances(lib, mask, spread):
    return [v for v in itertools.product(range(0, 6), *[(False, True)] * 4) if lib.sp_exists(*v, int(mask), int(spread))]


@pytest.mark.parametrize("fl", F.FLAVOURS)
def test_the_matrix_launches_every_instance_of_the_flavour_in_every_shape(lib, fl):
    mask, spread = F.has_mask(fl), F.has_spread(fl)
    seen = set()
    n_configs = 0
    for cls in M.CLASSES:
        big, two, pack, hint = (bool(x) for x in cls)
        items = F.plan_items(fl, cls)
        assert [i[:4] for i in items] == [i[:4] for i in M.plan_items(cls)]                       # the plain class's sizes, views and hints
        assert [i[4:] for i in items] == [(int(mask), int(spread)), (0, 0), (int(mask), int(spread))]     # item 1 stays plain
        cfgs = F.configs(lib, fl, cls)
        assert len(cfgs) == (8 if big else 12 if spread else 16), (fl, cls, cfgs)
        assert len(set(cfgs)) == len(cfgs)
        n_configs += len(cfgs)
        for launches, segment, waves in cfgs:
            pl = F.class_plan(lib, fl, cls, launches, segment, waves)
            at = 0
            for l in pl:
                assert l["exists"], (fl, cls, launches, segment, waves, l)
                assert (l["mask"], l["spread"]) == (mask, spread) and (l["big"], l["two"], l["pack"]) == (big, two, pack)
                assert l["nw"] == min(waves, 2 if big or l["hint"] else 3 if spread else 4)
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
    assert n_configs == N_CONFIGS[fl]
    want_shapes = set()
    inst = instances(lib, mask, spread)
    for nw, big, two, pack, hint in inst:
        for several, stretches in itertools.product((False, True), repeat=2):
            if not (hint and several):                     # a hint launch always holds one sweep
                want_shapes.add((nw, big, two, pack, hint, several, stretches))
    assert len(inst) == N_INSTANCES[fl] and len(want_shapes) == N_SHAPES[fl]
    assert seen == want_shapes, "missing %s, extra %s" % (sorted(want_shapes - seen), sorted(seen - want_shapes))


def test_the_plain_matrix_and_the_flavours_account_for_all_152_instances(lib):
    every = [v for v in itertools.product(range(0, 6), *[(False, True)] * 6) if lib.sp_exists(*(int(x) for x in v))]
    assert len(every) == 152
    pinned = [v + (m, s) for m, s in itertools.product((False, True), repeat=2) for v in instances(lib, m, s)]
    assert sorted(pinned) == sorted(every)
    assert len(instances(lib, False, False)) == 40 and sum(N_INSTANCES.values()) == 112
    assert sum(N_CONFIGS.values()) == 512 and sum(N_SHAPES.values()) == 352


def test_the_masks_hold_the_edges_they_are_built_for():
    for cls in ((0, 0, 1, 0), (1, 0, 1, 0)):
        b = M.border(M.adapthalfwin(cls))
        s0, _, s2 = F.class_scenes("mask", cls)
        (w, h) = M.SIZES[0]
        nrows, ncols = h - 2 * b, w - 2 * b
        k = s0["keep"][b:h - b, b:w - b]
        assert s0["labels"].shape == (h, w) and s0["labels"].dtype == np.uint16
        for q in (0, 31, 32, ncols - 33, ncols - 32, ncols - 1):
            assert not k[:nrows // 2, q].any()
        assert k[nrows // 2:, [0, 31, 32, ncols - 1]].any()                           # (the upper half only)
        r0, r1 = F.blank_rows(nrows)
        assert r1 == r0 + 1 and r0 > nrows // 2 and r1 < nrows - 2 and not k[r0:r1 + 1].any() and k[r0 - 1].any() and k[r1 + 1].any()
        assert not k[nrows - 1].any() and not s0["keep"][:b].any()
        assert set(np.unique(s0["labels"])) >= {0, 3, 4, 5} and (s0["keep"][s0["labels"] == 5] == 1).all()      # a label that is not ignored
        (w, h) = M.SIZES[2]
        assert s2["labels"].shape == (h // 2, w // 2)
        assert not s2["keep"][b, :].any() and s2["keep"][b + 2, :].any()             # inside row 0 is masked, through the resampling
        assert F.class_scenes("mask", cls)[1].get("keep") is None


@pytest.mark.parametrize("cls", M.CLASSES, ids=M.class_id)
@pytest.mark.parametrize("fl", [f for f in F.FLAVOURS if F.has_mask(f)])
def test_the_masked_items_are_still_estimates(fl, cls):
    b = M.border(M.adapthalfwin(cls))
    kw = F.params(fl, cls)
    for i, (sc, off) in enumerate(zip(F.class_scenes(fl, cls), M.SEED_OFFSETS)):
        assert (sc.get("keep") is not None) == F.flavoured(i)
        if not F.flavoured(i):
            continue
        kept = F.kept_share(sc["keep"], b)
        depth = want(F.want_key(fl, cls, i), sc, kw, off)[0]
        pos = F.positive_share(depth, sc["keep"], b)
        print("%s %s item %d: kept %.3f of the inside, depth > 0 on %.3f of the kept pixels" % (fl, M.class_id(cls), i, kept, pos))
        assert kept >= 0.5
        assert pos > 0.3


def test_the_second_view_set_of_item_2_holds_views_that_offer_and_views_that_do_not():
    for fl, cls in itertools.product([f for f in F.FLAVOURS if F.has_spread(f)], M.CLASSES):
        s0, s1, s2 = F.class_scenes(fl, cls)
        assert all(m is not None for m in s0["maps"]) and s1.get("maps") is None and s1["spread"]
        offers = [m is not None for m in s2["maps"]]
        assert len(offers) == M.VIEWS[cls[1:3]][2] and offers == [v % 2 == 0 for v in range(len(offers))]
        if cls[1]:
            assert any(offers[8:]) and not all(offers[:8])
        for m, v in zip(s2["maps"], s2["views"][1:]):        # a view spreads only with maps of its own size
            assert m is None or m[0].shape == v["gray"].shape
        conf = np.concatenate([m[2].ravel() for m in s0["maps"]])
        assert (conf < 0.3).any() and (conf > 0.6).any() and ((s0["maps"][0][0] == 0).mean() > 0.05)


def test_the_edge_batches(lib):
    """the 17-image batch still has more tickets than the plan's model of resident workgroups; the batch with a blank middle item and the
    one-sweep plan are what test_gpu_sweep_matrix_flavours.py says they are"""
    assert sum(F.many_masked(i) for i in range(M.MANY)) == 6 and sum(F.many_offers(i) for i in range(M.MANY)) == 9
    assert any(F.many_masked(i) and F.many_offers(i) for i in range(M.MANY)) and any(not F.many_masked(i) and not F.many_offers(i) for i in range(M.MANY))
    for launches in M.LAUNCHES:
        pl = P.plan(lib, F.many_plan_items(), M.N_SWEEPS, False, 256, M.LAUNCH_KNOB[launches], 32, 3)
        assert len(pl) == (3 if launches == "per-sweep" else 1)
        for l in pl:
            assert l["exists"] and l["mask"] and l["spread"] and l["nw"] == 3 and l["segLen"] == 32 and l["tickets"] * l["nw"] > 256 * 12
    cls = (0, 0, 1, 1)
    pl = F.class_plan(lib, "mask+spread", cls, "one", 32, 2, 1)
    assert [(l["first"], l["count"], l["hint"], l["mask"], l["spread"]) for l in pl] == [(0, 1, True, True, True)]
    items = F.blank_middle_plan_items((0, 0, 1, 0))
    assert [i[4:] for i in items] == [(0, 0), (1, 0), (0, 0)]

"""Every MASK, SPREAD and MASK + SPREAD sweep-kernel instance (what --ignore-mask-label and --n-viewspread 1 run) in every launch shape
against the CPU oracle, bit for bit: depth, normal, confidence, the evaluation count, the number of sweep launches and, with view spread,
its four counters.

tests/sweep_matrix_flavours.py holds the cases: the 16 classes and the knob grid of the plain matrix (test_gpu_sweep_matrix.py) in three
flavours -- 192 + 160 + 160 configurations after those with equal plans are dropped.  test_sweep_matrix_flavours_plan.py shows on the
CPU that these launch each of the 112 instances in each of its launch shapes.  These instances differ from the plain ones in the row
pipeline's synchronisation, not only in arithmetic: a masked pixel writes the row's ring and publishes its column by hand, and the
view-spread block runs in every wave of a row and hands its masks on to the hint.

Then the edges outside the matrix, as in the plain module: more tickets than the chip holds workgroups, HCMVS_SWEEP_LAG, ragged and
over-long stretches, one sweep in one launch -- and an item that is masked everywhere, whose rows only publish.

Every configuration gets a fresh Context (sweep_matrix_run.run); the oracle runs once per item.  Most of the module's time is the CPU
oracle's, not the GPU's: with view spread it scores every slot of every offering view against all views, so the first cell of a class
with 16 views that all offer maps pays for 8 to 10 s of oracle once; the other cells of the class take well under a second."""
import pytest

import sweep_matrix as M
import sweep_matrix_flavours as F
import sweep_plan_lib as P
from sweep_matrix_run import run, want

pytestmark = pytest.mark.gpu


def _knobs(launches, segment, waves, **more):
    k = {"HCMVS_SWEEP_LAUNCHES": launches, "HCMVS_SWEEP_SEGMENT": segment, "HCMVS_WAVES_PER_ROW": waves}
    k.update(more)
    return k


def _run_class(monkeypatch, fl, cls, launches, segment, waves, kw=None, **more):
    kw = kw or F.params(fl, cls)
    scenes = F.class_scenes(fl, cls)
    wants = [want(F.want_key(fl, cls, i), sc, kw, off) for i, (sc, off) in enumerate(zip(scenes, M.SEED_OFFSETS))]
    pl = F.class_plan(P.load(), fl, cls, launches, segment, waves, kw["n_estimation_iters"])
    run(monkeypatch, scenes, wants, M.SEED_OFFSETS, kw, _knobs(launches, segment, waves, **more), len(pl), "%s %s " % (fl, M.class_id(cls)))
    return wants


@pytest.mark.parametrize("segment", M.SEGMENTS)
@pytest.mark.parametrize("launches", M.LAUNCHES)
@pytest.mark.parametrize("cls", M.CLASSES, ids=M.class_id)
@pytest.mark.parametrize("fl", F.FLAVOURS)
def test_matrix(fl, cls, launches, segment, monkeypatch):
    waves = [w for l, s, w in F.configs(P.load(), fl, cls) if (l, s) == (launches, segment)]
    assert waves == ([1, 2] if cls[0] else [1, 2, 3] if F.has_spread(fl) else [1, 2, 3, 4])
    for w in waves:
        wants = _run_class(monkeypatch, fl, cls, launches, segment, w)
    b = M.border(M.adapthalfwin(cls))
    for sc, w in zip(F.class_scenes(fl, cls), wants):      # (the oracle's maps are estimates, not empty maps)
        if sc.get("keep") is None:
            assert (w[0][b:-b, b:-b] > 0).mean() > 0.3
        else:
            assert F.kept_share(sc["keep"], b) >= 0.5 and F.positive_share(w[0], sc["keep"], b) > 0.3


@pytest.mark.parametrize("launches", M.LAUNCHES)
def test_more_tickets_than_the_chip_holds_workgroups(launches, monkeypatch):
    """the 17 small images of the plain module in stretches of 32 columns with 3 waves per row, every third one masked and the source
    views of every second one offering maps: workgroups start late and loop over tickets of several images and sweeps"""
    kw = F.many_params()
    scenes = [F.many_scene(i) for i in range(M.MANY)]
    offsets = [M.many_seed_offset(i) for i in range(M.MANY)]
    wants = [want(("many", "mask+spread", i), sc, kw, off) for i, (sc, off) in enumerate(zip(scenes, offsets))]
    pl = P.plan(P.load(), F.many_plan_items(), M.N_SWEEPS, False, 256, M.LAUNCH_KNOB[launches], 32, 3)
    assert all(l["tickets"] * l["nw"] > 256 * 12 and l["nw"] == 3 and l["mask"] and l["spread"] for l in pl)
    run(monkeypatch, scenes, wants, offsets, kw, _knobs(launches, 32, 3), len(pl), "many ")


@pytest.mark.parametrize("segment", [0, 32])
@pytest.mark.parametrize("lag", [2, 200])
def test_sweep_lag(lag, segment, monkeypatch):
    """a masked column is published at once, an unmasked one below it waits `lag` columns; 200 is beyond every row and every stretch"""
    for launches in M.LAUNCHES:
        _run_class(monkeypatch, "mask+spread", (0, 0, 1, 0), launches, segment, 2, HCMVS_SWEEP_LAG=lag)


@pytest.mark.parametrize("segment", [33, 4096])
def test_stretch_lengths(segment, monkeypatch):
    """at 33 the masked columns 31 and 32 no longer sit on a stretch's border and every row has a ragged stretch; 4096 is one stretch per
    row with the stretch code paths on"""
    for launches in M.LAUNCHES:
        for waves in (1, 3):
            _run_class(monkeypatch, "mask+spread", (0, 1, 1, 0), launches, segment, waves)


@pytest.mark.parametrize("cls", [(0, 0, 1, 1), (0, 1, 0, 1)], ids=M.class_id)
def test_one_sweep_in_one_launch(cls, monkeypatch):
    """the only sweep is the HINT + MASK + SPREAD launch"""
    fl = "mask+spread"
    kw = dict(F.params(fl, cls), n_estimation_iters=1)
    for segment in (0, 32):
        pl = F.class_plan(P.load(), fl, cls, "one", segment, 2, 1)
        assert [(l["first"], l["count"], l["hint"]) for l in pl] == [(0, 1, True)]
        assert all(l["mask"] and l["spread"] for l in pl)
        _run_class(monkeypatch, fl, cls, "one", segment, 2, kw=kw)


@pytest.mark.parametrize("segment", [0, 32])
@pytest.mark.parametrize("launches", M.LAUNCHES)
def test_an_item_that_is_masked_everywhere(launches, segment, monkeypatch):
    """the middle item of three: its rows only publish, its rowsDone must still advance so that its later sweeps and the launch end, and
    it has no evaluation; the two unmasked items around it compute the plain matrix's maps"""
    cls = (0, 0, 1, 0)
    kw = M.params(cls)
    scenes = F.blank_middle_scenes(cls)
    wants = [want(("blank middle", cls, 1) if i == 1 else ("class", cls, i), sc, kw, off)
             for i, (sc, off) in enumerate(zip(scenes, M.SEED_OFFSETS))]
    assert not scenes[1]["keep"].any() and wants[1][3] == 0 and wants[0][3] > 0 and wants[2][3] > 0
    for waves in (1, 3):
        pl = P.plan(P.load(), F.blank_middle_plan_items(cls), M.N_SWEEPS, False, 256, M.LAUNCH_KNOB[launches], segment, waves)
        assert all(l["mask"] and not l["spread"] and l["nw"] == waves for l in pl)
        run(monkeypatch, scenes, wants, M.SEED_OFFSETS, kw, _knobs(launches, segment, waves), len(pl), "blank middle ")

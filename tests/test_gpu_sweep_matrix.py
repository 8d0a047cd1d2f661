"""Every plain sweep-kernel instance (MASK = SPREAD = false: what bench.py runs) in every launch shape against the CPU oracle, bit for bit.

tests/sweep_matrix.py holds the cases: 16 classes (big patch x 9..16 views x pair packing x restore hint), each a batch of three items of
different sizes, under HCMVS_WAVES_PER_ROW 1..4 x HCMVS_SWEEP_LAUNCHES per-sweep / one x HCMVS_SWEEP_SEGMENT 0 / 32 -- 192 configurations
after those with equal plans are dropped.  test_sweep_matrix_plan.py shows on the CPU that these launch each of the 40 plain instances in
each of its launch shapes.  One launch for all sweeps with items of different row counts is the case that mode exists for: the short image
is in sweep k + 1 while the tall ones are in k (the sweep << 16 progress tags, the rowsDone wait before a sweep's first row, pass 0 /
pass 1 of the ticket choice).

Then the edges outside the matrix: more tickets than the chip holds workgroups, 9 and 17 items with and without XCD affinity,
HCMVS_SWEEP_LAG, one sweep in one launch, no sweep at all, ragged and over-long stretches.

Every configuration gets a fresh Context (the knobs are read in hcmvs_create).  The oracle runs once per item (sweep_matrix_run.py, shared
with test_gpu_sweep_matrix_flavours.py)."""
import pytest

import sweep_matrix as M
import sweep_plan_lib as P
from sweep_matrix_run import run as _run, want as _want

pytestmark = pytest.mark.gpu

def _knobs(launches, segment, waves, **more):
    k = {"HCMVS_SWEEP_LAUNCHES": launches, "HCMVS_SWEEP_SEGMENT": segment, "HCMVS_WAVES_PER_ROW": waves}
    k.update(more)
    return k


def _run_class(monkeypatch, cls, launches, segment, waves, kw=None, **more):
    kw = kw or M.params(cls)
    scenes = M.class_scenes(cls)
    wants = [_want(("class", cls, i), sc, kw, off) for i, (sc, off) in enumerate(zip(scenes, M.SEED_OFFSETS))]
    pl = M.class_plan(P.load(), cls, launches, segment, waves, kw["n_estimation_iters"])
    _run(monkeypatch, scenes, wants, M.SEED_OFFSETS, kw, _knobs(launches, segment, waves, **more), len(pl))
    return wants


def _run_many(monkeypatch, n, launches, segment, waves, **more):
    kw = dict(adapthalfwin=M.MANY_AHW, n_estimation_iters=M.N_SWEEPS, seed=M.SEED)
    scenes = [M.many_scene(i) for i in range(n)]
    offsets = [M.many_seed_offset(i) for i in range(n)]
    wants = [_want(("many", i), sc, kw, off) for i, (sc, off) in enumerate(zip(scenes, offsets))]
    pl = P.plan(P.load(), M.many_plan_items(n), M.N_SWEEPS, False, 256, M.LAUNCH_KNOB[launches], segment, waves)
    _run(monkeypatch, scenes, wants, offsets, kw, _knobs(launches, segment, waves, **more), len(pl))
    return pl


@pytest.mark.parametrize("segment", M.SEGMENTS)
@pytest.mark.parametrize("launches", M.LAUNCHES)
@pytest.mark.parametrize("cls", M.CLASSES, ids=M.class_id)
def test_matrix(cls, launches, segment, monkeypatch):
    waves = [w for l, s, w in M.configs(P.load(), cls) if (l, s) == (launches, segment)]
    assert waves == ([1, 2] if cls[0] else [1, 2, 3, 4])
    for w in waves:
        wants = _run_class(monkeypatch, cls, launches, segment, w)
    b = M.border(M.adapthalfwin(cls))
    assert all((w[0][b:-b, b:-b] > 0).mean() > 0.3 for w in wants)      # (the oracle's maps are estimates, not empty maps)


@pytest.mark.parametrize("waves", [3, 4])
@pytest.mark.parametrize("launches", M.LAUNCHES)
def test_more_tickets_than_the_chip_holds_workgroups(launches, waves, monkeypatch):
    """17 small images in stretches of 32 columns: by the plan's own model of the chip (`slots` of plan_sweeps: 12 sweep workers on each of
    256 CUs -- how many workgroups really are resident nobody has measured) the launch has more tickets than resident workgroups, so
    workgroups start late and loop over tickets of several images and sweeps"""
    pl = _run_many(monkeypatch, M.MANY, launches, 32, waves)
    assert all(l["tickets"] * l["nw"] > 256 * 12 and l["nw"] == waves for l in pl)


@pytest.mark.parametrize("affinity", [1, 0])
@pytest.mark.parametrize("launches", M.LAUNCHES)
@pytest.mark.parametrize("n", [9, 17])
def test_more_than_eight_items(n, launches, affinity, monkeypatch):
    """with XCD affinity a workgroup maps the images that are not its home images to indices; without, it picks in rotation"""
    _run_many(monkeypatch, n, launches, 0, 1, HCMVS_XCD_AFFINITY=affinity)


@pytest.mark.parametrize("segment", [0, 32])
@pytest.mark.parametrize("lag", [2, 5, 200])
def test_sweep_lag(lag, segment, monkeypatch):
    """columns the row above must be ahead before a row starts; 200 is beyond every row and every stretch: the end of the stretch then"""
    for launches in M.LAUNCHES:
        _run_class(monkeypatch, (0, 0, 1, 0), launches, segment, 2, HCMVS_SWEEP_LAG=lag)


@pytest.mark.parametrize("segment", [33, 4096])
def test_stretch_lengths(segment, monkeypatch):
    """33 leaves a ragged stretch in every row; 4096 is one stretch per row with the stretch code paths on"""
    for launches in M.LAUNCHES:
        for waves in (1, 3):
            _run_class(monkeypatch, (0, 1, 1, 0), launches, segment, waves)


@pytest.mark.parametrize("cls", [(0, 0, 1, 0), (0, 0, 1, 1)], ids=M.class_id)
def test_one_sweep_in_one_launch(cls, monkeypatch):
    """with a hint that one sweep is the hint launch"""
    kw = dict(M.params(cls), n_estimation_iters=1)
    for segment in (0, 32):
        pl = M.class_plan(P.load(), cls, "one", segment, 2, 1)
        assert [(l["first"], l["count"], l["hint"]) for l in pl] == [(0, 1, bool(cls[3]))]
        _run_class(monkeypatch, cls, "one", segment, 2, kw=kw)


def test_no_sweep_at_all(monkeypatch):
    """an empty plan: the maps are those of the score pass and the end pass alone"""
    cls = (0, 0, 1, 0)
    kw = dict(M.params(cls), n_estimation_iters=0)
    for launches in M.LAUNCHES:
        assert M.class_plan(P.load(), cls, launches, 32, 2, 0) == []
        _run_class(monkeypatch, cls, launches, 32, 2, kw=kw)

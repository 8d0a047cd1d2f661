"""The speckle filter on the device (hcmvs_remove_speckles_batch_device; speckle_kernels.hip) against the numpy statement
(tests/speckle_ref.py, pinned to the host form by test_speckle_ref.py) on every case of tests/speckle_cases.py: depth, normal, conf,
the canonical labels and every counter, bit for bit.  The label buffers start out filled with a sentinel, so equality also shows
that every pixel is written."""
import importlib

import numpy as np
import pytest
import torch

import speckle_cases as SC
import speckle_ref as R

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")

DEV = torch.device("cuda", 0)
SENTINEL = -7


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


_WANT = {}


def want_of(name):
    """the statement's result of a case, with normal and conf; computed once and left unchanged"""
    if name not in _WANT:
        case = SC.by_name(name)
        n, c = SC.aux(case["depth"])
        _WANT[name] = R.remove_speckles(case["depth"], n, c, SC.thr_of(case), case["speckle_size"])
    return _WANT[name]


def dev_filter(ctx, jobs, thr, speckle_size, normal=True, conf=True, labels=True):
    """jobs: dicts(depth, normal, conf) of host arrays.  Returns (one dict(depth, normal, conf, labels) per job, the stats of the call)"""
    keep, items = [], []
    for m in jobs:
        h, w = m["depth"].shape
        d = torch.from_numpy(np.ascontiguousarray(m["depth"], np.float32)).to(DEV)
        n = torch.from_numpy(np.ascontiguousarray(m["normal"], np.float32)).to(DEV) if normal else None
        c = torch.from_numpy(np.ascontiguousarray(m["conf"], np.float32)).to(DEV) if conf else None
        l = torch.full((h, w), SENTINEL, dtype=torch.int32, device=DEV) if labels else None
        keep.append((d, n, c, l))
        items.append(dict(width=w, height=h, d_depth=d.data_ptr(), d_normal=n.data_ptr() if normal else 0, d_conf=c.data_ptr() if conf else 0,
                          d_labels=l.data_ptr() if labels else 0))
    torch.cuda.synchronize(DEV)      # the context works on a stream of its own
    st = ctx.remove_speckles_device(items, thr, speckle_size)
    out = [dict(depth=d.cpu().numpy(), normal=None if n is None else n.cpu().numpy(), conf=None if c is None else c.cpu().numpy(),
                labels=None if l is None else l.cpu().numpy()) for d, n, c, l in keep]
    return out, st


def job_of(name):
    case = SC.by_name(name)
    n, c = SC.aux(case["depth"])
    return dict(depth=case["depth"], normal=n, conf=c)


def assert_same(got, want, what, keys=("depth", "normal", "conf", "labels")):
    for key in keys:
        assert R.same_bits(got[key], want[key]), "%s: %s differs at %d elements" % (what, key, int((got[key] != want[key]).sum()))


def counters(st):
    return {k: st[k] for k in R.COUNTERS}


@pytest.mark.parametrize("name", SC.NAMES)
def test_device_equals_the_statement(ctx, name):
    case = SC.by_name(name)
    want = want_of(name)
    got, st = dev_filter(ctx, [job_of(name)], float(SC.thr_of(case)), case["speckle_size"])
    assert_same(got[0], want, name)
    assert counters(st) == want["stats"]
    assert st["device_bytes"] >= 8 * case["depth"].size and st["ms_device"] > 0


@pytest.mark.parametrize("name", ["blobs_200x50", "special_values", "serpentine_517x259"])
@pytest.mark.parametrize("normal, conf, labels", [(False, False, False), (True, False, False), (False, True, True), (False, False, True)])
def test_without_the_optional_pointers(ctx, name, normal, conf, labels):
    case = SC.by_name(name)
    want = want_of(name)
    got, st = dev_filter(ctx, [job_of(name)], float(SC.thr_of(case)), case["speckle_size"], normal, conf, labels)
    keys = ["depth"] + ["normal"] * normal + ["conf"] * conf + ["labels"] * labels
    assert_same(got[0], want, name, keys)
    assert counters(st) == want["stats"]


def test_default_threshold_and_size(ctx):
    """thr None and speckle_size left out: upstream's 0.01f * 0.7f and 100"""
    name = "blobs_200x50"
    assert SC.by_name(name)["speckle_size"] == 100 and "thr" not in SC.by_name(name)
    m = job_of(name)
    d = torch.from_numpy(m["depth"]).to(DEV)
    torch.cuda.synchronize(DEV)
    st = ctx.remove_speckles_device([dict(width=200, height=50, d_depth=d.data_ptr())])
    assert R.same_bits(d.cpu().numpy(), want_of(name)["depth"]) and counters(st) == want_of(name)["stats"]


def test_batch_equals_one_at_a_time(ctx):
    """three maps of different sizes in one call; one threshold and one size for the batch"""
    jobs = [job_of(n) for n in SC.BATCH]
    want = [R.remove_speckles(j["depth"], j["normal"], j["conf"], R.THR, 40) for j in jobs]
    got, st = dev_filter(ctx, jobs, float(R.THR), 40)
    total = {k: 0 for k in R.COUNTERS}
    for name, j, g, w in zip(SC.BATCH, jobs, got, want):
        assert_same(g, w, "batch: " + name)
        one, st1 = dev_filter(ctx, [j], float(R.THR), 40)
        assert_same(one[0], g, "alone: " + name)
        assert counters(st1) == w["stats"]
        for k in R.COUNTERS:
            total[k] = max(total[k], st1[k]) if k == "largest" else total[k] + st1[k]
    assert counters(st) == total


def test_the_largest_batch(ctx):
    """64 maps, the most a call takes: a few sizes, each map with its own content"""
    shapes = [(65, 17), (1, 40), (40, 1), (70, 33)]
    jobs = []
    for i in range(64):
        w, h = shapes[i % 4]
        d = SC.blobs(w, h, 100 + i, holes=0.2)
        n, c = SC.aux(d, i)
        jobs.append(dict(depth=d, normal=n, conf=c))
    got, st = dev_filter(ctx, jobs, float(R.THR), 12)
    total = {k: 0 for k in R.COUNTERS}
    for i, (j, g) in enumerate(zip(jobs, got)):
        w = R.remove_speckles(j["depth"], j["normal"], j["conf"], R.THR, 12)
        assert_same(g, w, "map %d" % i)
        for k in R.COUNTERS:
            total[k] = max(total[k], w["stats"][k]) if k == "largest" else total[k] + w["stats"][k]
    assert counters(st) == total and total["n_removed"] > 0


@pytest.mark.parametrize("name", ["blobs_130x70", "serpentine_517x259", "special_values"])
def test_twice_equals_once(ctx, name):
    case = SC.by_name(name)
    once, st1 = dev_filter(ctx, [job_of(name)], float(SC.thr_of(case)), case["speckle_size"])
    twice, st2 = dev_filter(ctx, [once[0]], float(SC.thr_of(case)), case["speckle_size"])
    assert_same(twice[0], once[0], name, ("depth", "normal", "conf"))
    assert st2["n_removed"] == 0 and st2["n_small"] == 0 and st2["n_valid"] == st1["n_valid"] - st1["n_removed"]


def test_two_runs_give_the_same_bits(ctx):
    jobs = [job_of(n) for n in ("blobs_200x50", "serpentine_517x259", "blobs_130x70")]
    a, sa = dev_filter(ctx, jobs, float(R.THR), 100)
    b, sb = dev_filter(ctx, jobs, float(R.THR), 100)
    for x, y in zip(a, b):
        assert_same(x, y, "second run")
    assert counters(sa) == counters(sb) and sa["device_bytes"] == sb["device_bytes"]


def test_refusals_leave_the_maps_alone(ctx):
    m = job_of("blobs_200x50")
    d = torch.from_numpy(m["depth"]).to(DEV); n = torch.from_numpy(m["normal"]).to(DEV); c = torch.from_numpy(m["conf"]).to(DEV)
    torch.cuda.synchronize(DEV)
    good = dict(width=200, height=50, d_depth=d.data_ptr(), d_normal=n.data_ptr(), d_conf=c.data_ptr())
    bad = [
        ("n_items", [good] * 65, R.THR, 100),
        ("n_items", [], R.THR, 100),
        ("size", [dict(good, width=0)], R.THR, 100),
        ("2^31", [dict(good, width=65536, height=32768)], R.THR, 100),
        ("null depth", [dict(good, d_depth=0)], R.THR, 100),
        ("threshold", [good], 0.0, 100),
        ("threshold", [good], float("nan"), 100),
        ("threshold", [good], float("inf"), 100),
        ("overlaps", [dict(good, d_conf=d.data_ptr() + 4)], R.THR, 100),
        ("overlaps", [good, dict(good, d_normal=0, d_conf=0)], R.THR, 100),
    ]
    for word, items, thr, size in bad:
        with pytest.raises(binding.HcmvsError) as e:
            ctx.remove_speckles_device(items, float(thr), size)
        assert e.value.code == binding.ERR_INVALID and "remove_speckles_batch_device" in str(e.value) and word in str(e.value), word
    torch.cuda.synchronize(DEV)
    assert R.same_bits(d.cpu().numpy(), m["depth"]) and R.same_bits(n.cpu().numpy(), m["normal"]) and R.same_bits(c.cpu().numpy(), m["conf"])
    # the context is as usable as before
    st = ctx.remove_speckles_device([good], float(R.THR), 100)
    assert counters(st) == want_of("blobs_200x50")["stats"]


def test_final_maps_of_an_estimate(ctx):
    """the maps a 96 x 80 estimate leaves on the device go through the filter there; the result is the statement applied to them"""
    views = synth.make_views(96, 80, 90.0, 3, seed=12)
    pts = synth.sparse_points(views, 80, seed=5)
    for i, v in enumerate(views):
        ctx.upload_view(900 + i, v["gray"], v["K"], v["R"], v["C"])
    d0, n0, dmin, dmax = ctx.splat_init(900, pts)
    p = binding.default_params(adapthalfwin=6, n_estimation_iters=2, seed=11)
    d, n, c = ctx.estimate(900, [901, 902, 903], p, dmin, dmax, d0, n0)
    want = R.remove_speckles(d, n, c, speckle_size=100)
    assert 0 < want["stats"]["n_removed"] < want["stats"]["n_valid"]          # the filter has work to do and leaves most of the map
    got, st = dev_filter(ctx, [dict(depth=d, normal=n, conf=c)], None, 100)
    assert_same(got[0], want, "estimate")
    assert counters(st) == want["stats"]
    print("96 x 80 estimate: %d valid, %d segments, %d small, %d pixels removed, %.3f ms" %
          (st["n_valid"], st["n_segments"], st["n_small"], st["n_removed"], st["ms_device"]))

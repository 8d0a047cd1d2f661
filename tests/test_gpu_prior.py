"""Depth priors (--n-para_prior, --sigma-prior, --n-photo2geo; DepthMap.cpp:941-954) on the GPU: estimates of reference views that carry a
prior map (hcmvs_set_depth_prior[_device] + hcmvs_set_prior_params) and the sweeps-only entry, against the oracle's prior inputs
(oracle/hcmvs_oracle.c) in device association, bit for bit -- depth, normal, conf, the evaluation count and the two prior counters.  Every
comparison with an active prior asserts on the oracle's side that the term was at work (evals_prior > 0, 50 .. 90 % of the estimated
pixels carry a usable prior), so none passes without it."""
import importlib

import numpy as np
import pytest

import oracle_lib as O
import prior_cases as PC

pytestmark = pytest.mark.gpu

binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")

KW = PC.KW
PRIOR = dict(para_prior=0.4, sigma_prior=0.2, photo2geo=1)      # the authors' schedule: --n-para_prior 0.4 --n-photo2geo 1


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def _compare(got, want, what=""):
    for g, w, n in zip(got, want, ("depth", "normal", "conf")):
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s differs at %d elements, first %s: gpu %r oracle %r" %
                                 (what, n, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))


def _params(**kw):
    pg = binding.default_params(**kw)
    po = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, **kw)
    return pg, po


_CASES = {}


def case(key, w, h, V, seed, prior=True, keep=None):
    """a scene, its start maps (one CPU outer iteration) and its prior; built once per key and left unchanged"""
    if key not in _CASES:
        views = synth.make_views(w, h, 90.0, V, seed=seed)
        d, n, c, dmin, dmax = PC.start_maps(views, seed)
        _CASES[key] = dict(views=views, d=d, n=n, c=c, dmin=dmin, dmax=dmax, prior=PC.make_prior(views[0], seed=seed) if prior else None, keep=keep)
    return _CASES[key]


_WANTS = {}


def oracle(key, cs, po, k, prior_kw, sweeps=None, start=None):
    """the oracle's answer for item k of a batch, computed once per (key, k) and shared by the tests that run the same batch"""
    if (key, k) not in _WANTS:
        p = O.Params.from_buffer_copy(po)
        p.seed = po.seed + 7 * k
        d, n, c = start if start is not None else (cs["d"], cs["n"], None)
        _WANTS[(key, k)] = PC.estimate(cs["views"], p, cs["dmin"], cs["dmax"], d, n, conf=c, prior=cs["prior"], keep=cs["keep"], sweeps=sweeps, **prior_kw)
    return _WANTS[(key, k)]


def run(ctx, key, cases, pg, po, base=0, prior_kw=PRIOR, active=True, sweeps=None, starts=None):
    """one hcmvs_estimate_batch_device (or, with sweeps = (first, n), one hcmvs_estimate_sweeps_batch_device) over the cases against the
    oracle.  Priors are registered from the host for even items, as device memory for odd ones.  active: the batch has an item
    whose prior is active.  Returns (stats, prior stats, the GPU's maps)."""
    import torch
    dev = torch.device("cuda:0")
    ctx.set_viewspread(False)
    ctx.set_prior_params(**prior_kw)
    items, held, wants = [], [], []
    vid = base
    est = 0
    for k, cs in enumerate(cases):
        views = cs["views"]
        ids = list(range(vid, vid + len(views)))
        vid += len(views)
        for i, v in zip(ids, views):
            ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"])
        if cs["prior"] is None:
            ctx.set_depth_prior(ids[0], None)
        elif k % 2 == 0:
            ctx.set_depth_prior(ids[0], cs["prior"])
        else:
            tp = torch.from_numpy(cs["prior"]).to(dev); held.append(tp)
            ctx.set_depth_prior_device(ids[0], tp.data_ptr())
        if cs["keep"] is not None:
            ctx.set_ignore_mask(ids[0], np.where(cs["keep"], 0, 3).astype(np.uint16), [3])
        start = None if starts is None else starts[k]
        want = oracle(key, cs, po, k, prior_kw, sweeps, start)
        wants.append(want)
        if cs["prior"] is not None and active:      # a condition on the inputs: the term is at work in this item
            border = max(7, pg.adapthalfwin)
            n_est = int(PC.estimated_pixels(cs["d"].shape, border, cs["keep"]).sum())
            assert want[3]["evals_prior"] > 0 and 0.5 < want[3]["pixels_prior"] / n_est < 0.9, (want[3], n_est)
        d0, n0, c0 = start if start is not None else (cs["d"], cs["n"], np.zeros_like(cs["d"]))
        td = torch.from_numpy(np.ascontiguousarray(d0)).to(dev); tn = torch.from_numpy(np.ascontiguousarray(n0)).to(dev)
        tc = torch.from_numpy(np.ascontiguousarray(c0)).to(dev)
        it = dict(ref_id=ids[0], src_ids=ids[1:], d_min=cs["dmin"], d_max=cs["dmax"], d_depth=td.data_ptr(), d_normal=tn.data_ptr(), d_conf=tc.data_ptr(),
                  seed_offset=7 * k)
        items.append((it, (td, tn, tc), ids))
    torch.cuda.synchronize()
    try:
        if sweeps is None:
            ctx.estimate_batch_device([it for it, _, _ in items], pg)
        else:
            ctx.estimate_sweeps_batch_device([it for it, _, _ in items], pg, sweeps[0], sweeps[1])
        ctx.synchronize()
        st = ctx.stats(); ps = ctx.prior_stats()
        maps = [(td.cpu().numpy(), tn.cpu().numpy(), tc.cpu().numpy()) for _, (td, tn, tc), _ in items]
    finally:
        for (it, _, ids), cs in zip(items, cases):
            ctx.set_depth_prior(ids[0], None)
            if cs["keep"] is not None:
                ctx.set_ignore_mask(ids[0], None, [])
    for i, want in enumerate(wants):
        _compare(maps[i], want[:3], "item %d" % i)
    assert st.evals == sum(w[3]["evals"] for w in wants)
    assert ps["evals_prior"] == sum(w[3]["evals_prior"] for w in wants)
    assert ps["pixels_prior"] == sum(w[3]["pixels_prior"] for w in wants)
    if not active:
        assert ps == dict(evals_prior=0, pixels_prior=0)
    return st, ps, maps


@pytest.mark.parametrize("it_external", [0, 1, 2])
@pytest.mark.parametrize("V", [1, 3, 5, 8, 10, 12])
def test_single_estimate(ctx, V, it_external):
    """the plain (8), PACK (1, 3, 5), TWO (12) and TWO + PACK (10) instances; outer iteration 0 lies below photo2geo = 1 (the plain
    instances run), 1 and 2 blend the term, and 2 of 3 ends with the end pass"""
    cs = case("single%d" % V, 96, 80, V, 10 + V)
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=it_external, n_external_iters=3, seed=40 + V, **KW)
    st, ps, _ = run(ctx, "single%d-%d" % (V, it_external), [cs], pg, po, active=it_external >= 1)
    assert (ps["evals_prior"] > 0) == (it_external >= 1)


@pytest.mark.parametrize("a", [5, 6, 7, 10])
def test_half_windows(ctx, a):
    """6 x 6, 7 x 7, 8 x 8 taps and the 11 x 11 big-patch kernels"""
    cs = case("hw%d" % a, 96, 88, 3, 30 + a)
    pg, po = _params(adapthalfwin=a, n_estimation_iters=2, it_external=1, n_external_iters=2, seed=a, **KW)
    run(ctx, "hw%d" % a, [cs], pg, po, base=100)


def twelve():
    return [case("twelve%d" % k, 88, 72, 3, 60 + k) for k in range(12)]


@pytest.mark.parametrize("mode", ["one", "per-sweep"])
@pytest.mark.parametrize("waves", [1, 2, 3, 4])
def test_waves_per_row_and_launch_modes_on_a_batch_of_twelve(waves, mode, monkeypatch):
    """one to four waves per row, all sweeps in one launch and one launch per sweep: identical maps (the oracle's are computed once)"""
    monkeypatch.setenv("HCMVS_WAVES_PER_ROW", str(waves))
    monkeypatch.setenv("HCMVS_SWEEP_LAUNCHES", mode)
    c = binding.Context(0)
    try:
        pg, po = _params(adapthalfwin=5, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=77, **KW)
        st, ps, _ = run(c, "twelve", twelve(), pg, po)
        assert st.n_sweep_launches == (1 if mode == "one" else 2)
    finally:
        c.close()


def test_batch_that_mixes_items_with_and_without_a_prior(ctx):
    cases = [case("mix%d" % k, 96, 80, 3, 80 + k, prior=k in (0, 3)) for k in range(4)]
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=5, **KW)
    run(ctx, "mix", cases, pg, po, base=200)


def test_prior_together_with_a_keep_mask(ctx):
    keep = np.ones((80, 96), np.uint8)
    keep[18:40, 30:66] = 0; keep[60:, :20] = 0
    cases = [case("keep0", 96, 80, 3, 91, keep=keep), case("keep1", 96, 80, 3, 92)]
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=2, n_external_iters=3, seed=6, **KW)
    run(ctx, "keep", cases, pg, po, base=300)


@pytest.mark.parametrize("last", [False, True])
def test_sweeps_only_entry_after_an_estimate(ctx, last):
    """the reference's two extra sweeps (indices N and N + 1) on the maps an estimate of N sweeps left, with the prior registered; on the
    last outer iteration the call ends with the end pass"""
    cases = [case("extra%d" % k, 96, 80, 3 + 2 * k, 95 + k) for k in range(2)]
    it_external = 2 if last else 1
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=4, seed=8, **KW)
    key = "extra-%d" % last
    _, _, maps = run(ctx, key + "-a", cases, pg, po, base=400)               # an estimate of N = 2 sweeps; not the last iteration: conf is the score
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=it_external, n_external_iters=3 if last else 4, seed=8, **KW)
    st, ps, _ = run(ctx, key + "-b", cases, pg, po, base=400, sweeps=(2, 2), starts=maps)
    assert st.n_sweeps == 2


def test_inactive_priors_compute_the_plain_maps(ctx):
    """with the prior removed, para_prior = 0 or photo2geo above the iteration the maps are those of the plain oracle, bit for bit"""
    cs = case("plain", 96, 80, 3, 50)
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=3, **KW)
    want = O.estimate(cs["views"], po, cs["dmin"], cs["dmax"], cs["d"], cs["n"])
    for name, kw in (("para0", dict(PRIOR, para_prior=0.0)), ("late", dict(PRIOR, photo2geo=2))):
        _, ps, maps = run(ctx, "plain-" + name, [cs], pg, po, base=500, prior_kw=kw, active=False)
        _compare(maps[0], want[:3], name)
    removed = dict(cs, prior=None)
    st, ps, maps = run(ctx, "plain-removed", [removed], pg, po, base=500, active=False)
    _compare(maps[0], want[:3], "removed")
    assert st.evals == want[3]


def test_the_two_refusals_and_the_argument_checks(ctx):
    import torch
    dev = torch.device("cuda:0")
    cs = case("refuse", 96, 80, 2, 55)
    for i, v in enumerate(cs["views"]):
        ctx.upload_view(600 + i, v["gray"], v["K"], v["R"], v["C"])
    ctx.set_prior_params(**PRIOR)
    td = torch.from_numpy(cs["d"]).to(dev); tn = torch.from_numpy(cs["n"]).to(dev); tc = torch.zeros_like(td)
    it = dict(ref_id=600, src_ids=[601, 602], d_min=cs["dmin"], d_max=cs["dmax"], d_depth=td.data_ptr(), d_normal=tn.data_ptr(), d_conf=tc.data_ptr())
    pg, _ = _params(adapthalfwin=6, n_estimation_iters=2, it_external=2, n_external_iters=3, **KW)
    ctx.set_depth_prior(600, cs["prior"])
    try:
        # the `restore` hint in effect (last outer iteration) together with an active prior
        hd = torch.from_numpy(cs["d"]).to(dev); hn = torch.from_numpy(cs["n"]).to(dev)
        with pytest.raises(binding.HcmvsError) as e:
            ctx.estimate_batch_device([dict(it, d_hint_depth=hd.data_ptr(), d_hint_normal=hn.data_ptr())], pg)
        assert e.value.code == binding.ERR_INVALID and "hint" in str(e.value) and "prior" in str(e.value)
        # view spread with maps to try together with an active prior
        ctx.set_viewspread(True)
        ctx.set_spread_maps_device(601, td.data_ptr(), tn.data_ptr(), tc.data_ptr())
        with pytest.raises(binding.HcmvsError) as e:
            ctx.estimate_batch_device([it], pg)
        assert e.value.code == binding.ERR_INVALID and "view spread" in str(e.value) and "prior" in str(e.value)
        ctx.set_spread_maps_device(601, None, None, None)
        ctx.set_viewspread(False)
        assert np.array_equal(td.cpu().numpy(), cs["d"])                      # nothing reached the device
        # the options
        for kw in (dict(para_prior=1.5), dict(para_prior=float("nan")), dict(sigma_prior=0.0), dict(photo2geo=-1)):
            with pytest.raises(binding.HcmvsError) as e:
                ctx.set_prior_params(**kw)
            assert e.value.code == binding.ERR_INVALID
        # the range of the sweeps-only entry
        for first, n in ((-1, 2), (2, 0), (62, 2)):
            with pytest.raises(binding.HcmvsError) as e:
                ctx.estimate_sweeps_batch_device([it], pg, first, n)
            assert e.value.code == binding.ERR_INVALID and "sweep" in str(e.value)
        # a view made by hcmvs_rescale_view takes no prior
        ctx.rescale_view(601, 603, 0.5)
        with pytest.raises(binding.HcmvsError) as e:
            ctx.set_depth_prior_device(603, 1 << 20)                          # (never dereferenced: refused)
        assert e.value.code == binding.ERR_INVALID and "rescale" in str(e.value)
    finally:
        ctx.set_viewspread(False)
        ctx.set_depth_prior(600, None)


# Measured on the CPU oracle (device association; the reference association gives 0.165 / 0.769): within the low-contrast region the
# fraction of pixels within 1 % of the ground truth is 0.1847 without the prior and 0.7692 with it.
EFFECT_WITHOUT, EFFECT_WITH = 0.1847, 0.7692


def test_the_prior_repairs_a_low_contrast_region(ctx):
    """one region of the reference image has its contrast scaled to 5 %, where the plain estimate is poor; the prior is the exact analytic
    depth.  The fraction of the region's pixels within 1 % of the ground truth must rise by at least half the gain measured on the oracle."""
    views = [dict(v) for v in synth.make_views(96, 80, 90.0, 3, seed=12)]
    g = views[0]["gray"].copy(); reg = (slice(24, 56), slice(28, 72))
    g[reg] = g[reg].mean() + (g[reg] - g[reg].mean()) * 0.05
    views[0]["gray"] = g.astype(np.float32)
    d, n, c, dmin, dmax = PC.start_maps(views, 0)
    gt = views[0]["depth"]
    for i, v in enumerate(views):
        ctx.upload_view(700 + i, v["gray"], v["K"], v["R"], v["C"])
    pg, _ = _params(adapthalfwin=6, n_estimation_iters=2, it_external=2, n_external_iters=3, seed=11, **KW)
    ctx.set_viewspread(False)
    ctx.set_prior_params()                                                     # the reference's defaults: 0.5, 0.2, 2
    frac = []
    for prior in (None, gt.astype(np.float32)):
        ctx.set_depth_prior(700, prior)
        dd, _, _ = ctx.estimate(700, [701, 702, 703], pg, dmin, dmax, d, n)
        ok = (dd > 0) & (np.abs(dd - gt) < 0.01 * gt)
        frac.append(float(ok[reg].mean()))
    ctx.set_depth_prior(700, None)
    print("fraction within 1 %% in the region: without %.4f, with %.4f" % tuple(frac))
    assert frac[1] - frac[0] >= 0.5 * (EFFECT_WITH - EFFECT_WITHOUT)

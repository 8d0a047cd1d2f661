"""The geometric-consistency term (--geo-consistency) on the GPU: estimates whose source views offer their maps
(hcmvs_set_spread_maps_device + hcmvs_set_geo_params) against the oracle variant (tests/oracle_geo.c) in device association, bit for bit
-- depth, normal, conf, the evaluation count and the two counters of the term.  Every comparison with the term at work checks on the
oracle's side that it is not vacuous (geo_cases.conditions): each pair class occurs, all three weights occur, and the result differs
from the plain estimate of the same inputs."""
import importlib

import numpy as np
import pytest

import geo_cases as GC
import oracle_geo_lib as G
import oracle_lib as O
import prior_cases as PC

pytestmark = pytest.mark.gpu

binding = importlib.import_module("hc-mvs_amd.binding")

KW = GC.KW
# max_px 1: with the cameras of these scenes a neighbour depth off by 20 % moves the pixel by 1 .. 2.5 px, so that `worst` pairs occur
GEO = dict(para_tapa=0.25, para_tapa2=0.15, photo2geo=1, max_px=1.0)


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


def case(key, w, h, V, seed, offers=None, keep=None, crop=(20, 12)):
    """a scene, its start maps (one CPU outer iteration), the maps its source views offer (offers: which of them, default all) and the
    thresholds under which all three weights occur; built once per key and left unchanged"""
    if key not in _CASES:
        views = GC.make_views(w, h, V, seed, crop=crop)
        d, n, dmin, dmax = GC.start(views, seed)
        maps = [GC.neighbour_maps(v, seed + i) if offers is None or offers[i] else None for i, v in enumerate(views[1:])]
        _CASES[key] = dict(views=views, d=d, n=n, dmin=dmin, dmax=dmax, maps=maps, keep=keep, tx=GC.thresholds(views[0]["gray"]))
    return _CASES[key]


_WANTS = {}


def oracle(key, cs, po, k, geo):
    """the oracle variant's answer for item k of a batch and the plain estimate of the same inputs, computed once per (key, k)"""
    if (key, k) not in _WANTS:
        p = O.Params.from_buffer_copy(po)
        p.seed = po.seed + 7 * k
        maps = cs["maps"] if any(m is not None for m in cs["maps"]) else None
        want = G.estimate(cs["views"], p, cs["dmin"], cs["dmax"], cs["d"], cs["n"], maps=maps, geo=geo, keep=cs["keep"])
        plain = G.estimate(cs["views"], p, cs["dmin"], cs["dmax"], cs["d"], cs["n"], keep=cs["keep"])
        _WANTS[(key, k)] = (want, plain)
    return _WANTS[(key, k)]


def run(ctx, key, cases, pg, po, base=0, geo=GEO, tx=None, at_work=True, three_weights=True):
    """one hcmvs_estimate_batch_device over the cases against the oracle variant.  tx: the two texture thresholds (default: the first
    case's, under which all three weights occur).  at_work: the term blends in every item whose source views offer maps, and the
    conditions on the inputs hold there; otherwise the maps equal the plain estimate and the counters are zero.
    Returns (stats, geo stats, the GPU's maps)."""
    import torch
    dev = torch.device("cuda:0")
    tx = tx if tx is not None else cases[0]["tx"]
    geo = dict(geo, on=1, txthreshold=tx[0], txthreshold2=tx[1]) if geo is not None else None
    ctx.set_viewspread(False)
    if geo is not None:
        ctx.set_geo_params(**geo)
    else:
        ctx.set_geo_params(on=False)
    items, held, wants, ids_all = [], [], [], []
    vid = base
    for k, cs in enumerate(cases):
        views = cs["views"]
        ids = list(range(vid, vid + len(views)))
        vid += len(views)
        ids_all += ids
        for i, v in zip(ids, views):
            ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"])
        for i, m in zip(ids[1:], cs["maps"]):
            if m is None:
                ctx.set_spread_maps_device(i, None, None, None)
                continue
            t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in m]
            held.append(t)
            ctx.set_spread_maps_device(i, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
        if cs["keep"] is not None:
            ctx.set_ignore_mask(ids[0], np.where(cs["keep"], 0, 3).astype(np.uint16), [3])
        want, plain = oracle(key, cs, po, k, geo)
        wants.append(want)
        border = max(7, pg.adapthalfwin)
        n_est = int(PC.estimated_pixels(cs["d"].shape, border, cs["keep"]).sum())
        offered = any(m is not None for m in cs["maps"])
        if at_work and offered:                     # conditions on the inputs: the term is at work in this item, in every branch
            differ = int(((want[0] != plain[0]) & PC.estimated_pixels(cs["d"].shape, border, cs["keep"])).sum())
            GC.conditions(want[3], n_est, differ, three_weights)
        else:
            assert want[3]["evals_geo"] == 0 and all(np.array_equal(a, b) for a, b in zip(want[:3], plain[:3]))
        td = torch.from_numpy(np.ascontiguousarray(cs["d"])).to(dev); tn = torch.from_numpy(np.ascontiguousarray(cs["n"])).to(dev)
        tc = torch.zeros_like(td)
        it = dict(ref_id=ids[0], src_ids=ids[1:], d_min=cs["dmin"], d_max=cs["dmax"], d_depth=td.data_ptr(), d_normal=tn.data_ptr(), d_conf=tc.data_ptr(),
                  seed_offset=7 * k)
        items.append((it, (td, tn, tc), ids))
    torch.cuda.synchronize()
    try:
        ctx.estimate_batch_device([it for it, _, _ in items], pg)
        ctx.synchronize()
        st = ctx.stats(); gs = ctx.get_geo_stats()
        maps = [(td.cpu().numpy(), tn.cpu().numpy(), tc.cpu().numpy()) for _, (td, tn, tc), _ in items]
    finally:
        ctx.set_geo_params(on=False)
        for i in ids_all:
            ctx.set_spread_maps_device(i, None, None, None)
        for (it, _, ids), cs in zip(items, cases):
            if cs["keep"] is not None:
                ctx.set_ignore_mask(ids[0], None, [])
    for i, want in enumerate(wants):
        _compare(maps[i], want[:3], "item %d" % i)
    assert st.evals == sum(w[3]["evals"] for w in wants)
    assert gs["evals_geo"] == sum(w[3]["evals_geo"] for w in wants)
    assert gs["pixels_geo"] == sum(w[3]["pixels_geo"] for w in wants)
    return st, gs, maps


@pytest.mark.parametrize("V", [1, 3, 8, 10])
def test_single_estimate(ctx, V):
    """the plain (8), PACK (1, 3) and TWO + PACK (10) instances, 96 x 80, two sweeps; the last source view is smaller than the reference"""
    cs = case("single%d" % V, 96, 80, V, 10 + V)
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=40 + V, **KW)
    st, gs, _ = run(ctx, "single%d" % V, [cs], pg, po)
    assert gs["evals_geo"] > 0


@pytest.mark.parametrize("a,sweeps", [(5, 1), (6, 3), (7, 2), (10, 1)])
def test_patch_sizes(ctx, a, sweeps):
    """6 x 6, 7 x 7, 8 x 8 taps and the 11 x 11 big-patch instances, 144 x 112 with 1 .. 3 sweeps; the last outer iteration ends with the
    end pass, so the stored confidence is that of the blended score"""
    cs = case("patch", 144, 112, 3, 31)
    pg, po = _params(adapthalfwin=a, n_estimation_iters=sweeps, it_external=2, n_external_iters=3, seed=a, **KW)
    run(ctx, "patch%d" % a, [cs], pg, po, base=100)


@pytest.mark.parametrize("waves", [1, 2, 3])
@pytest.mark.parametrize("mode", ["one", "per-sweep"])
def test_waves_per_row_and_launch_modes(waves, mode, monkeypatch):
    """one, two and three waves per row, all sweeps in one launch and one launch per sweep: identical maps"""
    monkeypatch.setenv("HCMVS_WAVES_PER_ROW", str(waves))
    monkeypatch.setenv("HCMVS_SWEEP_LAUNCHES", mode)
    c = binding.Context(0)
    try:
        cs = case("waves", 96, 80, 4, 44)
        pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=9, **KW)
        st, _, _ = run(c, "waves", [cs], pg, po)
        assert st.n_sweep_launches == (1 if mode == "one" else 2)
    finally:
        c.close()


def test_a_mask(ctx):
    """a keep-mask (the MASK + GEO instances): the ignored pixels are neither estimated nor counted"""
    keep = np.ones((80, 96), np.uint8)
    keep[20:50, 30:60] = 0
    keep[::7, ::5] = 0
    cs = case("mask", 96, 80, 3, 51, keep=keep)
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=5, **KW)
    run(ctx, "mask", [cs], pg, po, base=200)


def test_a_batch_of_items_with_maps_without_and_a_view_without_between_two_with(ctx):
    """one launch for an item whose source views all offer maps, an item whose middle source view offers none (that view's pairs are
    neutral), and an item whose source views offer none (the term is not active for it: a plain item inside a GEO launch)"""
    a = case("mixA", 96, 80, 3, 61)
    b = case("mixB", 96, 80, 3, 62, offers=(True, False, True))
    c = case("mixC", 96, 80, 3, 63, offers=(False, False, False))
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=21, **KW)
    tx = a["tx"]
    st, gs, _ = run(ctx, "mix", [a, b, c], pg, po, base=300, tx=tx)
    assert _WANTS[("mix", 2)][0][3]["evals_geo"] == 0 and _WANTS[("mix", 1)][0][3]["pairs"]["nomaps"] > 0


@pytest.mark.parametrize("why", ["w0", "early", "off"])
def test_the_term_without_effect_equals_the_plain_estimate(ctx, why):
    """w = 0 everywhere (both thresholds below every texture value), it_external < photo2geo, and on = 0 after having been on: each
    equals the plain estimate bit for bit and reports evals_geo == 0"""
    cs = case("single3", 96, 80, 3, 13)
    it_external = 1
    geo, tx = dict(GEO), cs["tx"]
    if why == "w0":
        tx = (-1.0, -0.5)
    if why == "early":
        geo["photo2geo"] = 2
    if why == "off":
        pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=1, n_external_iters=3, seed=43, **KW)
        run(ctx, "single3", [cs], pg, po)                    # on, at work ...
        geo = None                                          # ... and off again
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, it_external=it_external, n_external_iters=3, seed=43, **KW)
    st, gs, maps = run(ctx, "noeffect-" + why, [cs], pg, po, geo=geo, tx=tx, at_work=False)
    assert gs == dict(evals_geo=0, pixels_geo=0)
    plain = O.estimate(cs["views"], po, cs["dmin"], cs["dmax"], cs["d"], cs["n"])
    _compare(maps[0], plain[:3], "against the oracle's plain estimate")
    assert st.evals == plain[3]


def test_refusals(ctx):
    """every refusal returns HCMVS_ERR_INVALID with nothing enqueued: the options, and the term active together with view spread at
    work, the hint in effect, an active depth prior, and maps that alias the item's in/out maps"""
    import torch
    dev = torch.device("cuda:0")
    for kw in (dict(para_tapa=1.5), dict(para_tapa2=-0.1), dict(para_tapa=float("nan")), dict(txthreshold=float("inf")), dict(txthreshold2=float("nan")),
               dict(max_px=0.0), dict(max_px=float("inf")), dict(photo2geo=-1)):
        with pytest.raises(binding.HcmvsError) as e:
            ctx.set_geo_params(**kw)
        assert e.value.code == binding.ERR_INVALID
    cs = case("single3", 96, 80, 3, 13)
    ids = [400, 401, 402, 403]
    for i, v in zip(ids, cs["views"]):
        ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"])
    held = [[torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in m] for m in cs["maps"]]
    for i, t in zip(ids[1:], held):
        ctx.set_spread_maps_device(i, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
    td = torch.from_numpy(cs["d"]).to(dev); tn = torch.from_numpy(cs["n"]).to(dev); tc = torch.zeros_like(td)
    before = (td.clone(), tn.clone(), tc.clone())
    it = dict(ref_id=ids[0], src_ids=ids[1:], d_min=cs["dmin"], d_max=cs["dmax"], d_depth=td.data_ptr(), d_normal=tn.data_ptr(), d_conf=tc.data_ptr())
    pg, _ = _params(adapthalfwin=6, n_estimation_iters=1, it_external=2, n_external_iters=3, seed=1, **KW)
    ctx.set_geo_params(**dict(GEO, on=1))
    try:
        def refused(word, item=it):
            with pytest.raises(binding.HcmvsError) as e:
                ctx.estimate_batch_device([item], pg)
            assert e.value.code == binding.ERR_INVALID and word in str(e.value), str(e.value)
        ctx.set_viewspread(True)
        refused("view spread")
        ctx.set_viewspread(False)
        refused("hint", dict(it, d_hint_depth=td.data_ptr(), d_hint_normal=tn.data_ptr()))
        ctx.set_prior_params(para_prior=0.5, sigma_prior=0.2, photo2geo=1)
        ctx.set_depth_prior(ids[0], cs["views"][0]["depth"].astype(np.float32))
        refused("prior")
        ctx.set_depth_prior(ids[0], None)
        # the maps a source view offers must not be the maps the item writes (same size here: views 0 and 1)
        ctx.set_spread_maps_device(ids[1], td.data_ptr(), tn.data_ptr(), tc.data_ptr())
        refused("overlap")
        ctx.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (td, tn, tc)))        # nothing was enqueued
    finally:
        ctx.set_viewspread(False)
        ctx.set_geo_params(on=False)
        ctx.set_depth_prior(ids[0], None)
        for i in ids[1:]:
            ctx.set_spread_maps_device(i, None, None, None)

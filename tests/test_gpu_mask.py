"""--ignore-mask-label on the GPU: estimates of reference views that carry a keep-mask (hcmvs_set_ignore_mask) against the oracle's
masked estimate (oracle_lib.estimate with a keep-mask), bit for bit, with equal evaluation counts -- single estimates, batches mixing masked and
unmasked items in every launch mode, the 9..16-view and big-patch kernels, the restore hint, and the device-side resampling of a
label image of another size."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle_lib as O
import oracle_mask_lib as M

pytestmark = pytest.mark.gpu

binding = importlib.import_module("hc-mvs_amd.binding")
synth = importlib.import_module("hc-mvs_amd.synth")


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def _scene(w, h, n_src, seed, n_pts=80):
    views = synth.make_views(w, h, 90.0, n_src, seed=seed)
    return views, synth.sparse_points(views, n_pts)


def _compare(got, want, what=""):
    for g, w, n in zip(got, want, ("depth", "normal", "conf")):
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s %s differs at %d elements, first %s: gpu %r oracle %r" %
                                 (what, n, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))


def _blobs(h, w, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros((h, w), np.uint16)
    yy, xx = np.mgrid[:h, :w]
    for k in range(8):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(3, 12)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 3 + (k % 3)
    return lab


def _labels(kind, h, w, seed=1):
    lab = np.zeros((h, w), np.uint16)
    if kind == "blobs":
        return _blobs(h, w, seed)
    if kind == "line":
        lab[:, w // 2] = 3                        # one-pixel line: the median gives it a positive depth where its neighbours have one
        lab[h // 3, :] = 3
    elif kind == "border":
        lab[:] = 3; lab[9: h - 12, 11: w - 8] = 0  # covers the 7 px border and some of the inside
    elif kind == "all":
        lab[:] = 3
    return lab


def _upload(ctx, views, base):
    ids = list(range(base, base + len(views)))
    for i, v in zip(ids, views):
        ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"])
    return ids


def _want(views, po, dmin, dmax, d0, n0, keep):
    return O.estimate(views, po, dmin, dmax, d0, n0, keep=keep)


def _params(**kw):
    pg = binding.default_params(**kw)
    po = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, **kw)
    return pg, po


@pytest.mark.parametrize("kind", ["blobs", "line", "border", "all", "none"])
@pytest.mark.parametrize("last", [True, False])
def test_single_estimate(ctx, kind, last):
    views, pts = _scene(104, 84, 3, seed=11)
    ids = _upload(ctx, views, 0)
    h, w = views[0]["gray"].shape
    d0, n0, dmin, dmax = ctx.splat_init(0, pts)
    d0 = np.where(d0 > 0, d0, np.float32(0)).astype(np.float32)
    kw = dict(adapthalfwin=6, n_estimation_iters=3, it_external=0, n_external_iters=1 if last else 2)
    pg, po = _params(**kw)
    lab = _labels(kind, h, w)
    ignore = [3, 4, 5] if kind != "none" else [9]
    ctx.set_ignore_mask(0, lab, ignore)
    keep = M.keep_mask(lab, ignore, w, h)
    assert np.array_equal(ctx.ignore_mask(0), keep)
    got = ctx.estimate(0, ids[1:], pg, dmin, dmax, d0, n0)
    st = ctx.stats()
    want = _want(views, po, dmin, dmax, d0, n0, keep)
    _compare(got, want, kind)
    assert st.evals == want[3]
    if kind == "none":  # a mask that ignores nothing is no mask at all
        ctx.set_ignore_mask(0, None, [])
        assert ctx.ignore_mask(0).all()
        _compare(ctx.estimate(0, ids[1:], pg, dmin, dmax, d0, n0), want, "unmasked")
        assert ctx.stats().evals == want[3]
    ctx.set_ignore_mask(0, None, [])


def _batch(ctx, torch, scenes, masks, pg, po, base=2000, hints=None):
    """one batch call over scene i's view 0 with mask masks[i] (None = unmasked); checks every item against the masked oracle"""
    dev = torch.device("cuda:0")
    items, held, wants = [], [], []
    vid = base
    for si, (views, pts) in enumerate(scenes):
        ids = _upload(ctx, views, vid)
        vid += len(views)
        h, w = views[0]["gray"].shape
        d0, n0, dmin, dmax = ctx.splat_init(ids[0], pts)
        keep = None
        if masks[si] is not None:
            ctx.set_ignore_mask(ids[0], masks[si], [3, 4])
            keep = M.keep_mask(masks[si], [3, 4], w, h)
        po.seed = pg.seed + 5 * si
        if hints:
            po.hint_depth = hints[si][0].ctypes.data_as(C.POINTER(C.c_float)); po.hint_normal = hints[si][1].ctypes.data_as(C.POINTER(C.c_float))
        wants.append(_want(views, po, dmin, dmax, d0, n0, keep))
        td = torch.from_numpy(d0).to(dev); tn = torch.from_numpy(n0).to(dev); tc = torch.zeros_like(td)
        it = dict(ref_id=ids[0], src_ids=ids[1:], d_min=dmin, d_max=dmax, d_depth=td.data_ptr(), d_normal=tn.data_ptr(),
                  d_conf=tc.data_ptr(), seed_offset=5 * si)
        if hints:
            hd = torch.from_numpy(hints[si][0]).to(dev); hn = torch.from_numpy(hints[si][1]).to(dev)
            it.update(d_hint_depth=hd.data_ptr(), d_hint_normal=hn.data_ptr()); held.append((hd, hn))
        held.append((td, tn, tc)); items.append(it)
    torch.cuda.synchronize()
    ctx.estimate_batch_device(items, pg)
    ctx.synchronize()
    st = ctx.stats()
    maps = [h for h in held if len(h) == 3]
    for i, ((td, tn, tc), want) in enumerate(zip(maps, wants)):
        _compare((td.cpu().numpy(), tn.cpu().numpy(), tc.cpu().numpy()), want[:3], "item %d" % i)
    assert st.evals == sum(w[3] for w in wants)
    return st


@pytest.mark.parametrize("mode", [None, "per-sweep", "one", "segment"])
def test_batch_mixing_masked_and_unmasked(mode, monkeypatch):
    torch = pytest.importorskip("torch")
    if mode == "segment":
        monkeypatch.setenv("HCMVS_SWEEP_SEGMENT", "40")
    elif mode:
        monkeypatch.setenv("HCMVS_SWEEP_LAUNCHES", mode)
    c = binding.Context(0)
    try:
        scenes = [_scene(96, 80, 3, seed=21 + k) for k in range(4)]
        masks = [_blobs(80, 96, 1), None, _labels("line", 80, 96), _blobs(40, 48, 2)]
        pg, po = _params(adapthalfwin=6, n_estimation_iters=3, seed=700)
        st = _batch(c, torch, scenes, masks, pg, po)
        if mode == "one":
            assert st.n_sweep_launches == 1
        if mode == "per-sweep":
            assert st.n_sweep_launches == 3
    finally:
        c.close()


def test_batch_big_patch(ctx):
    torch = pytest.importorskip("torch")
    scenes = [_scene(88, 80, 3, seed=51), _scene(88, 80, 3, seed=52)]
    pg, po = _params(adapthalfwin=10, n_estimation_iters=2, seed=900)  # 11 x 11 taps: the big-patch kernels
    _batch(ctx, torch, scenes, [_blobs(80, 88, 5), None], pg, po, base=3000)


def test_batch_more_than_eight_views(ctx):
    torch = pytest.importorskip("torch")
    scenes = [_scene(80, 72, 10, seed=61), _scene(80, 72, 10, seed=62)]
    pg, po = _params(adapthalfwin=5, n_estimation_iters=2, seed=300, it_external=1, n_external_iters=2)  # + the cross pattern
    _batch(ctx, torch, scenes, [None, _blobs(72, 80, 6)], pg, po, base=4000)


def test_restore_hint(ctx):
    torch = pytest.importorskip("torch")
    scenes = [_scene(96, 80, 3, seed=71)]
    rng = np.random.default_rng(4)
    hd = (scenes[0][0][0]["depth"] * (1 + 0.004 * rng.normal(size=(80, 96)))).astype(np.float32)
    hn = np.ascontiguousarray(scenes[0][0][0]["normal"], np.float32)
    pg, po = _params(adapthalfwin=6, n_estimation_iters=2, seed=400)
    _batch(ctx, torch, scenes, [_blobs(80, 96, 7)], pg, po, base=5000, hints=[(hd, hn)])


@pytest.mark.parametrize("lw,lh", [(48, 40), (200, 150), (37, 91), (96, 80)])
def test_label_image_of_another_size(ctx, lw, lh):
    views, _ = _scene(96, 80, 1, seed=81)
    _upload(ctx, views, 6000)
    lab = np.random.default_rng(lw).integers(0, 6, (lh, lw)).astype(np.uint16)
    lab[-1, :] = 7; lab[:, -1] = 7                 # the last row and column of the label image
    for ignore in ([3], [7, 0, -1, 70000], []):
        ctx.set_ignore_mask(6000, lab, ignore)
        assert np.array_equal(ctx.ignore_mask(6000), M.keep_mask(lab, ignore, 96, 80))
    torch = pytest.importorskip("torch")
    dl = torch.from_numpy(lab.astype(np.int16)).to("cuda:0")  # (the same bits as u16)
    torch.cuda.synchronize()
    ctx.set_ignore_mask_device(6000, dl.data_ptr(), lw, lh, [5, 7])
    assert np.array_equal(ctx.ignore_mask(6000), M.keep_mask(lab, [5, 7], 96, 80))
    ctx.release_view(6000)

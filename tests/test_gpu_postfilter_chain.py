"""hcmvs_postfilter_sequence's incremental fusions (pf_kernels.hip) against the oracle run image after image, bit for bit, after EVERY
prefix of a chain: the device exposes no owner map, but the image a fusion masks shows it -- seq[:k] ends with the gap interpolation of image
seq[k-1] under the owner map of fusion k, so a wrong owner map that a later fusion would repair is seen.  k = 1 runs the fusion from scratch,
every k >= 2 the incremental path.  The scenes (chain_scenes.py) are the ones test_postfilter_chain_scenarios.py shows, on the oracle alone,
to release, steal, hand on and re-link estimates between their fusions: nMinViewsFuse 2 and 3, neighbours of other sizes, pixel counts that
are no multiple of 64, an image that is a target but no seed, thinned lists, an id that is no view, 17 neighbours, and a change that walks a
whole row inside an incremental fusion.  No tolerance anywhere: ARITH_DEVICE is the mode in which the oracle's transcendentals are the
device's."""
import importlib

import numpy as np
import pytest

import chain_scenes as S
import oracle_lib as O

pytestmark = pytest.mark.gpu
binding = importlib.import_module("hc-mvs_amd.binding")


@pytest.fixture(scope="module")
def ctx():
    c = binding.Context(0)
    yield c
    c.close()


def upload(ctx, maps, keep_stale=False):
    """register the scene as views 0 .. n-1; views a scene before it left under other ids go (unless keep_stale: they stay, with their maps)"""
    if not keep_stale:
        for vid in [v for v in ctx.shapes if v >= len(maps)]:
            ctx.release_view(vid)
    for i, m in enumerate(maps):
        ctx.upload_view(i, m["gray"], m["K"], m["R"], m["C"], bgr=m["bgr"])
        ctx.set_depthmap(i, m["depth"], m["normal"], m["conf"], m["d_min"], m["d_max"])
        ctx.set_neighbors(i, m["neighbors"])


def check_maps(ctx, state, what):
    """depth, normal and confidence of every image against one entry of chain_scenes.run_chain"""
    for i in range(len(state["depth"])):
        d, n, c = ctx.get_depthmap(i, with_normal=True)
        assert np.array_equal(d, state["depth"][i]), (what, i, "depth", int((d != state["depth"][i]).sum()))
        assert np.array_equal(n, state["normal"][i]), (what, i, "normal")
        assert np.array_equal(c, state["conf"][i]), (what, i, "conf")


def check_prefixes(ctx, maps, order, seq, chain, capfd, monkeypatch, **kw):
    for k in range(1, len(seq) + 1):
        upload(ctx, maps)
        debug = k == len(seq) and k >= 2
        if debug:   # a silent fall-back to fusions from scratch must not pass for the incremental path
            monkeypatch.setenv("HCMVS_FUSE_DEBUG", "1")
            capfd.readouterr()
        filled = ctx.postfilter_sequence(seq[:k], order, **kw)
        if debug:
            err = capfd.readouterr().err
            monkeypatch.delenv("HCMVS_FUSE_DEBUG")
            assert "fusions computed incrementally" in err
        assert filled == chain[k - 1]["filled"], (k, filled, chain[k - 1]["filled"])
        check_maps(ctx, chain[k - 1], "prefix %d" % k)


def check_fuse(ctx, maps, order, **kw):
    """ctx.fuse against the oracle: cloud, point order, invalidated depths"""
    want = O.fuse_depthmaps(maps, order, 100000, **kw)
    got = ctx.fuse(order, 100000, **kw)
    assert got["n_points"] == want["n_points"] > 100 and got["n_depths"] == want["n_depths"]
    assert np.array_equal(got["xyz"], want["xyz"]) and np.array_equal(got["n_views"], want["n_views"])
    assert np.array_equal(got["normal"], want["normal"]) and np.array_equal(got["bgr"], want["bgr"])
    for i, d in enumerate(want["depths"]):
        assert np.array_equal(ctx.get_depthmap(i)[0], d), i


@pytest.mark.parametrize("name", list(S.SCENES))
def test_device_gradient_map_is_the_oracles(ctx, name):
    """the oracle chains read the gradient map the device derives from the uploaded image: GapInterpolation's long-gap rule sees the same"""
    maps, _, seq = S.scene(name)
    upload(ctx, maps)
    for v in seq:
        assert np.array_equal(ctx.gradient_map(v), S.gradient_of(maps[v])), v


@pytest.mark.parametrize("name,nmin", S.CASES)
def test_every_prefix_of_the_chain(ctx, capfd, monkeypatch, name, nmin):
    """(a) seq[:k] for k = 1 .. len(seq), maps uploaded afresh each time: maps of every image and the fill count equal the oracle chain after
    k images; the longest prefix is shown to have run incrementally"""
    maps, order, seq = S.scene(name)
    check_prefixes(ctx, maps, order, seq, S.chain_of(name, nmin), capfd, monkeypatch, n_min_views_fuse=nmin)


@pytest.mark.parametrize("name,nmin", S.CASES)
def test_chain_with_every_fusion_from_scratch(ctx, monkeypatch, name, nmin):
    """(b) HCMVS_PF_FULL=1: the same chains without the incremental state -- the oracle's result, hence that of (a)"""
    maps, order, seq = S.scene(name)
    chain = S.chain_of(name, nmin)
    upload(ctx, maps)
    monkeypatch.setenv("HCMVS_PF_FULL", "1")
    filled = ctx.postfilter_sequence(seq, order, n_min_views_fuse=nmin)
    monkeypatch.delenv("HCMVS_PF_FULL")
    assert filled == chain[-1]["filled"]
    check_maps(ctx, chain[-1], "from scratch")


@pytest.mark.parametrize("gap", [3, 0])
def test_other_thresholds(ctx, capfd, monkeypatch, gap):
    """(c) R1 with a wider depth threshold, a narrower normal cone and short / no short gaps"""
    maps, order, seq = S.scene("R1")
    chain = S.run_chain(maps, order, seq, 2, thr=0.02, normal_deg=15.0, gap=gap)
    assert chain[-1]["filled"] > 100 and chain[-1]["filled"] != S.chain_of("R1", 2)[-1]["filled"]
    check_prefixes(ctx, maps, order, seq, chain, capfd, monkeypatch, n_min_views_fuse=2, depth_diff_threshold=0.02, normal_diff_deg=15.0, gap_size=gap)


def test_state_reuse_on_one_context(ctx):
    """(d) R5's chain, then R2's on the same context (smaller tables inside the grown state buffer, ids 0 .. 3 are other images now, view
    4 of R5 is still registered with its maps but nobody names it), then a cloud fusion of R2's maps, then R5 again: nothing of the chain
    state, the per-pass scratch or the claim marks leaks from one call into the next"""
    for name, nmin, stale in (("R5", 3, False), ("R2", 3, True), (None, 0, True), ("R5", 3, False), ("R2", 2, True)):
        if name is None:
            maps, order, _ = S.scene("R2")
            upload(ctx, maps, keep_stale=True)
            check_fuse(ctx, maps, order)
            continue
        maps, order, seq = S.scene(name)
        chain = S.chain_of(name, nmin)
        upload(ctx, maps, keep_stale=stale)
        assert ctx.postfilter_sequence(seq, order, n_min_views_fuse=nmin) == chain[-1]["filled"], name
        check_maps(ctx, chain[-1], name)


@pytest.mark.parametrize("registered", [False, True])
def test_neighbour_id_that_is_no_view_with_maps(ctx, registered):
    """(e) R4b: view 3's list starts with id 7, which is no view (registered = False) or a view without maps (True).  The entry is passed
    over, as the oracle does (hcmvs_fuse.c: `B >= n_maps || !maps[B].depth`): chain, single post-filter calls and the cloud fusion equal
    the oracle's, which equal those of the list without the entry (test_postfilter_chain_scenarios.py)"""
    maps, order, seq = S.scene("R4b")
    chain = S.chain_of("R4b", 2)
    def put():
        upload(ctx, maps)
        if registered:
            m = maps[0]
            ctx.upload_view(7, m["gray"], m["K"], m["R"], m["C"], bgr=m["bgr"])     # a view, but it has no maps
    assert max(max(m["neighbors"], default=0) for m in maps) == 7 and len(maps) == 5
    put()
    assert ctx.postfilter_sequence(seq, order) == chain[-1]["filled"]
    check_maps(ctx, chain[-1], "sequence")
    put()
    for k, v in enumerate(seq):
        assert ctx.postfilter(v, order) == chain[k]["filled_image"]
        check_maps(ctx, chain[k], "single call %d" % k)
    put()
    check_fuse(ctx, maps, order)
    put()
    check_fuse(ctx, maps, order, n_min_views_fuse=3)


def test_neighbour_id_beyond_the_bound_is_refused(ctx):
    """(e) ids of views lie below 65536 (hcmvs_upload_view); hcmvs_set_neighbors refuses a list that names a larger one with ERR_INVALID,
    leaves the view's list as it was, and the context goes on working"""
    maps, order, seq = S.scene("R4b")
    chain = S.chain_of("R4b", 2)
    upload(ctx, maps)
    for bad in ([65536], [1, 0xFFFFFFFF, 2], [0x7FFFFFFF]):
        with pytest.raises(binding.HcmvsError) as e:
            ctx.set_neighbors(3, bad)
        assert e.value.code == binding.ERR_INVALID
    ctx.set_neighbors(1, maps[1]["neighbors"] + [65535])     # the largest id a view can have: accepted, no such view, passed over
    assert ctx.postfilter_sequence(seq, order) == chain[-1]["filled"]
    check_maps(ctx, chain[-1], "after the refusals")


@pytest.mark.parametrize("name", ["F512", "F130"])
def test_phase_flip_through_single_calls(ctx, name):
    """(f) scene F image by image (every fusion from scratch; the chain itself is in test_every_prefix_of_the_chain, where the second
    fusion walks every row, one pixel per step, through the single-workgroup settle loop of an INCREMENTAL pass): maps and fill counts
    equal the oracle's, and no call gives up (ERR_TIMEOUT would raise)"""
    maps, order, seq = S.scene(name)
    chain = S.chain_of(name, 3)
    upload(ctx, maps)
    for k, v in enumerate(seq):
        assert ctx.postfilter(v, order, n_min_views_fuse=3) == chain[k]["filled_image"]
        check_maps(ctx, chain[k], "single call %d" % k)

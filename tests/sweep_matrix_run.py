"""helper: one estimate_batch_device of a batch of scenes in a fresh Context created under the sweep knobs, against the CPU oracle bit for
bit.  Shared by test_gpu_sweep_matrix.py (plain items) and test_gpu_sweep_matrix_flavours.py (items with a keep-mask, with source views
that offer maps, or both).

A scene is a dict as sweep_matrix.render makes it (views, d0, n0, dmin, dmax, hint) with, optionally,
  labels, ignore, keep   a label image (u16, any size), the ignored labels, and the keep-mask they must give (what the oracle gets);
  maps                   per source view None or (depth, normal, conf): what the view offers;
  spread                 view spread is switched on for the estimate (an item without maps then runs the SPREAD instance all the same).
The oracle runs once per item and process (`want`); nobody writes to what it returns."""
import importlib

import numpy as np

import oracle_lib as O

KNOBS = ("HCMVS_WAVES_PER_ROW", "HCMVS_SWEEP_LAUNCHES", "HCMVS_SWEEP_SEGMENT", "HCMVS_XCD_AFFINITY", "HCMVS_SWEEP_LAG")

_ORACLE = {}


def want(key, item, kw, seed_offset):
    """the oracle's (depth, normal, conf, evals, spread counters) of one item, computed once (device association, row order, 8 threads);
    the spread counters are O.stats(): (slots scored, accepted, dropped, candidates outside), all 0 without view spread"""
    key = (key, tuple(sorted(kw.items())), seed_offset)
    if key not in _ORACLE:
        po = O.default_params(arith_mode=O.ARITH_DEVICE, order=O.ORDER_ROWS, n_threads=8, **kw)
        po.seed = kw["seed"] + seed_offset
        if item["hint"] is not None:
            po.hint_depth = O.fptr(item["hint"][0]); po.hint_normal = O.fptr(item["hint"][1])
        O.stats(reset=True)
        res = O.estimate(item["views"], po, item["dmin"], item["dmax"], item["d0"], item["n0"], keep=item.get("keep"), maps=item.get("maps"),
                         on=bool(item.get("spread")))
        _ORACLE[key] = res + (O.stats(),)
    return _ORACLE[key]


def compare(got, want, what):
    for g, w, n in zip(got, want, ("depth", "normal", "conf")):
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d elements, first %s: gpu %r oracle %r" %
                                 (what, n, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))


def run(monkeypatch, scenes, wants, offsets, kw, knobs, n_launches, tag=""):
    """one estimate_batch_device over the scenes' reference views in a fresh context created under `knobs`: maps, evaluation count, the
    number of sweep launches and, with view spread, its four counters"""
    import torch
    binding = importlib.import_module("hc-mvs_amd.binding")
    dev = torch.device("cuda:0")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        assert k in KNOBS
        monkeypatch.setenv(k, str(v))
    what = tag + " ".join("%s=%s" % (k[6:], v) for k, v in knobs.items())
    spread = any(sc.get("spread") for sc in scenes)
    c = binding.Context(0)
    try:
        items, held, outs, masked, offering = [], [], [], [], []
        vid = 0
        for sc, off in zip(scenes, offsets):
            ids = list(range(vid, vid + len(sc["views"])))
            vid += len(ids)
            for i, v in zip(ids, sc["views"]):
                c.upload_view(i, v["gray"], v["K"], v["R"], v["C"])
            if sc.get("labels") is not None:
                c.set_ignore_mask(ids[0], sc["labels"], sc["ignore"])
                assert np.array_equal(c.ignore_mask(ids[0]), sc["keep"]), "%s: the keep-mask of view %d" % (what, ids[0])
                masked.append(ids[0])
            for i, m in zip(ids[1:], sc.get("maps") or ()):
                if m is not None:
                    t = [torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in m]
                    c.set_spread_maps_device(i, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr())
                    held.append(t); offering.append(i)
            td = torch.from_numpy(sc["d0"]).to(dev); tn = torch.from_numpy(sc["n0"]).to(dev); tc = torch.zeros_like(td)
            it = dict(ref_id=ids[0], src_ids=ids[1:], d_min=sc["dmin"], d_max=sc["dmax"], d_depth=td.data_ptr(), d_normal=tn.data_ptr(),
                      d_conf=tc.data_ptr(), seed_offset=off)
            if sc["hint"] is not None:
                hd = torch.from_numpy(sc["hint"][0]).to(dev); hn = torch.from_numpy(sc["hint"][1]).to(dev)
                it.update(d_hint_depth=hd.data_ptr(), d_hint_normal=hn.data_ptr()); held.append((hd, hn))
            outs.append((td, tn, tc)); items.append(it)
        if spread:
            c.set_viewspread(True)
        torch.cuda.synchronize()
        c.estimate_batch_device(items, binding.default_params(**kw))
        c.synchronize()
        st = c.stats()      # (a sweep worker that gave up waiting raises here)
        for i, (h, wt) in enumerate(zip(outs, wants)):
            compare([t.cpu().numpy() for t in h], wt[:3], "%s, item %d" % (what, i))
        assert st.evals == sum(w[3] for w in wants), what
        assert st.n_sweep_launches == n_launches, what
        if spread:
            sp = c.spread_stats()
            got = (sp["slots_scored"], sp["slots_accepted"], sp["slots_dropped"], sp["candidates_outside"])
            tot = tuple(int(x) for x in np.sum([w[4] for w in wants], axis=0))
            assert got == tot, "%s: spread counters %s, the oracle's %s" % (what, got, tot)
            assert tot[0] > 0 and tot[2] == 0, "%s: the oracle scored %d slots and dropped %d" % (what, tot[0], tot[2])
        for i in masked:
            c.set_ignore_mask(i, None, [])
            assert c.ignore_mask(i).all()
        for i in offering:
            c.set_spread_maps_device(i, None, None, None)
        if spread:
            c.set_viewspread(False)
    finally:
        c.close()

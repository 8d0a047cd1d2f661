"""Time the sweeps of outer iteration 2 with the geometric-consistency term (--geo-consistency) on a batch of
1920x1080 images with 8 source views: the term off (the plain instances), on with w = 0 everywhere (the GEO instances run and blend
nothing: both texture thresholds below every texture value), and on at every pixel (both thresholds above every texture value).

    python tools/geo_bench.py [--batch 32] [--steps 3] [--sweeps 3]

The maps a source view offers are its analytic depth times 1 + u, u uniform in +-2 %, and its analytic normal.  The maps outer iteration 2
starts from are those of an outer iteration 0 (one sweep) run first.  Prints one JSON line per case: estimate ms (best of the steps), ms
per sweep, ScorePixel evaluations per pixel-sweep (of the sequential algorithm, and issued: with the discarded speculative ones), the
share of evaluations that blended the term, the share of pixels with a weight."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("hc-mvs_amd.binding")
    W, H, B = bench.W, bench.H, args.batch
    HW = W * H
    dev = torch.device("cuda", 0)
    ctx = binding.Context(0)
    kw = dict(adapthalfwin=bench.AHW, propagate_halfwin=5, propagate_step=4, seed=1234)
    scenes = dict(enumerate(bench.make_scenes([(2 + k, 5 + k) for k in range(min(B, 4))])))
    rng = np.random.default_rng(7)
    synth = importlib.import_module("hc-mvs_amd.synth")
    px = 10.0 / bench.FOCAL
    offered = {}
    for k, (views, _) in scenes.items():    # the maps scene k's source views offer (shared by the images that use the scene)
        sc = synth.Scene(2 + k, min_wavelength=3.5 * px, max_wavelength=150 * px)     # (bench.make_scenes keeps the reference view's depth only)
        offered[k] = []
        for v in views[1:]:
            _, depth, normal = sc.render(v["K"], v["R"], v["C"], W, H)
            d = (depth * (1.0 + rng.uniform(-0.02, 0.02, (H, W)))).astype(np.float32)
            offered[k].append((torch.from_numpy(d).to(dev), torch.from_numpy(np.ascontiguousarray(normal, np.float32)).to(dev),
                               torch.zeros(H, W, device=dev)))
    items, slabs = [], []
    work = torch.empty(B, 5 * HW, dtype=torch.float32, device=dev)
    start = torch.empty(B, 5 * HW, dtype=torch.float32, device=dev)
    for b in range(B):
        views, pts = scenes[b % 4]
        slab = torch.from_numpy(np.stack([v["gray"] for v in views])).to(dev)
        slabs.append(slab)
        for i, v in enumerate(views):
            ctx.set_view_device(100 * b + i, W, H, slab[i].data_ptr(), v["K"], v["R"], v["C"])
        ctx.shapes[100 * b] = (H, W)
        d0, n0, dmin, dmax = ctx.splat_init(100 * b, pts)
        work[b].copy_(torch.cat([torch.from_numpy(d0).reshape(-1), torch.from_numpy(n0).reshape(-1), torch.zeros(HW)]).to(dev))
        base = work[b].data_ptr()
        items.append(dict(ref_id=100 * b, src_ids=[100 * b + i for i in range(1, bench.N_SRC + 1)], d_min=dmin, d_max=dmax,
                          d_depth=base, d_normal=base + 4 * HW, d_conf=base + 16 * HW, seed_offset=b))
    torch.cuda.synchronize()
    ctx.estimate_batch_device(items, binding.default_params(n_estimation_iters=1, it_external=0, n_external_iters=4, **kw))
    ctx.synchronize()
    start.copy_(work)
    params = binding.default_params(n_estimation_iters=args.sweeps, it_external=2, n_external_iters=4, **kw)   # (not the last: conf stays the score)
    for b in range(B):
        for i, m in enumerate(offered[b % 4]):
            ctx.set_spread_maps_device(100 * b + 1 + i, m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr())
    ctx.set_viewspread(False)
    inner = (W - 14) * (H - 14)

    def run():
        best = None
        for _ in range(args.steps + 1):  # (the first is a warm-up)
            work.copy_(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.estimate_batch_device(items, params)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            st = ctx.stats(); gs = ctx.get_geo_stats()
            if best is None or dt < best[0]:
                best = (dt, st, gs)
        return best

    cases = (("term off", dict(on=False)), ("on, w = 0 everywhere", dict(on=True, txthreshold=-2.0, txthreshold2=-1.0)),
             ("on at every pixel", dict(on=True, txthreshold=300.0, txthreshold2=301.0)), ("term off again", dict(on=False)))
    for name, geo in cases:
        ctx.set_geo_params(**geo)
        dt, st, gs = run()
        pxs = float(B) * inner * args.sweeps
        scored = B * inner      # the init-score pass: one evaluation per pixel
        print(json.dumps({"case": name, "batch": B, "sweeps": args.sweeps, "estimate_ms": round(dt * 1e3, 1), "ms_sweep_avg": round(st.ms_sweep_avg, 2),
                          "ms_score": round(st.ms_score, 2), "evals_per_pixel_sweep": round((st.evals - scored) / pxs, 3),
                          "evals_issued_per_pixel_sweep": round((st.evals_issued - scored) / pxs, 3),
                          "evals_geo_share": round(gs["evals_geo"] / max(st.evals, 1), 3),
                          "pixels_geo_share": round(gs["pixels_geo"] / (float(B) * inner), 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

"""Time the sweeps of outer iteration 1 with view spread (--n-viewspread) on a batch of 1920x1080 images with 8 source views: spread
off, on with the source views' analytic maps (converged source views: the case the feature is for), and on with maps that hold nothing
(every candidate is looked up, none becomes a slot).

    python tools/spread_bench.py [--batch 32] [--steps 3] [--sweeps 3]

The maps outer iteration 1 starts from are those of an outer iteration 0 (one sweep) run first.  Prints one JSON line per case: estimate
ms (best of the steps), ms per sweep, ScorePixel evaluations per pixel-sweep, spread slots scored / accepted per sweep."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def render_maps(scene, K, R, C, w, h):
    _, depth, normal = scene.render(K, R, C, w, h)
    return depth, normal


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
    items, slabs, offered, empty = [], [], {}, {}
    work = torch.empty(B, 5 * HW, dtype=torch.float32, device=dev)
    start = torch.empty(B, 5 * HW, dtype=torch.float32, device=dev)
    # what the source views of scene k offer (shared by the images that use the scene): their analytic depth and normal maps
    import multiprocessing
    from concurrent.futures import ProcessPoolExecutor
    synth = importlib.import_module("hc-mvs_amd.synth")
    px = 10.0 / bench.FOCAL
    with ProcessPoolExecutor(int(os.environ.get("OMP_NUM_THREADS") or 16), mp_context=multiprocessing.get_context("spawn")) as ex:
        futs = {k: [ex.submit(render_maps, synth.Scene(2 + k, min_wavelength=3.5 * px, max_wavelength=150 * px), v["K"], v["R"], v["C"], W, H) for v in views[1:]]
                for k, (views, _) in scenes.items()}
        for k, fs in futs.items():
            offered[k] = []
            for f in fs:
                d, n = f.result()
                offered[k].append((torch.from_numpy(d).to(dev), torch.from_numpy(np.ascontiguousarray(n, np.float32)).to(dev), torch.full((H, W), 0.1, device=dev)))
            empty[k] = [(torch.zeros(H, W, device=dev), o[1], o[2]) for o in offered[k]]
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
    ctx.estimate_batch_device(items, binding.default_params(n_estimation_iters=1, it_external=0, n_external_iters=3, **kw))
    ctx.synchronize()
    start.copy_(work)
    params = binding.default_params(n_estimation_iters=args.sweeps, it_external=1, n_external_iters=3, **kw)
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
            st = ctx.stats(); sp = ctx.spread_stats()
            if best is None or dt < best[0]:
                best = (dt, st, sp)
        return best

    for name, on, maps in (("off", False, None), ("on, converged source maps", True, offered), ("on, empty source maps", True, empty), ("off again", False, None)):
        ctx.set_viewspread(on)
        for b in range(B):
            for i in range(1, bench.N_SRC + 1):
                m = maps[b % 4][i - 1] if maps else None
                ctx.set_spread_maps_device(100 * b + i, *(t.data_ptr() for t in m)) if m else ctx.set_spread_maps_device(100 * b + i, None, None, None)
        dt, st, sp = run()
        ps = float(B) * inner * args.sweeps
        print(json.dumps({"viewspread": name, "batch": B, "sweeps": args.sweeps, "estimate_ms": round(dt * 1e3, 1), "ms_sweep_avg": round(st.ms_sweep_avg, 2),
                          "ms_score": round(st.ms_score, 2), "evals_per_pixel_sweep": round((st.evals - B * inner) / ps, 3),
                          "evals_issued_per_pixel_sweep": round((st.evals_issued - B * inner) / ps, 3),
                          "slots_scored_per_sweep": sp["slots_scored"] // args.sweeps, "slots_accepted_per_sweep": sp["slots_accepted"] // args.sweeps,
                          "slots_per_pixel_sweep": round(sp["slots_scored"] / ps, 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

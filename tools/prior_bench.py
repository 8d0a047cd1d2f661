"""Time the sweeps of outer iteration 2 with a depth prior (--depth-priors; DepthMap.cpp:941-954) on a batch of 1920x1080 images with 8
source views: no prior registered (the plain instances), a prior on every pixel, on about 70 % of the pixels, and registered but with every
value 0 (the PRIOR instances run and blend nothing); then the reference's two extra sweeps (hcmvs_estimate_sweeps_batch_device).

    python tools/prior_bench.py [--batch 32] [--steps 3] [--sweeps 3]

The prior of an image is the analytic depth of its reference view times 1 + u, u uniform in +-3 %.  The maps outer iteration 2 starts from
are those of an outer iteration 0 (one sweep) run first.  Prints one JSON line per case: estimate ms (best of the steps), ms per sweep,
ScorePixel evaluations per pixel-sweep (of the sequential algorithm, and issued: with the discarded speculative ones), the share of
evaluations that blended the term, the share of pixels with a usable prior."""
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
    full, part, none = {}, {}, {}
    for k, (views, _) in scenes.items():    # the priors of scene k's reference view (shared by the images that use the scene)
        p = (views[0]["depth"] * (1.0 + rng.uniform(-0.03, 0.03, (H, W)))).astype(np.float32)
        full[k] = torch.from_numpy(p).to(dev)
        q = p.copy(); q[rng.uniform(size=(H, W)) < 0.3] = 0
        part[k] = torch.from_numpy(q).to(dev)
        none[k] = torch.zeros(H, W, device=dev)
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
    ctx.set_prior_params()      # the reference's defaults 0.5, 0.2, 2
    inner = (W - 14) * (H - 14)

    def run(extra):
        best = None
        for _ in range(args.steps + 1):  # (the first is a warm-up)
            work.copy_(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if extra:
                ctx.estimate_sweeps_batch_device(items, params, args.sweeps, 2)
            else:
                ctx.estimate_batch_device(items, params)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            st = ctx.stats(); ps = ctx.prior_stats()
            if best is None or dt < best[0]:
                best = (dt, st, ps)
        return best

    cases = (("no prior", None, False), ("prior on every pixel", full, False), ("prior on 70 % of the pixels", part, False),
             ("prior registered, all zero", none, False), ("no prior again", None, False),
             ("two extra sweeps, no prior", None, True), ("two extra sweeps, prior on 70 % of the pixels", part, True))
    for name, maps, extra in cases:
        for b in range(B):
            ctx.set_depth_prior_device(100 * b, maps[b % 4].data_ptr() if maps else None)
        dt, st, ps = run(extra)
        n_sweeps = 2 if extra else args.sweeps
        pxs = float(B) * inner * n_sweeps
        scored = 0 if extra else B * inner      # the init-score pass: one evaluation per pixel
        print(json.dumps({"case": name, "batch": B, "sweeps": n_sweeps, "estimate_ms": round(dt * 1e3, 1), "ms_sweep_avg": round(st.ms_sweep_avg, 2),
                          "ms_score": round(st.ms_score, 2), "evals_per_pixel_sweep": round((st.evals - scored) / pxs, 3),
                          "evals_issued_per_pixel_sweep": round((st.evals_issued - scored) / pxs, 3),
                          "evals_prior_share": round(ps["evals_prior"] / max(st.evals, 1), 3),
                          "pixels_prior_share": round(ps["pixels_prior"] / (float(B) * inner), 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

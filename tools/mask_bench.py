"""Time the batch estimate of bench.py's headline workload (32 x 1920x1080, 8 source views, 8 sweeps) with --ignore-mask-label masks
that ignore 0, 1/3 and 2/3 of the rows of every reference image (the top rows: sky), plus the unmasked context as the baseline.

    python tools/mask_bench.py [--batch 32] [--steps 3]

Prints one JSON line per mask share: estimate ms (best of the steps), ms per sweep, ScorePixel evaluations."""
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
    args = ap.parse_args()
    import numpy as np
    import torch
    bench = importlib.import_module("bench")
    binding = importlib.import_module("hc-mvs_amd.binding")
    W, H, B = bench.W, bench.H, args.batch
    HW = W * H
    dev = torch.device("cuda", 0)
    ctx = binding.Context(0)
    params = binding.default_params(adapthalfwin=bench.AHW, n_estimation_iters=bench.SWEEPS, it_external=0, n_external_iters=1, seed=1234)
    scenes = dict(enumerate(bench.make_scenes([(2 + k, 5 + k) for k in range(min(B, 4))])))
    items, inits, slabs = [], [], []
    work = torch.empty(B, 5 * HW, dtype=torch.float32, device=dev)
    for b in range(B):
        views, pts = scenes[b % 4]
        slab = torch.from_numpy(np.stack([v["gray"] for v in views])).to(dev)
        slabs.append(slab)
        for i, v in enumerate(views):
            ctx.set_view_device(100 * b + i, W, H, slab[i].data_ptr(), v["K"], v["R"], v["C"])
        ctx.shapes[100 * b] = (H, W)
        d0, n0, dmin, dmax = ctx.splat_init(100 * b, pts)
        inits.append(torch.cat([torch.from_numpy(d0).reshape(-1), torch.from_numpy(n0).reshape(-1), torch.zeros(HW)]).to(dev))
        base = work[b].data_ptr()
        items.append(dict(ref_id=100 * b, src_ids=[100 * b + i for i in range(1, bench.N_SRC + 1)], d_min=dmin, d_max=dmax,
                          d_depth=base, d_normal=base + 4 * HW, d_conf=base + 16 * HW, seed_offset=b))

    def run():
        best = None
        for _ in range(args.steps + 1):  # (the first is a warm-up)
            for b in range(B):
                work[b].copy_(inits[b])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.estimate_batch_device(items, params)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            st = ctx.stats()
            if best is None or dt < best[0]:
                best = (dt, st)
        return best

    for share in (None, 0.0, 1.0 / 3.0, 2.0 / 3.0):
        for b in range(B):
            if share is None:
                ctx.set_ignore_mask(100 * b, None, [])
            else:
                lab = np.zeros((H, W), np.uint16)
                lab[: int(round(share * H)), :] = 1
                ctx.set_ignore_mask(100 * b, lab, [1])
        dt, st = run()
        print(json.dumps({"masked_rows": "none (no mask)" if share is None else "%.3f" % share, "batch": B, "estimate_ms": round(dt * 1e3, 1),
                          "ms_sweep_avg": round(st.ms_sweep_avg, 2), "ms_score": round(st.ms_score, 2), "evals": int(st.evals)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

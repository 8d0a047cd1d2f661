"""Time the depth-map filter stage (hcmvs_filter_sequence) on a ring of N images with 8 neighbours each, maps in device memory, against
the per-image route (N calls of hcmvs_filter, each with its two device-to-host copies and its synchronisation) on the same maps.

    python tools/filter_stage_bench.py [--images 64] [--width 1920] [--height 1080] [--neighbors 8] [--steps 3] [--route stage|per-image|both]
                                       [--tree path/to/another/checkout]

--tree takes the package (binding + built library) of another checkout of this repository, for instance the parent commit's: the per-image
route exists in every one, the stage only where it has been added.
Prints one JSON line per route and variant: the stage's device time (HIP events on the context's stream, hcmvs_filter_stats::ms_device)
and wall time, best and all of the steps after one warm-up; for the per-image route the wall time of the N calls.  `atomic_bytes` is what
the splat issues at most: 4 footprint corners x 8 B per valid pixel of every (image, neighbour) pair (corners outside the image issue
nothing)."""
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
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--neighbors", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--route", default="both", choices=["stage", "per-image", "both"])
    ap.add_argument("--tree", default=None)
    args = ap.parse_args()
    import torch
    if args.tree:      # another checkout's package: its binding and its build of the library
        sys.path.insert(0, os.path.abspath(args.tree))
    binding = importlib.import_module("hc-mvs_amd.binding")
    if args.route != "per-image" and not hasattr(binding.Context, "filter_sequence"):
        sys.exit("that checkout has no filter stage (use --route per-image)")
    import filter_stage as FS
    dev = torch.device("cuda", 0)
    n, w, h = args.images, args.width, args.height
    cams, depth, normal, conf, rng, nbrs = FS.device_ring(n, w, h, args.neighbors, dev)
    gray = torch.zeros(h, w, dtype=torch.float32, device=dev)
    d0, c0 = depth.clone(), conf.clone()
    valid = (d0 > 0).sum((1, 2)).tolist()
    atomic_bytes = sum(4 * 8 * int(valid[j]) for i in range(n) for j in nbrs[i])
    ctx = binding.Context(0)
    FS.register_device_ring(ctx, cams, depth, normal, conf, rng, nbrs, gray)

    def restore():
        depth.copy_(d0); conf.copy_(c0)
        torch.cuda.synchronize()

    for adjust in (False, True):
        name = "adjust" if adjust else "strict"
        if args.route in ("stage", "both"):
            ms, wall, st = [], [], None
            for _ in range(args.steps + 1):     # (the first is a warm-up: allocations, code objects)
                restore()
                t0 = time.perf_counter()
                st = ctx.filter_sequence(range(n), max_neighbors=args.neighbors, adjust=adjust)
                wall.append((time.perf_counter() - t0) * 1e3); ms.append(st["ms_device"])
            print(json.dumps({"route": "stage", "variant": name, "images": n, "size": [w, h], "neighbors": args.neighbors, "batch": st["batch"],
                              "device_ms_best": round(min(ms[1:]), 3), "device_ms": [round(x, 3) for x in ms[1:]], "wall_ms_best": round(min(wall[1:]), 3),
                              "wall_ms": [round(x, 3) for x in wall[1:]], "ms_per_image": round(min(wall[1:]) / n, 4), "device_gib": round(st["device_bytes"] / 2 ** 30, 2),
                              "discarded": st["n_discarded"], "processed": st["n_processed"], "atomic_bytes": atomic_bytes}), flush=True)
        if args.route in ("per-image", "both"):
            restore()
            wall = []
            for _ in range(args.steps + 1):
                t0 = time.perf_counter()
                nd = 0
                for i in range(n):
                    nd += ctx.filter(i, nbrs[i], adjust=adjust)[3]
                wall.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"route": "per-image", "variant": name, "images": n, "size": [w, h], "neighbors": args.neighbors, "tree": args.tree or "this checkout",
                              "wall_ms_best": round(min(wall[1:]), 3), "wall_ms": [round(x, 3) for x in wall[1:]], "ms_per_image": round(min(wall[1:]) / n, 4),
                              "discarded": nd}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

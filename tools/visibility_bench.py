"""diagnostic (not a test): time hcmvs_point_cloud_filter (DensifyPointCloud --filter-point-cloud < 0) on a synthetic cloud of the
size of configs[2]'s fused cloud -- about 23.7 M points over a ring of 64 cameras at 1080p, 1 % floaters (tests/test_gpu_visibility.py
ring_cloud) -- and print the counters of the call as one JSON line.  usage: visibility_bench.py [points] [cameras]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
binding = importlib.import_module("hc-mvs_amd.binding")
from test_gpu_visibility import ring_cloud

N = int(float(sys.argv[1])) if len(sys.argv) > 1 else 24_000_000
M = int(sys.argv[2]) if len(sys.argv) > 2 else 64
t0 = time.perf_counter()
xyz, nv, vi, cams, floaters = ring_cloud(N, n_cams=M)
t1 = time.perf_counter()
ctx = binding.Context(0)
res = {}
for rep in range(2):  # the first call pays the kernels' first load
    t2 = time.perf_counter()
    vis, kept = ctx.point_cloud_filter(xyz, nv, vi, cams, th_remove=-1)
    wall = time.perf_counter() - t2
    st = ctx.visibility_stats
    res = dict(points=len(xyz), cameras=M, pairs=st["pairs"], ms_device=round(st["ms_device"], 2), wall_s=round(wall, 3),
               candidates_per_pair=round(st["candidates"] / max(st["pairs"], 1), 2), hits=st["hits"], fallback_pairs=st["fallback_pairs"],
               device_mib=round(st["device_bytes"] / 2 ** 20, 1), kept=len(kept), floaters_removed=float(np.isin(floaters, kept, invert=True).mean()),
               gen_s=round(t1 - t0, 1))
    print(json.dumps(res), flush=True)
ctx.close()

"""diagnostic (not a test): time hcmvs_sample_mesh (DensifyPointCloud --sample-mesh) on a synthetic height field of about 2 M triangles
sampled to about 50 M points, without and with a texture, and print the counters of each call as one JSON line.
usage: sample_mesh_bench.py [grid side] [points]"""
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
binding = importlib.import_module("hc-mvs_amd.binding")

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
P = int(float(sys.argv[2])) if len(sys.argv) > 2 else 50_000_000
t0 = time.perf_counter()
r = np.random.default_rng(1)
g = np.linspace(0, 1, N + 1, dtype=np.float32)
u, v = np.meshgrid(g, g, indexing="xy")
V = np.stack([100 * u, 100 * v, 0.05 * r.standard_normal(u.shape)], -1).reshape(-1, 3).astype(np.float32)
i = (np.arange(N, dtype=np.int64)[:, None] * (N + 1) + np.arange(N)[None, :]).ravel()
Fc = np.concatenate([np.stack([i, i + 1, i + N + 2], -1), np.stack([i, i + N + 2, i + N + 1], -1)]).astype(np.uint32)
tc = np.stack([u, v], -1).reshape(-1, 2).astype(np.float32)[Fc]
tex = r.integers(0, 256, (2048, 2048, 3)).astype(np.uint8)
t1 = time.perf_counter()
ctx = binding.Context(0)
for textured in (False, True):
    for rep in range(2):  # the first call pays the kernels' first load
        kw = dict(texcoords=tc, texture_bgr=tex) if textured else {}
        t2 = time.perf_counter()
        st = ctx.sample_mesh(V, Fc, -P, seed=1, count_only=True, **kw)[3]
        t3 = time.perf_counter()
        xyz, fid, bgr, st2 = ctx.sample_mesh(V, Fc, -P, seed=1, **kw)
        t4 = time.perf_counter()
        print(json.dumps(dict(faces=len(Fc), vertices=len(V), textured=textured, points=st2["n_points"], area=round(st2["area"], 3),
                              density=round(st2["density"], 3), count_only_ms_device=round(st["ms_device"], 2), count_only_wall_s=round(t3 - t2, 3),
                              ms_device=round(st2["ms_device"], 2), wall_s_count_and_fill=round(t4 - t3, 3), device_mib=round(st2["device_bytes"] / 2 ** 20, 1),
                              gen_s=round(t1 - t0, 1))), flush=True)
        del xyz, fid, bgr
ctx.close()

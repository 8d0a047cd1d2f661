"""diagnostic (not a test): the initial depth / normal maps of one image, device form against host form.  Per size (1920 x 1080 and
3840 x 2160, each with --points sparse points inside the image: 6 000, about what an image of the configs[2] sparse cloud sees), first
call discarded:
  device: Context.triangulate_init_device into a torch slab: ms_host, ms_device, wall of the call, wall of call + synchronize
  host:   binding's hcmvs_triangulate_points into numpy, then the copy into the slab as distributed.densify_scene makes it for tuple
          entries (pageable torch.from_numpy(..).to(dev)), and the copy out of page-locked tensors (with and without the memcpy into them)
  splat:  the same two forms of the splat, briefly
--host-lib PATH times the host form of ANOTHER build of libhcmvs_hip.so (e.g. the parent commit's) in the same process, alternating with
this tree's, so the two host forms see the same machine state.  One JSON line per size; times are median [min, max] over --reps.
usage: init_bench.py [--reps 7] [--points 6000] [--host-lib other/libhcmvs_hip.so] [--out profiles/init_bench.txt]"""
import argparse
import ctypes as C
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
binding = importlib.import_module("hc-mvs_amd.binding")

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--points", type=int, default=6000)
ap.add_argument("--host-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def stat(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 3), round(ts[0], 3), round(ts[-1], 3)]


def host_form(L, w, h, K, R, Cc, pts):
    """hcmvs_triangulate_points of library L into fresh numpy maps; returns (ms, depth, normal, d_min, d_max)"""
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.hcmvs_triangulate_points.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, fp, C.c_int32, C.c_float, C.c_int32, fp, fp, fp, fp]
    t0 = time.perf_counter()
    d = np.zeros((h, w), np.float32); n = np.zeros((h, w, 3), np.float32)
    lo, hi = C.c_float(), C.c_float()
    rc = L.hcmvs_triangulate_points(w, h, K.ctypes.data_as(dp), R.ctypes.data_as(dp), Cc.ctypes.data_as(dp), pts.ctypes.data_as(fp), len(pts), 0.0, 1,
                                    d.ctypes.data_as(fp), n.ctypes.data_as(fp), C.byref(lo), C.byref(hi))
    assert rc == 0
    return (time.perf_counter() - t0) * 1e3, d, n, lo.value, hi.value


dev = torch.device("cuda", 0)
ctx = binding.Context(0)
other = C.CDLL(os.path.abspath(args.host_lib)) if args.host_lib else None
lines = []
for (w, h) in ((1920, 1080), (3840, 2160)):
    f = 1600.0 * w / 1920
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float64)
    R = np.eye(3); Cc = np.zeros(3)
    rng = np.random.RandomState(11)
    px = rng.uniform(0, w, args.points); py = rng.uniform(0, h, args.points)
    z = 10.0 + 0.8 * np.sin(px / w * 9.0) * np.cos(py / h * 7.0) + 0.05 * rng.standard_normal(args.points)
    pts = np.ascontiguousarray(np.stack([(px - K[0, 2]) * z / f, (py - K[1, 2]) * z / f, z], -1), np.float32)
    ctx.upload_view(0, np.zeros((h, w), np.float32), K, R, Cc)
    hw = h * w
    slab = torch.zeros(5 * hw, dtype=torch.float32, device=dev)
    pin_d = torch.empty(hw, dtype=torch.float32).pin_memory(); pin_n = torch.empty(3 * hw, dtype=torch.float32).pin_memory()
    torch.cuda.synchronize(dev)
    base = slab.data_ptr()
    T = dict(ms_host=[], ms_device=[], call=[], call_sync=[], host=[], host_other=[], pageable=[], pinned=[], pinned_staged=[],
             splat_dev=[], splat_host=[])
    st = None
    for rep in range(args.reps + 1):
        keep = rep > 0      # the first call pays the kernels' first load and the first allocations
        # device form
        t0 = time.perf_counter()
        dmin, dmax = ctx.triangulate_init_device(0, pts, base, base + 4 * hw)
        t1 = time.perf_counter()
        ctx.synchronize()
        t2 = time.perf_counter()
        st = ctx.init_stats()
        got_d = slab[:hw].cpu().numpy().reshape(h, w); got_n = slab[hw:4 * hw].cpu().numpy().reshape(h, w, 3)
        # host forms, alternating
        ms_o = host_form(other, w, h, K, R, Cc, pts)[0] if other is not None else None
        ms_h, d0, n0, lo, hi = host_form(binding.lib(), w, h, K, R, Cc, pts)
        same = bool(np.array_equal(got_d, d0) and np.array_equal(got_n, n0) and (dmin, dmax) == (lo, hi))
        # the copy as densify_scene makes it for a tuple entry
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        slab[:hw] = torch.from_numpy(np.ascontiguousarray(d0, np.float32)).reshape(-1).to(dev)
        slab[hw:4 * hw] = torch.from_numpy(np.ascontiguousarray(n0, np.float32)).reshape(-1).to(dev)
        torch.cuda.synchronize(dev)
        t4 = time.perf_counter()
        # page-locked: memcpy into pinned tensors, then the transfer
        pin_d.copy_(torch.from_numpy(d0).reshape(-1)); pin_n.copy_(torch.from_numpy(n0).reshape(-1))
        t5 = time.perf_counter()
        slab[:hw].copy_(pin_d, non_blocking=True); slab[hw:4 * hw].copy_(pin_n, non_blocking=True)
        torch.cuda.synchronize(dev)
        t6 = time.perf_counter()
        # the splat, both forms
        t7 = time.perf_counter()
        ctx.splat_init_device(0, pts, base, base + 4 * hw)
        ctx.synchronize()
        t8 = time.perf_counter()
        ctx.splat_init(0, pts)
        t9 = time.perf_counter()
        if keep:
            T["ms_host"].append(st["ms_host"]); T["ms_device"].append(st["ms_device"]); T["call"].append((t1 - t0) * 1e3); T["call_sync"].append((t2 - t0) * 1e3)
            T["host"].append(ms_h); T["pageable"].append((t4 - t3) * 1e3); T["pinned"].append((t6 - t5) * 1e3); T["pinned_staged"].append((t6 - t4) * 1e3)
            T["splat_dev"].append((t8 - t7) * 1e3); T["splat_host"].append((t9 - t8) * 1e3)
            if ms_o is not None:
                T["host_other"].append(ms_o)
    rec = dict(size=[w, h], points=len(pts), n_used=st["n_used"], n_faces=st["n_faces"], tile_entries=st["n_tile_entries"],
               covered=st["covered_pixels"], cover_hits=st["cover_hits"], device_kib=round(st["device_bytes"] / 1024, 1), bit_exact=same,
               device=dict(ms_host=stat(T["ms_host"]), ms_device=stat(T["ms_device"]), call_ms=stat(T["call"]), call_sync_ms=stat(T["call_sync"])),
               host=dict(triangulate_points_ms=stat(T["host"]), pageable_copy_ms=stat(T["pageable"]), pinned_copy_ms=stat(T["pinned"]),
                         pinned_copy_with_staging_ms=stat(T["pinned_staged"])),
               splat=dict(device_call_sync_ms=stat(T["splat_dev"]), host_ms=stat(T["splat_host"])))
    if other is not None:
        rec["host_other_lib"] = dict(path=args.host_lib, triangulate_points_ms=stat(T["host_other"]))
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
    del slab, pin_d, pin_n
ctx.close()
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")

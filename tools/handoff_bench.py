"""diagnostic (not a test): the hand-off between two pyramid levels, device form against host form, at the size of a real schedule step:
--images maps (64) of 960 x 540 brought to 1920 x 1080, in both modes (init: INTER_CUBIC + clean-up; hint: INTER_AREA + clean-up).
  device: Context.handoff_maps_device, ONE call for all images: ms_device (HIP events around the kernels) and the wall time of the call
          (it ends in the call's one synchronisation), over --reps calls after a discarded first one
  host:   binding.handoff_maps on the same maps, once per mode in the same session (a single-threaded loop, as the stand-alone driver's)
Bytes moved = what the kernel must move: every destination pixel written once (16 B), every source pixel read once (16 B); the rate
is that over ms_device.  The maps: depths in 1 .. 9 with 10 % holes, normals of length 0.5 .. 1.5 (one map, rolled per image).
One JSON line per mode.
usage: handoff_bench.py [--images 64] [--reps 7] [--host-images 64] [--out profiles/handoff_64x1080p.txt]"""
import argparse
import importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
binding = importlib.import_module("hc-mvs_amd.binding")

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-images", type=int, default=64, help="images the host form is timed on (its time is reported per image and for all)")
ap.add_argument("--src", type=int, nargs=2, default=(960, 540))
ap.add_argument("--dst", type=int, nargs=2, default=(1920, 1080))
ap.add_argument("--out", default=None)
args = ap.parse_args()


def stat(ts):
    ts = sorted(ts)
    return [round(ts[len(ts) // 2], 3), round(ts[0], 3), round(ts[-1], 3)]


(sw, sh), (dw, dh) = args.src, args.dst
N = args.images
rng = np.random.RandomState(5)
d0 = rng.uniform(1.0, 9.0, (sh, sw)).astype(np.float32)
d0[rng.uniform(size=(sh, sw)) < 0.1] = 0
n0 = rng.normal(size=(sh, sw, 3)).astype(np.float32)
n0 = (n0 / np.linalg.norm(n0, axis=-1, keepdims=True) * rng.uniform(0.5, 1.5, (sh, sw, 1))).astype(np.float32)
src_d = np.stack([np.roll(d0, 7 * i, 1) for i in range(N)]); src_n = np.stack([np.roll(n0, 7 * i, 1) for i in range(N)])

dev = torch.device("cuda", 0)
ctx = binding.Context(0)
t_sd = torch.from_numpy(src_d).to(dev); t_sn = torch.from_numpy(src_n).to(dev)
t_dd = torch.empty(N, dh * dw, dtype=torch.float32, device=dev); t_dn = torch.empty(N, dh * dw * 3, dtype=torch.float32, device=dev)
torch.cuda.synchronize(dev)
bytes_moved = N * 16 * (dw * dh + sw * sh)
lines = []
for mode in ("init", "hint"):
    items = [dict(src_depth=t_sd[i].data_ptr(), src_normal=t_sn[i].data_ptr(), src_w=sw, src_h=sh, dst_depth=t_dd[i].data_ptr(), dst_normal=t_dn[i].data_ptr(),
                  dst_w=dw, dst_h=dh, d_min=2.0, d_max=7.0) for i in range(N)]
    ms_dev, wall = [], []
    for rep in range(args.reps + 1):        # the first call pays the kernels' first load and the first allocations
        t0 = time.perf_counter()
        res = ctx.handoff_maps_device(items, mode)
        t1 = time.perf_counter()
        st = ctx.handoff_stats()
        if rep:
            ms_dev.append(st["ms_device"]); wall.append((t1 - t0) * 1e3)
    # the host form on the same maps
    nh = min(args.host_images, N)
    maps = [dict(depth=src_d[i], normal=src_n[i], dst_w=dw, dst_h=dh, d_min=2.0, d_max=7.0) for i in range(nh)]
    t0 = time.perf_counter()
    host = binding.handoff_maps(maps, mode)
    host_ms = (time.perf_counter() - t0) * 1e3
    got_d = t_dd[:nh].cpu().numpy(); got_n = t_dn[:nh].cpu().numpy()
    same = all(np.array_equal(got_d[i].reshape(dh, dw), host[i]["depth"]) and np.array_equal(got_n[i].reshape(dh, dw, 3), host[i]["normal"], equal_nan=True) and
               (res[i]["d_min"], res[i]["d_max"], res[i]["n_valid"], res[i]["n_clamped"], res[i]["n_rescaled"]) ==
               (host[i]["d_min"], host[i]["d_max"], host[i]["n_valid"], host[i]["n_clamped"], host[i]["n_rescaled"]) for i in range(nh))
    med = stat(ms_dev)[0]
    rec = dict(mode=mode, images=N, src=[sw, sh], dst=[dw, dh], bytes_moved=bytes_moved, bit_exact=bool(same),
               device=dict(ms_device=stat(ms_dev), call_wall_ms=stat(wall), tb_per_s=round(bytes_moved / (med * 1e-3) / 1e12, 3)),
               host=dict(images=nh, ms=round(host_ms, 1), ms_per_image=round(host_ms / nh, 2), ms_all_images=round(host_ms / nh * N, 1)),
               counters={k: st[k] for k in ("n_pixels", "n_valid", "n_clamped", "n_rescaled", "n_empty")})
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)
ctx.close()
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")

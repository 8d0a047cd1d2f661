"""diagnostic (not a test): ms_device of the speckle filter (Context.remove_speckles_device; HIP events around its five launches) at
1920 x 1080, speckle_size 100, default threshold, for 1 map and for a batch of 32 in ONE call, three calls each:
  bench final maps        the maps one bench.py step leaves (its four scenes, 8 source views, 8 sweeps)
  all valid, one segment  every depth 2.0: the worst case for the atomics, one segment per map
and one bench map against the numpy statement (tests/speckle_ref.py), bit for bit.
usage: speckle_bench.py > profiles/speckle_1080p.txt"""
import importlib, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
binding = importlib.import_module("hc-mvs_amd.binding")
W, H, B = bench.W, bench.H, 32
HW = W * H
def main():
    dev = torch.device("cuda", 0)
    ctx = binding.Context(0)
    t0 = time.time()
    scenes = dict(enumerate(bench.make_scenes([(2 + k, 5 + k) for k in range(4)])))
    print("scenes %.1f s" % (time.time() - t0), flush=True)
    params = binding.default_params(adapthalfwin=bench.AHW, n_estimation_iters=bench.SWEEPS, it_external=0, n_external_iters=1, seed=1234)
    allwork = torch.empty(B, 5 * HW, dtype=torch.float32, device=dev)
    items, keep = [], []
    for b_ in range(B):
        views, pts = scenes[b_ % 4]
        slab = torch.from_numpy(np.stack([v["gray"] for v in views])).to(dev); keep.append(slab)
        for i, v in enumerate(views):
            ctx.set_view_device(100 * b_ + i, W, H, slab[i].data_ptr(), v["K"], v["R"], v["C"])
        ctx.shapes[100 * b_] = (H, W)
        d0, n0, dmin, dmax = ctx.splat_init(100 * b_, pts)
        allwork[b_].copy_(torch.cat([torch.from_numpy(d0).reshape(-1), torch.from_numpy(n0).reshape(-1), torch.zeros(HW)]).to(dev))
        w = allwork[b_]
        items.append(dict(ref_id=100 * b_, src_ids=[100 * b_ + i for i in range(1, bench.N_SRC + 1)], d_min=dmin, d_max=dmax, d_depth=w.data_ptr(),
                          d_normal=w.data_ptr() + HW * 4, d_conf=w.data_ptr() + 4 * HW * 4, seed_offset=b_))
    torch.cuda.synchronize()
    ctx.estimate_batch_device(items, params); ctx.synchronize()
    print("estimated %.1f s" % (time.time() - t0), flush=True)
    final = allwork.clone()
    flat = torch.full_like(allwork, 2.0)
    def sp(store, n):
        return [dict(width=W, height=H, d_depth=store[b].data_ptr(), d_normal=store[b].data_ptr() + HW * 4, d_conf=store[b].data_ptr() + 4 * HW * 4) for b in range(n)]
    work = torch.empty_like(allwork)
    for name, src in (("bench final maps", final), ("all valid, one segment", flat)):
        for n in (1, 32):
            for rep in range(3):
                work.copy_(src); torch.cuda.synchronize()
                st = ctx.remove_speckles_device(sp(work, n), None, 100)
                print("%s, %2d maps, run %d: %.3f ms device; valid %d segments %d small %d removed %d largest %d; scratch %.1f MB" %
                      (name, n, rep, st["ms_device"], st["n_valid"], st["n_segments"], st["n_small"], st["n_removed"], st["largest"], st["device_bytes"] / 1e6), flush=True)
    # cross-check one bench map against the statement
    import speckle_ref as R
    d = final[0][:HW].view(H, W).cpu().numpy()
    t1 = time.time(); want = R.remove_speckles(d, speckle_size=100); print("statement on one map: %.1f s" % (time.time() - t1))
    work.copy_(final); torch.cuda.synchronize()
    st = ctx.remove_speckles_device(sp(work, 1), None, 100)
    print("1080p map equals the statement:", R.same_bits(work[0][:HW].view(H, W).cpu().numpy(), want["depth"]), {k: st[k] for k in R.COUNTERS} == want["stats"])
    ctx.close()


if __name__ == "__main__":
    main()

"""diagnostic (not a test): what the plane detection (S4) of hcmvs_generate_plane_prior_device costs with and without the clustering of a
plane's inliers (cluster_mul) and the refit of a round's winner (refit_iters, S4r), from
hcmvs_plane_prior_stats.ms_rounds (host clock between the waits):
  doorway  96 x 80, tests/plane_prior_cases.py::doorway, cluster_mul 0 and 2, then refit_iters 4
  crease   1920 x 1080, the two planes of tests/plane_prior_cases.py::crease at a focal length of 1800, region = the middle half of the
           rows, cluster_mul 0 and 7, then refit_iters 4
--reps calls each after a discarded first one (it allocates).  One JSON line per scene, cluster_mul and refit_iters: ms_rounds of every call,
rounds, rounds with a winner, planes, and -- against the cluster_mul 0, refit_iters 0 line of the scene -- the extra time per round that has
a winner.
--root <tree> measures the library of another checkout (one without the cluster_mul or the refit_iters field runs the lines it has).
usage: plane_prior_bench.py [--reps 3] [--root .] [--out profiles/plane_prior_cluster.txt]"""
import argparse
import importlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--root", default=ROOT)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch
binding = importlib.import_module("hc-mvs_amd.binding")
import plane_prior_cases as PC


def big_crease(w=1920, h=1080, focal=1800.0):
    rng = np.random.RandomState(100)
    K = PC._K(w, h, focal)
    ray = PC._rays(K, w, h)
    n1 = np.array([0.45, 0.05, 1.0]); n1 /= np.linalg.norm(n1)
    n2 = np.array([-0.5, -0.08, 1.0]); n2 /= np.linalg.norm(n2)
    t1, t2 = PC._plane_depth(ray, n1, n1[2] * 6.0), PC._plane_depth(ray, n2, n2[2] * 6.0)
    left = t1 <= t2
    region = np.zeros((h, w), bool); region[h // 4:h - h // 4] = True
    nrm = np.where(left[..., None], PC._facing(n1, ray), PC._facing(n2, ray))
    return PC._case(rng, K, np.minimum(t1, t2), nrm, region, [], depth_noise=0.003, outliers=0.05, normal_noise=0.08, bad_conf=0.1)


has_field = hasattr(binding.PlanePriorParams(), "cluster_mul")
has_refit = hasattr(binding.PlanePriorParams(), "refit_iters")
ctx = binding.Context(0)
lines = []
for vid, (name, case, muls) in enumerate((("doorway", PC.doorway(), (0.0, 2.0)), ("crease_1080p", big_crease(), (0.0, 7.0)))):
    h, w = case["depth"].shape
    ctx.upload_view(vid, np.zeros((h, w), np.float32), case["K"], np.eye(3), np.zeros(3))
    ctx.set_prior_region(vid, np.where(case["region"], 255, 7).astype(np.uint16), 255)
    d, n, cf = (torch.from_numpy(np.ascontiguousarray(case[k])).cuda() for k in ("depth", "normal", "conf"))
    prior = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    base = None
    for mul, iters in [(m, 0) for m in muls] + [(0.0, 4)]:
        if (mul and not has_field) or (iters and not has_refit):
            continue
        p = binding.default_plane_prior_params(seed=1, **(dict(cluster_mul=mul) if has_field else {}), **(dict(refit_iters=iters) if has_refit else {}))
        ms, st = [], None
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            _, st = ctx.generate_plane_prior_device(vid, d.data_ptr(), n.data_ptr(), cf.data_ptr(), prior.data_ptr(), None, p)
            if rep:
                ms.append(round(st["ms_rounds"], 4))
        rounds = ctx.plane_prior_trace(vid)["rounds"]
        winners = int((rounds[:, 0] >= 0).sum())
        line = dict(scene=name, size=[w, h], cluster_mul=mul, refit_iters=iters, fitting_samples=st["fitting_samples"], rounds=st["rounds"], winners=winners, planes=st["planes"],
                    ms_rounds=ms, ms_device=round(st["ms_device"], 3), ms_search=round(st["ms_search"], 3))
        if mul == 0 and iters == 0:
            base = line
        elif base is not None:   # (the rounds differ once a plane is split: per round without a winner the cluster_mul 0 line's cost is taken off)
            per_round0 = float(np.median(base["ms_rounds"])) / max(base["rounds"], 1)
            line["extra_ms_per_winner"] = round((float(np.median(ms)) - per_round0 * st["rounds"]) / max(winners, 1), 4)
            line.update(cluster_rejects=st["cluster_rejects"], cluster_left=st["cluster_left"])
            if iters:
                line.update(refit_rounds=st["refit_rounds"], refit_steps=st["refit_steps"])
        lines.append(line)
        print(json.dumps(line), flush=True)
ctx.close()
if args.out:
    with open(args.out, "w") as f:
        f.writelines(json.dumps(l) + "\n" for l in lines)

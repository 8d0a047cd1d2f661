"""helper of the filter-stage tests (test infrastructure only): the scene-level oracle of Scene::DenseReconstructionFilter
(SceneDensify.cpp:4100-4185) -- a Python loop over oracle_lib.filter_depthmap on a SNAPSHOT of the maps ("load the filtered maps after
all depth-maps were filtered", :4134-4135) --, the in-place loop it must not be confused with, a stand-in context that runs the stage
with the oracle, and scenes: the small one with every special case in it, and a full-size ring whose maps are made on the device."""
import importlib

import numpy as np

import oracle_lib as O
import scene_oracle as S
from fusion_scene import make_maps

synth = importlib.import_module("hc-mvs_amd.synth")


def usable_neighbors(maps, i, max_neighbors):
    """the first max_neighbors entries of image i's neighbour list that have maps (SceneDensify.cpp:4116-4131: others are passed over)"""
    return [n for n in maps[i]["neighbors"] if n < len(maps) and maps[n] is not None and maps[n].get("depth") is not None][:max_neighbors]


def stage(maps, ids, max_neighbors=8, adjust=True, n_min_views=2, n_min_views_adjust=1, thr=0.01, in_place=False):
    """maps: list indexed by image id of dicts (K, R, C, depth, normal, conf, d_min, d_max, neighbors); None or depth None = no maps.
    in_place=False is the stage: every image is filtered from the maps as they are on entry.  in_place=True filters image after image,
    each seeing what the images before it left (NOT the stage).
    Returns (maps after the stage: new list, arrays copied; {id: (processed, discarded)} of the filtered images; [skipped ids])"""
    cur = [None if m is None else dict(m) for m in maps]
    out = [None if m is None else dict(m) for m in maps]
    counts, skipped = {}, []
    for i in ids:
        if i >= len(maps) or maps[i] is None or maps[i].get("depth") is None:
            skipped.append(i)
            continue
        src = out if in_place else cur
        nbs = usable_neighbors(src, i, max_neighbors)
        sub = [dict(src[k], neighbors=[]) for k in [i] + nbs]          # image 0 of the call and its neighbours 1 .. N
        ok, d, c, npr, nd = (0, None, None, 0, 0) if not nbs else O.filter_depthmap(sub, 0, list(range(1, len(sub))), adjust=adjust,
                                                                                    n_min_views=n_min_views, n_min_views_adjust=n_min_views_adjust, thr=thr)
        if not ok:                                                      # SceneDensify.cpp:3016-3019: FilterDepthMap returns false, the maps stay
            skipped.append(i)
            continue
        out[i] = dict(out[i], depth=d, conf=c)
        counts[i] = (npr, nd)
    return out, counts, skipped


class FilterOracleContext(S.OracleContext):
    """tests/scene_oracle.OracleContext + the filter stage, with the oracle as its engine and host memory as device memory"""

    def filter_sequence(self, ids, max_neighbors=8, adjust=True, n_min_views=2, n_min_views_adjust=1, depth_diff_threshold=0.01):
        cur = self._dicts()
        out, counts, skipped = stage(cur, list(ids), max_neighbors, adjust, n_min_views, n_min_views_adjust, depth_diff_threshold)
        for i in counts:
            cur[i]["depth"][...] = out[i]["depth"]; cur[i]["conf"][...] = out[i]["conf"]
        return dict(n_processed=sum(v[0] for v in counts.values()), n_discarded=sum(v[1] for v in counts.values()), n_filtered=len(counts),
                    n_skipped=len(skipped), image_processed=[counts.get(i, (0, 0))[0] for i in ids], image_discarded=[counts.get(i, (0, 0))[1] for i in ids])


def issue_scene():
    """the scene the stage was characterised on: six views of 144x112, noisy maps with outliers and holes"""
    return make_maps(w=144, h=112, f=130.0, n_views=6, noise=0.002, outliers=0.06, holes=0.05)


def crop_view(m, x0, y0, w, h):
    """the same camera looking through a smaller window: maps cropped, principal point shifted -- a view of another size"""
    K = np.array(m["K"], np.float64).copy()
    K[0, 2] -= x0; K[1, 2] -= y0
    out = dict(m, K=K)
    for k in ("depth", "conf", "normal", "gray", "bgr", "gt"):
        out[k] = np.ascontiguousarray(m[k][y0:y0 + h, x0:x0 + w])
    return out


def special_scene():
    """issue_scene with every special case of the stage in it: view 2 has another size (120x96), image 6 is registered without maps and
    leads the neighbour lists of images 0 and 3, image 5 has a single usable neighbour (too few for n_min_views = 2: skipped).
    Returns maps (list of 7, maps[6] has depth None), ids to filter (0 .. 6)"""
    maps, _ = issue_scene()
    maps[2] = crop_view(maps[2], 13, 9, 120, 96)
    blank = dict(maps[0], depth=None, normal=None, conf=None, neighbors=[0, 1])
    maps.append(blank)
    maps[0] = dict(maps[0], neighbors=[6] + maps[0]["neighbors"])
    maps[3] = dict(maps[3], neighbors=maps[3]["neighbors"][:1] + [6] + maps[3]["neighbors"][1:])
    maps[5] = dict(maps[5], neighbors=[6, maps[5]["neighbors"][0]])
    return maps, list(range(7))


def upload(ctx, maps):
    """register views, maps (the context's own copies) and neighbour lists of `maps` on a binding.Context"""
    for i, m in enumerate(maps):
        ctx.upload_view(i, m["gray"], m["K"], m["R"], m["C"], bgr=m.get("bgr"))
        if m.get("depth") is not None:
            ctx.set_depthmap(i, m["depth"], m["normal"], m["conf"], m["d_min"], m["d_max"])
        ctx.set_neighbors(i, m["neighbors"])


def device_ring(n, w, h, n_neighbors, dev, seed=5, noise=0.002, outliers=0.06, holes=0.05):
    """n cameras on a ring around hc-mvs_amd/synth.Scene's plane and sphere, their ground-truth depth maps computed ON THE DEVICE with torch
    (float64 ray casting, as Scene.render does it), then noise, outliers and holes as fusion_scene.make_maps adds them.  Returns
    (cams: list of (K, R, C), depth [n, h, w], normal [n, h, w, 3], conf [n, h, w] f32 device tensors, (d_min, d_max), neighbour lists:
    the n_neighbors nearest cameras of the ring, nearest first)"""
    import torch
    sc = synth.Scene(seed)
    f = 1600.0 * w / 1920
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1]], np.float64)
    g = torch.Generator(device=dev); g.manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
    X0 = torch.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], torch.ones_like(xs)], -1)
    pn = torch.tensor(sc.plane_n, device=dev); sphere_c = torch.tensor(sc.sphere_c, device=dev)
    cams = []
    depth = torch.empty(n, h, w, dtype=torch.float32, device=dev); normal = torch.empty(n, h, w, 3, dtype=torch.float32, device=dev)
    conf = torch.empty(n, h, w, dtype=torch.float32, device=dev)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=dev)
    for i in range(n):
        ang = 2 * np.pi * i / n
        C = np.array([0.9 * np.cos(ang), 0.7 * np.sin(ang), 0.02 * (i % 5)])
        R = synth.look_at(C, np.array([0.0, 0.0, sc.depth0]))
        cams.append((K.copy(), R, C))
        Rt = torch.tensor(R, device=dev); Ct = torch.tensor(C, device=dev)
        d = X0 @ Rt
        tp = (sc.plane_d - float(C @ sc.plane_n)) / (d @ pn)
        tp = torch.where(tp > 0, tp, inf)
        oc = Ct - sphere_c
        a = (d * d).sum(-1); b = 2 * (d @ oc); c = float(oc @ oc) - sc.sphere_r ** 2
        disc = b * b - 4 * a * c
        ts = torch.where(disc > 0, (-b - torch.sqrt(torch.clamp(disc, min=0))) / (2 * a), inf)
        ts = torch.where(ts > 0, ts, inf)
        hit = ts < tp
        t = torch.where(hit, ts, tp)
        P = Ct + d * t[..., None]
        nw = torch.where(hit[..., None], (P - sphere_c) / sc.sphere_r, -pn.expand_as(P))
        nc = nw @ Rt.T
        nc = torch.where(((nc * X0).sum(-1) > 0)[..., None], -nc, nc)
        dd = t.to(torch.float32)
        dd = dd * (1 + noise * torch.randn(h, w, generator=g, device=dev))
        m = torch.rand(h, w, generator=g, device=dev) < outliers
        dd = torch.where(m, dd * (0.6 + 0.9 * torch.rand(h, w, generator=g, device=dev)), dd)
        dd = torch.where(torch.rand(h, w, generator=g, device=dev) < holes, torch.zeros_like(dd), dd)
        dd[:7] = 0; dd[-7:] = 0; dd[:, :7] = 0; dd[:, -7:] = 0
        depth[i] = dd; normal[i] = nc.to(torch.float32)
        conf[i] = torch.where(dd > 0, 0.5 + 0.45 * torch.rand(h, w, generator=g, device=dev), torch.zeros_like(dd))
    Cs = np.stack([c[2] for c in cams])
    nbrs = [[int(j) for j in np.argsort(np.linalg.norm(Cs - Cs[i], axis=1), kind="stable") if j != i][:n_neighbors] for i in range(n)]
    return cams, depth, normal, conf, (0.5 * sc.depth0, 2.0 * sc.depth0), nbrs


def register_device_ring(ctx, cams, depth, normal, conf, rng, nbrs, gray):
    """views (sharing one device gray image: the stage reads cameras and maps only), device maps and neighbour lists of device_ring()"""
    n, h, w = depth.shape
    for i in range(n):
        K, R, C = cams[i]
        ctx.set_view_device(i, w, h, gray.data_ptr(), K, R, C)
        ctx.set_depthmap_device(i, depth[i].data_ptr(), normal[i].data_ptr(), conf[i].data_ptr(), rng[0], rng[1])
        ctx.set_neighbors(i, nbrs[i])

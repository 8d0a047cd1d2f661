"""Multi-GPU sharding of the densify path: one process per GPU, torch.distributed (backend "nccl" = RCCL over
xGMI on ROCm; "gloo" on CPU for tests).

Depth maps are independent units given the read-only images and cameras of their source views, so reference
images are sharded over the ranks with NO collective on the estimation path; the only exchange is one all-gather
of the packed {depth, normal, conf} maps (20 B/px) before fusion, because fusing image A reads and writes every
neighbour's map (SceneDensify.cpp:3381-3449).  SURVEY.md section 8e.
"""
import torch
import torch.distributed as dist

FLOATS_PER_PIXEL = 5  # depth + normal xyz + conf


def shard_order(order, world):
    """image -> rank map: position k of the fusion order (best connected first, SceneDensify.cpp:3302) goes to
    rank k mod world, so ranks are load balanced.  Returns per-rank lists of image ids."""
    return [list(order[r::world]) for r in range(world)]


def plan_order(ids, n_neighbors):
    """the fusion order (SceneDensify.cpp:3285-3302): the images `ids` by decreasing number of neighbours, equal counts in the order
    given (a stable sort).  n_neighbors: {id: count} or a sequence indexed by id"""
    return sorted(ids, key=lambda i: -int(n_neighbors[i]))


def plan_scene(ctx, cameras, sizes, xyz, n_views, view_ids, number_views=5, **params):
    """What densify_scene expects from the caller, from the cameras and the sparse cloud alone: binding.Context.select_views
    (DepthMapsData::SelectViews + the InitViews cut, on the device) for every image, then the fusion order.  Arguments as select_views.
    Returns (srcs, neighbors, order, points) over the images that got views: srcs {id: [source view ids]}, neighbors {id: [neighbour
    ids, decreasing score]}, order = plan_order of those images, points {id: indices into xyz of the image's points} -- densify_scene
    takes init = {id: dict(points=xyz[points[id]])} and triangulates on the rank's device.  A source view whose scale differs from 1 is reported by select_views (srcs as (id, scale));
    densify_scene estimates against the views as uploaded."""
    import numpy as np
    sel = ctx.select_views(cameras, sizes, xyz, n_views, view_ids, number_views=number_views, **params)
    done = [i for i, s in enumerate(sel) if s is not None]
    srcs = {i: [j for j, _ in sel[i]["srcs"]] for i in done}
    neighbors = {i: [n["id"] for n in sel[i]["neighbors"]] for i in done}
    points = {i: np.asarray(sel[i]["points"], np.int64) for i in done}
    return srcs, neighbors, plan_order(done, {i: len(neighbors[i]) for i in done}), points


def slab_index(k, world, n_local):
    """row of order position k in the gathered [world * n_local, ...] tensor (rank-major)"""
    return (k % world) * n_local + k // world


def pack_maps(depth, normal, conf, out=None):
    """(H,W), (H,W,3), (H,W) -> flat [5*H*W] slab: depth | normal | conf"""
    hw = depth.numel()
    if out is None:
        out = torch.empty(FLOATS_PER_PIXEL * hw, dtype=torch.float32, device=depth.device)
    out[:hw] = depth.reshape(-1)
    out[hw:4 * hw] = normal.reshape(-1)
    out[4 * hw:] = conf.reshape(-1)
    return out


def unpack_maps(slab, h, w):
    hw = h * w
    return slab[:hw].view(h, w), slab[hw:4 * hw].view(h, w, 3), slab[4 * hw:].view(h, w)


def allgather_maps(local_slabs, group=None, out=None):
    """local_slabs: [n_local, 5*H*W] (the same n_local on every rank; pad with zero slabs if the images do not
    divide evenly).  Returns [world * n_local, 5*H*W], rank-major, identical on every rank.  One collective:
    with fixed equal slabs RCCL moves each rank's block directly to all peers over its xGMI links.
    out: optional preallocated result buffer (reused by callers that gather every step)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world == 1:
        return local_slabs
    if out is None:
        out = torch.empty((world * local_slabs.shape[0],) + tuple(local_slabs.shape[1:]), dtype=local_slabs.dtype,
                          device=local_slabs.device)
    if local_slabs.is_cuda and dist.get_backend(group) == "gloo":
        # rehearsal on one GPU box (several ranks on device 0): gloo gathers host tensors; staged through pinned-size copies
        host = torch.empty(out.shape, dtype=out.dtype)
        dist.all_gather_into_tensor(host, local_slabs.cpu().contiguous(), group=group)
        out.copy_(host)
        return out
    dist.all_gather_into_tensor(out, local_slabs.contiguous(), group=group)
    return out


def gather_scene_maps(order, my_maps, h, w, group=None, device=None):
    """my_maps: {image id: (depth, normal, conf) tensors} for the images shard_order() gave this rank.
    Returns {image id: (depth, normal, conf)} for every image of `order` on every rank."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    mine = shard_order(order, world)[rank]
    n_local = (len(order) + world - 1) // world
    dev = device if device is not None else (next(iter(my_maps.values()))[0].device if my_maps else torch.device("cpu"))
    slabs = torch.zeros(n_local, FLOATS_PER_PIXEL * h * w, dtype=torch.float32, device=dev)
    for j, img in enumerate(mine):
        pack_maps(*my_maps[img], out=slabs[j])
    allm = allgather_maps(slabs, group)
    return {img: unpack_maps(allm[slab_index(k, world, n_local)], h, w) for k, img in enumerate(order)}


def _device_sync(dev):
    """The context enqueues on a stream of its own (hipStreamNonBlocking, hcmvs_api.cpp hcmvs_create): whatever torch or RCCL wrote into
    buffers the context is about to read -- gathered maps, copied-back slabs -- must have landed first, and the other way round."""
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


HANDOFF_BATCH = 64      # HCMVS_MAX_BATCH: images one hand-off call serves


def _device_map(m, dev):
    """a map of the previous level as a contiguous float32 device tensor: a torch tensor is taken as it is (moved when it lives elsewhere),
    a numpy array is copied in"""
    if not torch.is_tensor(m):
        import numpy as np
        m = torch.from_numpy(np.ascontiguousarray(m, np.float32))
    return m.to(device=dev, dtype=torch.float32).contiguous()


def _handoff(ctx, dev, mode, jobs, w, h):
    """binding.Context.handoff_maps_device over jobs = (image, depth (sh, sw), normal (sh, sw, 3) device tensors, destination depth and normal
    addresses of w x h maps, d_min, d_max), in calls of at most HANDOFF_BATCH items.  Returns the per-item results"""
    for img, d, n, _, _, _, _ in jobs:
        if d.dim() != 2 or tuple(n.shape) != tuple(d.shape) + (3,):
            raise ValueError("densify_scene: the previous maps of image %d are not depth (h, w) and normal (h, w, 3)" % img)
    _device_sync(dev)       # torch filled the sources (and zeroed the slabs) on its own stream
    out = []
    for b0 in range(0, len(jobs), HANDOFF_BATCH):
        out += ctx.handoff_maps_device([dict(src_depth=d.data_ptr(), src_normal=n.data_ptr(), src_w=d.shape[1], src_h=d.shape[0], dst_depth=dd, dst_normal=dn,
                                             dst_w=w, dst_h=h, d_min=lo, d_max=hi) for _, d, n, dd, dn, lo, hi in jobs[b0:b0 + HANDOFF_BATCH]], mode)
    return out


def densify_scene(ctx, views, srcs, neighbors, order, init, params, group=None, device=None, batch=32, capacity=None,
                  fuse_kw=None, n_external_iters=1, postfilter=False, pf_kw=None, interleave=False, masks=None, viewspread=False,
                  geometric_filter=None, gf_kw=None, hints=None, fuse=True, priors=None, prior_params=None,
                  plane_priors=None, plane_prior_params=None, geo=None, speckle_size=0, speckle_diff=None):
    """The multi-rank scene path (BASELINE.json configs[3]) over the C-ABI binding, with the reference's outer
    iterations (SceneDensify.cpp:3684) and the fork's post-filters after outer iterations 1 and 2 (SceneDensify.cpp:3939-3958):

        shard_order
        for it in 0 .. n_external_iters-1:
            per-rank hcmvs_estimate_batch_device of the rank's reference images          (NO collective)
            if postfilter and it in (1, 2):
                all-gather of the packed maps -> hcmvs_postfilter_sequence over ALL images, on every rank -> the rank
                takes its own images' filtered maps back out of the gathered buffer
        all-gather of the packed maps -> hcmvs_set_depthmap_device [+ hcmvs_filter_sequence] + hcmvs_fuse on every rank (identical clouds)

    The post-filter is REPLICATED, not sharded: filtering image k is a fusion over the whole scene whose result (the depths it
    invalidates, the gaps it fills) is what image k + 1's fusion sees, so the images form one sequential chain; every rank runs that
    chain on identical gathered maps with a deterministic kernel, hence every rank holds identical filtered maps and no scatter is
    needed -- the result is independent of the number of ranks.  One all-gather per filtered outer iteration and one before the
    fusion (SURVEY.md 8e budgets exactly that).

    That batch schedule is a DEPARTURE from the reference: there image k is filtered right after its own
    estimate (EVTEstimateDepthMap queues EVTOptimizeDepthMap FIRST, SceneDensify.cpp:3914-3925), so its fusion sees the images > k as
    the previous outer iteration left them and zeroes depths in them before they are estimated again.  interleave=True is that order,
    exactly (the single-thread event order; image ids ascending): in outer iterations 1 and 2 the images are estimated ONE AT A TIME,
    each followed by its post-filter on every rank; the owner of an image broadcasts its fresh maps first.  Nothing runs in parallel
    across ranks there -- it is the exact mode, not the fast one.

    ctx:       binding.Context of this rank's device (one process per GPU)
    views:     {image id: dict(gray, K, R, C[, bgr])} of EVERY image (all the same size).  A rank uploads the gray image only of
               its own reference images and their source views; of the others it registers the camera and the colour image (what
               fusion and the post-filters read), so a 512-image scene does not sit on every GPU eight times
    srcs:      {image id: [source view ids]}            (DepthMapsData::InitViews, SceneDensify.cpp:336-397)
    neighbors: {image id: [neighbour ids]}              (DepthData::neighbors, decreasing importance)
    order:     fusion order, best connected first       (SceneDensify.cpp:3302)
    init:      {image id: entry}, at least for this rank's images.  An entry is (depth0 (H,W), normal0 (H,W,3), d_min, d_max) numpy -- maps
               made on the host, copied in -- or a dict: dict(points=xyz (n,3) [, avg_depth=, add_corners=]) for the triangulation,
               dict(splat=xyz (n,3)) for the splat; the rank's context then rasterises the maps straight into its slab
               (binding.Context.triangulate_init_device / splat_init_device: only the face / point tables travel) and d_min, d_max come
               from that call.  Same bits either way; the two kinds may be mixed.  dict(previous=(depth (sh, sw), normal (sh, sw, 3))): the maps
               of the previous level of the coarse-to-fine schedule (--n-initTriangulate 0), torch device tensors or numpy arrays of ANY size:
               the rank's context hands them over on the device straight into its slab rows (binding.Context.handoff_maps_device, mode
               "init": copied or cv::resize INTER_CUBIC, cleaned), all of the rank's images in calls of at most 64, and d_min, d_max come from
               the call; an image whose previous map holds no valid depth raises ValueError naming it
    hints:     optional {image id: (depth, normal)} of a coarser or equally sized level, tensors or arrays as above: the `restore` variant's
               extra hypothesis.  The rank's context enlarges them on the device (mode "hint": INTER_AREA) into a hint buffer of 16 B per
               pixel of the rank's images, the image's range -- after its init -- is widened by every enlarged depth, and the estimate offers
               the hint on the last sweep of the last outer iteration (hcmvs_batch_item d_hint_depth / d_hint_normal)
    fuse:      False: no final fusion -- the result holds only `maps` (and `ranges`: {id: (d_min, d_max)}), what an intermediate level of
               the schedule needs.  The geometric filter, when asked for, still runs
    params:    binding.Params of the estimate; it_external / n_external_iters are set here
    masks:     optional {image id: (labels (h, w) u16 of any size, [ignored labels])}: --ignore-mask-label for those reference images
               (binding.Context.set_ignore_mask on the rank that estimates them)
    viewspread: --n-viewspread (DepthMap.cpp:1504-1608): from outer iteration 1 on every pixel also tries what its
               source views' own maps hold around the place it projects to.  Batch schedule: before each outer iteration >= 1 the maps of
               ALL images are copied into a second buffer set (one all-gather with several ranks; 20 B per pixel of the scene), which the
               estimates of that iteration read -- every image sees its source views as the previous outer iteration left them, post-filters
               included (a Jacobi order).  interleave=True: the reference's own order -- the images are then estimated one after the other in
               EVERY outer iteration >= 1 (not only the filtered ones) and read the live maps: images < k as this iteration left them (in the
               last one: after the end pass), images > k from the previous one
    priors:    optional {image id: prior depth map (h, w)}, numpy arrays (copied) or torch device tensors (float32, contiguous, read in place):
               depth priors of those REFERENCE images (DepthMap.cpp:941-954), with prior_params =
               dict(para_prior=, sigma_prior=, photo2geo=) (missing keys: the reference's 0.5, 0.2, 2).  The reference's schedule
               (SceneDensify.cpp:983-1031): on outer iteration n_external_iters - 2, after the ordinary estimate of a batch, the priors of its
               images are registered and two extra sweeps run on them, with the sweep indices n_estimation_iters and n_estimation_iters + 1
               (binding.Context.estimate_sweeps_batch_device); on the last outer iteration the priors stay registered.  Whether an estimate
               blends the term is the library's active-prior rule (para_prior > 0 and it_external >= photo2geo).  With fewer than two outer
               iterations the priors are never registered -- the result then carries priors_used = False; nothing is raised.  Priors belong
               to reference images, so ranks exchange nothing new: a rank registers those of its own images.  Not together with viewspread
               or hints (ValueError: the library refuses the combination)
    geo:       the geometric-consistency term: True for the defaults or a dict of the options of
               binding.Context.set_geo_params (para_tapa, para_tapa2, txthreshold, txthreshold2, photo2geo, max_px).  From outer iteration 1
               on every image offers the maps the previous outer iteration left it to the estimates it is a source view of, as for
               viewspread (and across ranks by the same exchange); the term blends from outer iteration max(1, photo2geo) on.  Not together
               with viewspread, hints, priors or plane_priors (ValueError: the library refuses the combinations)
    plane_priors: optional {image id: label image (any size, 16-bit)}: the priors of those REFERENCE images are GENERATED on the device
               (binding.Context.generate_plane_prior_device) from planes fitted inside the pixels labelled
               plane_prior_params.region_label (binding.default_plane_prior_params(); None: the defaults, label 255): on outer iteration
               n_external_iters - 2, after the ordinary estimate of a batch, from each listed image's live maps into a tensor this call
               owns; from there the path is exactly that of priors= (register, sweeps N and N + 1, registered for the last iteration).  The
               result carries plane_prior_maps {id: (h, w) device tensor} and plane_prior_planes {id: plane count} of this rank's images.
               The call OWNS the prior regions of the listed images: it registers them (Context.set_prior_region) and removes them at the end,
               a region the caller had registered for such an image included.  An id in both priors and plane_priors is a ValueError; the refusals of priors= apply (viewspread, hints)
    geometric_filter: None (default: off), "adjust" or "strict": the depth-map filter stage (Scene::DenseReconstructionFilter,
               SceneDensify.cpp:4100-4185; binding.Context.filter_sequence) over ALL images between the final all-gather and the fusion.
               Replicated on every rank like the fusion -- every rank filters identical gathered maps with a deterministic kernel, and a
               second all-gather of the filtered maps would cost more than the filter; gf_kw: max_neighbors, n_min_views,
               n_min_views_adjust, depth_diff_threshold.  The returned `maps` are the filtered ones, `filter` the stage's counters
    speckle_size: above 0, the speckle filter (binding.Context.remove_speckles_device): right after the end pass of
               the last outer iteration the finished maps of every batch lose their segments of fewer than speckle_size pixels (upstream's
               nSpeckleSize is 100), on the rank that estimated them and before anything else reads them -- the post-filters of that
               iteration, geometric_filter, the fusion, the returned `maps`.  speckle_diff: the relative depth difference below which two
               neighbours are of one segment (None: upstream's 0.01f * 0.7f).  `speckle` in the result: the counters, summed over this
               rank's calls.  0 (default): off
    Returns the fused cloud dict of binding.Context.fuse plus `maps`: {id: (depth, normal, conf) device tensors}."""
    import copy
    import numpy as np
    if geo and (viewspread or hints or priors or plane_priors):
        raise ValueError("densify_scene: geo is not combined with viewspread, hints, priors or plane_priors (the library refuses the term together with each)")
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
    ids = list(order)
    h, w = views[ids[0]]["gray"].shape
    hw = h * w
    for i in ids:
        assert views[i]["gray"].shape == (h, w), "densify_scene: all images must have one size (equal slabs for one all-gather)"
    mine = shard_order(ids, world)[rank]
    n_local = (len(ids) + world - 1) // world
    need_gray = set(mine)
    for img in mine:
        need_gray.update(srcs[img])
    for i, v in views.items():
        if i in need_gray or v.get("bgr") is None:        # without a colour image the gradient map comes from the gray image
            ctx.upload_view(i, v["gray"], v["K"], v["R"], v["C"], bgr=v.get("bgr"))
        else:
            ctx.upload_view(i, None, v["K"], v["R"], v["C"], bgr=v["bgr"])
    for img in mine:
        if masks and img in masks:
            ctx.set_ignore_mask(img, masks[img][0], masks[img][1])
    slabs = torch.zeros(n_local, FLOATS_PER_PIXEL * hw, dtype=torch.float32, device=dev)
    rng = torch.zeros(n_local, 2, dtype=torch.float32, device=dev)      # (d_min, d_max) travel with the maps
    zeroed = False      # the context writes a dict entry's row on its own stream: torch's zero fill of the slabs must have landed first
    previous = []       # (row, image, depth, normal): the entries handed over from a previous level, after the loop, in batches
    for j, img in enumerate(mine):
        if isinstance(init[img], dict) and "previous" in init[img]:
            previous.append((j, img) + tuple(_device_map(m, dev) for m in init[img]["previous"]))
            continue
        if isinstance(init[img], dict):
            e = init[img]
            if not zeroed:
                _device_sync(dev)
                zeroed = True
            base = slabs[j].data_ptr()
            if "splat" in e:
                dmin, dmax = ctx.splat_init_device(img, e["splat"], base, base + 4 * hw)
            else:
                dmin, dmax = ctx.triangulate_init_device(img, e["points"], base, base + 4 * hw, avg_depth=e.get("avg_depth", 0.0),
                                                         add_corners=e.get("add_corners", True))
        else:
            d0, n0, dmin, dmax = init[img]
            slabs[j, :hw] = torch.from_numpy(np.ascontiguousarray(d0, np.float32)).reshape(-1).to(dev)
            slabs[j, hw:4 * hw] = torch.from_numpy(np.ascontiguousarray(n0, np.float32)).reshape(-1).to(dev)
        rng[j, 0], rng[j, 1] = float(dmin), float(dmax)
    if previous:        # the previous level's maps, of any size, straight into the slab rows: one pass per batch, the ranges come from it
        done = _handoff(ctx, dev, "init", [(img, d, n, slabs[j].data_ptr(), slabs[j].data_ptr() + 4 * hw, 0.0, 0.0) for j, img, d, n in previous], w, h)
        for (j, img, _, _), r in zip(previous, done):
            if r["status"] != 0:
                raise ValueError("densify_scene: the previous level's depth map of image %d holds no valid depth" % img)
            rng[j, 0], rng[j, 1] = r["d_min"], r["d_max"]
    hint_at = {}        # image -> (hint depth, hint normal) addresses: the `restore` variant's extra hypothesis of the last sweep
    hintbuf = None
    if hints:
        rows = [(j, img) for j, img in enumerate(mine) if img in hints]
        hintbuf = torch.empty(max(len(rows), 1), 4 * hw, dtype=torch.float32, device=dev)      # 16 B per pixel of the rank's hinted images
        host_rng = rng.cpu()
        jobs = []
        for k, (j, img) in enumerate(rows):
            d, n = (_device_map(m, dev) for m in hints[img])
            hint_at[img] = (hintbuf[k].data_ptr(), hintbuf[k].data_ptr() + 4 * hw)
            jobs.append((img, d, n) + hint_at[img] + (float(host_rng[j, 0]), float(host_rng[j, 1])))
        for (j, img), r in zip(rows, _handoff(ctx, dev, "hint", jobs, w, h)):
            rng[j, 0], rng[j, 1] = r["d_min"], r["d_max"]       # the range takes the enlarged map in
    allr = allgather_maps(rng, group)
    gathered = torch.empty(world * n_local, FLOATS_PER_PIXEL * hw, dtype=torch.float32, device=dev) if world > 1 else None

    def item_of(img, base):
        r = allr[slab_index(ids.index(img), world, n_local)]
        it = dict(ref_id=img, src_ids=list(srcs[img]), d_min=float(r[0]), d_max=float(r[1]), d_depth=base, d_normal=base + 4 * hw,
                  d_conf=base + 16 * hw, seed_offset=img)
        if img in hint_at:
            it["d_hint_depth"], it["d_hint_normal"] = hint_at[img]
        return it

    def my_items(store, row_of):
        by_class = {}
        for img in mine:        # the items of a batch share a lane-layout class (up to 8 views, or 9..16)
            by_class.setdefault(8 if len(srcs[img]) <= 8 else 16, []).append(item_of(img, store[row_of(img)].data_ptr()))
        return by_class

    def register_spread(allm):      # every image offers the maps in allm to the estimates it is a source view of
        for k, img in enumerate(ids):
            base = allm[slab_index(k, world, n_local)].data_ptr()
            ctx.set_spread_maps_device(img, base, base + 4 * hw, base + 16 * hw)

    priors = dict(priors) if priors else {}
    plane_priors = dict(plane_priors) if plane_priors else {}
    both = sorted(set(priors) & set(plane_priors))
    if both:
        raise ValueError("densify_scene: image %d is listed in priors and in plane_priors" % both[0])
    if (priors or plane_priors) and (viewspread or hints):
        raise ValueError("densify_scene: depth priors are not combined with viewspread or hints (the library refuses an active prior together with either)")
    prior_it = int(n_external_iters) - 2 if (priors or plane_priors) else -1      # the outer iteration that registers the priors and runs the two extra sweeps
    if priors or plane_priors:
        ctx.set_prior_params(**(prior_params or {}))
    prior_keep = []
    plane_maps, plane_counts = {}, {}
    ppp = plane_prior_params
    if plane_priors and ppp is None:
        from .binding import default_plane_prior_params
        ppp = default_plane_prior_params()
    if prior_it >= 0:
        for img in mine:
            if img in plane_priors:
                ctx.set_prior_region(img, plane_priors[img], ppp.region_label)

    def extra_sweeps(items):        # after the ordinary estimate of `items` on outer iteration prior_it: their priors, then sweeps N and N + 1
        extra = [x for x in items if x["ref_id"] in priors or x["ref_id"] in plane_priors]
        for x in extra:
            if x["ref_id"] in plane_priors:     # generated from the live maps of the image (ordered behind its estimate on the context's stream)
                m = torch.empty(h, w, dtype=torch.float32, device=dev)
                _device_sync(dev)
                planes, _ = ctx.generate_plane_prior_device(x["ref_id"], x["d_depth"], x["d_normal"], x["d_conf"], m.data_ptr(), None, ppp)
                plane_maps[x["ref_id"]] = m; plane_counts[x["ref_id"]] = len(planes)
            else:
                m = priors[x["ref_id"]]
            if torch.is_tensor(m):
                assert m.is_cuda and m.dtype == torch.float32 and m.is_contiguous() and tuple(m.shape) == (h, w)
                prior_keep.append(m)
                ctx.set_depth_prior_device(x["ref_id"], m.data_ptr())
            else:
                ctx.set_depth_prior(x["ref_id"], m)
        if extra:
            ctx.estimate_sweeps_batch_device(extra, p, p.n_estimation_iters, 2)

    speckle_size = int(speckle_size)
    if speckle_size < 0:
        raise ValueError("densify_scene: speckle_size is a number of pixels >= 0, not %d" % speckle_size)
    speckle_stats = {}

    def remove_speckles(items):     # the finished maps of `items`, behind their estimate on the context's stream
        st = ctx.remove_speckles_device([dict(width=w, height=h, d_depth=x["d_depth"], d_normal=x["d_normal"], d_conf=x["d_conf"]) for x in items],
                                        speckle_diff, speckle_size)
        for k, v in st.items():
            speckle_stats[k] = max(speckle_stats.get(k, 0), v) if k in ("largest", "device_bytes") else speckle_stats.get(k, 0) + v

    last_it = int(n_external_iters) - 1
    geo_kw = None
    if geo:
        geo_kw = dict(geo) if isinstance(geo, dict) else {}
        geo_kw.pop("on", None)
        ctx.set_geo_params(on=True, **geo_kw)
    offer = bool(viewspread) or geo_kw is not None      # the source views offer their previous maps: to view spread, or to the term
    if viewspread:
        ctx.set_viewspread(True)
    snapshot = torch.empty_like(slabs) if offer and world == 1 and not interleave and n_external_iters > 1 else None

    def register(allm):
        for k, img in enumerate(ids):
            row = slab_index(k, world, n_local)
            base = allm[row].data_ptr()
            ctx.set_depthmap_device(img, base, base + 4 * hw, base + 16 * hw, float(allr[row, 0]), float(allr[row, 1]))
            ctx.set_neighbors(img, [n for n in neighbors[img] if n in views][:31])

    p = copy.copy(params)
    p.n_external_iters = int(n_external_iters)
    _device_sync(dev)
    for it in range(int(n_external_iters)):
        p.it_external = it
        filt = postfilter and it in (1, 2)
        spread = offer and it >= 1
        if (filt or spread) and interleave:
            # the reference's order: estimate(k) -> post-filter(k) -> estimate(k + 1), image ids ascending.  The gathered buffer is the
            # state of the whole scene on every rank; an image is estimated in place by its owner and broadcast before its filter runs
            allm = allgather_maps(slabs, group, out=gathered)
            _device_sync(dev)
            register(allm)
            if spread:
                register_spread(allm)   # the live maps: the reference image is never its own source view, so no estimate reads what it writes
            for img in sorted(ids):
                k = ids.index(img)
                row = slab_index(k, world, n_local)
                owner = k % world
                if owner == rank:
                    ctx.estimate_batch_device([item_of(img, allm[row].data_ptr())], p)
                    if it == prior_it:
                        extra_sweeps([item_of(img, allm[row].data_ptr())])
                    if speckle_size > 0 and it == last_it:
                        remove_speckles([item_of(img, allm[row].data_ptr())])
                    ctx.synchronize()
                if world > 1:
                    if allm.is_cuda and dist.get_backend(group) == "gloo":      # one-GPU rehearsal: gloo moves host tensors
                        host = allm[row].cpu()
                        dist.broadcast(host, src=dist.get_global_rank(group, owner) if group is not None else owner, group=group)
                        allm[row].copy_(host)
                    else:
                        dist.broadcast(allm[row], src=dist.get_global_rank(group, owner) if group is not None else owner, group=group)
                    _device_sync(dev)
                if filt:
                    ctx.postfilter(img, ids, **(pf_kw or {}))
            ctx.synchronize()
            if world > 1:
                for j, img in enumerate(mine):
                    slabs[j].copy_(allm[slab_index(ids.index(img), world, n_local)])
                _device_sync(dev)
            continue
        if spread:      # the maps as the previous outer iteration left them, of every image, apart from the ones being written
            if world > 1:
                snap = allgather_maps(slabs, group, out=gathered)
            else:
                snapshot.copy_(slabs)
                snap = snapshot
            _device_sync(dev)
            register_spread(snap)
        for cls, items in sorted(my_items(slabs, lambda img: mine.index(img)).items()):     # NO collective on the estimation path (view spread: the one above)
            for b0 in range(0, len(items), batch):
                ctx.estimate_batch_device(items[b0:b0 + batch], p)
                if it == prior_it:
                    extra_sweeps(items[b0:b0 + batch])
                if speckle_size > 0 and it == last_it:
                    remove_speckles(items[b0:b0 + batch])
        ctx.synchronize()
        if filt:
            allm = allgather_maps(slabs, group, out=gathered)  # every rank: every image's current maps
            _device_sync(dev)
            register(allm)
            ctx.postfilter_sequence(sorted(ids), ids, **(pf_kw or {}))   # image after image (batch schedule, D6)
            ctx.synchronize()
            if world > 1:                                      # my images' filtered maps: out of the gathered buffer, back into my slabs
                for j, img in enumerate(mine):
                    slabs[j].copy_(allm[slab_index(ids.index(img), world, n_local)])
                _device_sync(dev)                              # the next estimate reads the slabs on the context's stream
    allm = allgather_maps(slabs, group, out=gathered)          # the exchange before fusion: 20 B/px, rank-major equal slabs
    _device_sync(dev)
    register(allm)
    maps = {img: unpack_maps(allm[slab_index(k, world, n_local)], h, w) for k, img in enumerate(ids)}
    filter_stats = None
    if geometric_filter is not None:
        if geometric_filter not in ("adjust", "strict"):
            raise ValueError("densify_scene: geometric_filter is None, 'adjust' or 'strict', not %r" % (geometric_filter,))
        filter_stats = ctx.filter_sequence(ids, adjust=geometric_filter == "adjust", **(gf_kw or {}))   # in place, synchronised on return

    def finish(cloud):
        cloud["maps"] = maps
        if filter_stats is not None:
            cloud["filter"] = filter_stats
        if speckle_size > 0:
            cloud["speckle"] = speckle_stats
        if viewspread:
            ctx.set_viewspread(False)
        if geo_kw is not None:
            ctx.set_geo_params(on=False)
        if offer:
            for img in ids:
                ctx.set_spread_maps_device(img, None, None, None)
        if priors or plane_priors:
            cloud["priors_used"] = prior_it >= 0
            for img in mine:
                if (img in priors or img in plane_priors) and prior_it >= 0:
                    ctx.set_depth_prior(img, None)
                if img in plane_priors and prior_it >= 0:
                    ctx.set_prior_region(img, None)
        if plane_priors:
            cloud["plane_prior_maps"] = plane_maps; cloud["plane_prior_planes"] = plane_counts
        cloud["_keep"] = (allm, allr, slabs, hintbuf, prior_keep)      # the registered device maps must outlive the context's use of them
        return cloud

    if not fuse:        # an intermediate level: the maps are the result
        return finish(dict(ranges={img: (float(allr[slab_index(k, world, n_local), 0]), float(allr[slab_index(k, world, n_local), 1])) for k, img in enumerate(ids)}))
    # the cloud's buffers: as given, or counted -- a counting fusion first (no buffers), then the real one with exactly what it needs,
    # instead of half a point per pixel of the scene on every rank (66 GB of device and of host memory each at BASELINE configs[3]); a
    # fusion repeated on the maps a fusion has left makes the same decisions, so the cloud is the single pass's
    if capacity is not None:
        cap = capacity
    elif hasattr(ctx, "fuse_count"):
        kw = {k: v for k, v in (fuse_kw or {}).items() if k not in ("with_normals", "with_colors")}
        counted = ctx.fuse_count(ids, **kw)
        cap = counted[0] + 1
    else:
        cap = hw * len(ids) // 2
    cloud = ctx.fuse(ids, cap, **(fuse_kw or {}))          # replicated on every rank: identical clouds
    if capacity is None and hasattr(ctx, "fuse_count"):
        cloud["n_depths"] = counted[1]                     # the depths the fusion visited before it invalidated any (SceneDensify.cpp:3461 logs that number)
    return finish(cloud)


def densify_pyramid(ctx, stages, srcs, neighbors, order, init, **kw):
    """The fork's coarse-to-fine schedule (run.sh: levels 3 -> 2 -> 2 -> 1 -> 1) as a chain of densify_scene calls whose maps never leave
    the device: a level starts from the previous level's maps, or takes them as the extra hypothesis of its last sweep.

    stages: one dict per level, in order: views (that level's images and cameras, as densify_scene takes them), params, mode, plus any
            densify_scene keyword (n_external_iters, postfilter, ...; they override **kw).  mode is
              "triangulate"  the level starts from `init` (a stage may bring its own under the key init); stage 0 always does.  An init of
                             dict(points=...) entries is rasterised at the level's own size, so one `init` serves every level
              "handoff"      it starts from the previous stage's maps (--n-initTriangulate 0): init = dict(previous=...) for every image
              "restore"      it starts from `init` like "triangulate" and takes the previous stage's maps as hints (the `restore` binary)
    Only the last stage fuses.  Every rank holds all maps of a stage after its all-gather, so the chain runs unchanged with several ranks.
    Returns the last stage's result (densify_scene's)"""
    if not stages:
        raise ValueError("densify_pyramid: no stages")
    prev = None
    for k, stage in enumerate(stages):
        st = dict(stage)
        views, params, mode = st.pop("views"), st.pop("params"), st.pop("mode")
        if mode not in ("triangulate", "handoff", "restore"):
            raise ValueError("densify_pyramid: stage %d: mode is 'triangulate', 'handoff' or 'restore', not %r" % (k, mode))
        if k == 0 and mode != "triangulate":
            raise ValueError("densify_pyramid: stage 0 has no previous maps: its mode is 'triangulate'")
        opts = dict(kw)
        stage_init = st.pop("init", init)
        opts.update(st)
        opts["fuse"] = k == len(stages) - 1
        if mode == "handoff":
            stage_init = {i: dict(previous=prev["maps"][i][:2]) for i in order}
        elif mode == "restore":
            opts["hints"] = {i: prev["maps"][i][:2] for i in order}
        res = densify_scene(ctx, views, srcs, neighbors, order, stage_init, params, **opts)
        prev = res          # the previous stage's buffers live until the next stage has taken them over
    return prev

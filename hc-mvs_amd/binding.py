"""ctypes binding of libhcmvs_hip.so (the C-ABI of include/hcmvs_hip.h).

Mirrors the reference's per-image interface (SceneDensify.h:63-70 DepthMapsData::EstimateDepthMap /
FilterDepthMap / FuseDepthMaps) for tests and bench.py.  There is no CPU fallback: loading fails loudly
when the library is missing, and creating a context fails when no gfx950 device is usable.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhcmvs_hip.so")

OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_TIMEOUT, ERR_CAPACITY, ERR_INTERNAL = range(7)


class Params(C.Structure):
    _fields_ = [("adapthalfwin", C.c_int32), ("n_estimation_iters", C.c_int32), ("it_external", C.c_int32),
                ("n_external_iters", C.c_int32), ("propagate_halfwin", C.c_int32), ("propagate_step", C.c_int32),
                ("n_random_iters", C.c_int32), ("ncc_threshold_keep", C.c_float), ("random_depth_ratio", C.c_float),
                ("random_angle1_deg", C.c_float), ("random_angle2_deg", C.c_float),
                ("random_smooth_depth", C.c_float), ("random_smooth_normal_deg", C.c_float),
                ("random_smooth_bonus", C.c_float), ("photometric_flow", C.c_float), ("seed", C.c_uint32),
                ("median_blur", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("evals", C.c_uint64), ("evals_issued", C.c_uint64), ("tap_evals", C.c_uint64), ("ms_score", C.c_float), ("ms_sweeps", C.c_float),
                ("ms_sweep_avg", C.c_float), ("ms_end", C.c_float), ("ms_total", C.c_float),
                ("n_sweeps", C.c_int32), ("n_sweep_launches", C.c_int32)]


class BatchItem(C.Structure):
    _fields_ = [("ref_id", C.c_uint32), ("src_ids", C.POINTER(C.c_uint32)), ("n_src", C.c_int32),
                ("seed_offset", C.c_uint32), ("d_min", C.c_float), ("d_max", C.c_float), ("d_depth", C.c_void_p),
                ("d_normal", C.c_void_p), ("d_conf", C.c_void_p), ("d_hint_depth", C.c_void_p), ("d_hint_normal", C.c_void_p)]


class Cloud(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("xyz", C.POINTER(C.c_float)), ("normal", C.POINTER(C.c_float)), ("bgr", C.POINTER(C.c_uint8)),
                ("n_views", C.POINTER(C.c_uint32)), ("views_capacity", C.c_uint64), ("view_ids", C.POINTER(C.c_uint32)),
                ("view_weights", C.POINTER(C.c_float)), ("n_points", C.c_uint64), ("n_depths", C.c_uint64), ("n_view_entries", C.c_uint64)]


class VisibilityStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("skipped_pairs", C.c_uint64), ("fallback_pairs", C.c_uint64), ("candidates", C.c_uint64),
                ("hits", C.c_uint64), ("device_bytes", C.c_uint64), ("ms_device", C.c_float)]


class MeshSampleStats(C.Structure):
    _fields_ = [("n_faces", C.c_uint64), ("n_zero_area_faces", C.c_uint64), ("n_points", C.c_uint64), ("area", C.c_double), ("density", C.c_double),
                ("ms_device", C.c_float), ("device_bytes", C.c_uint64)]


class ViewSelectParams(C.Structure):
    _fields_ = [("n_min_views", C.c_int32), ("n_min_point_views", C.c_int32), ("n_max_views", C.c_int32), ("number_views", C.c_int32),
                ("optim_angle_deg", C.c_float), ("min_angle_deg", C.c_float), ("max_angle_deg", C.c_float), ("min_area", C.c_float),
                ("min_scale", C.c_float), ("max_scale", C.c_float), ("min_score_ratio", C.c_float), ("min_score", C.c_float)]


class ViewSelection(C.Structure):
    _U32, _F32 = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    _fields_ = [("status", C.POINTER(C.c_int32)), ("n_seen", _U32), ("avg_depth", _F32), ("n_candidates", _U32), ("n_neighbors", _U32), ("n_srcs", _U32),
                ("nb_id", _U32), ("nb_points", _U32), ("nb_scale", _F32), ("nb_angle", _F32), ("nb_area", _F32), ("nb_score", _F32), ("src_scale", _F32),
                ("points_first", C.POINTER(C.c_uint64)), ("point_ids", _U32)]


class ViewSelectStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("skipped", C.c_uint64), ("chunks", C.c_uint64), ("device_bytes", C.c_uint64), ("ms_device", C.c_float)]


class InitStats(C.Structure):
    _fields_ = [("n_used", C.c_uint64), ("n_faces", C.c_uint64), ("n_tile_entries", C.c_uint64), ("covered_pixels", C.c_uint64),
                ("cover_hits", C.c_uint64), ("ms_host", C.c_float), ("ms_device", C.c_float), ("device_bytes", C.c_uint64)]


class HandoffItem(C.Structure):
    _fields_ = [("src_depth", C.c_void_p), ("src_normal", C.c_void_p), ("src_w", C.c_int32), ("src_h", C.c_int32),
                ("dst_depth", C.c_void_p), ("dst_normal", C.c_void_p), ("dst_w", C.c_int32), ("dst_h", C.c_int32),
                ("d_min", C.c_float), ("d_max", C.c_float), ("status", C.c_int32),
                ("n_valid", C.c_uint64), ("n_clamped", C.c_uint64), ("n_rescaled", C.c_uint64)]


class HandoffStats(C.Structure):
    _fields_ = [("n_pixels", C.c_uint64), ("n_valid", C.c_uint64), ("n_clamped", C.c_uint64), ("n_rescaled", C.c_uint64),
                ("n_items", C.c_int32), ("n_empty", C.c_int32), ("ms_device", C.c_float)]


class SpeckleItem(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("d_depth", C.c_void_p), ("d_normal", C.c_void_p), ("d_conf", C.c_void_p),
                ("d_labels", C.c_void_p)]


class SpeckleStats(C.Structure):
    _fields_ = [("n_valid", C.c_uint64), ("n_removed", C.c_uint64), ("n_segments", C.c_uint64), ("n_small", C.c_uint64),
                ("largest", C.c_uint32), ("ms_device", C.c_float), ("device_bytes", C.c_uint64)]


SPECKLE_DIFF = float(np.float32(0.01) * np.float32(0.7))   # upstream's threshold: 0.01f * 0.7f, the product taken in float

HANDOFF_INIT, HANDOFF_HINT = 0, 1           # hcmvs_handoff_maps*: mode
HANDOFF_OK, HANDOFF_EMPTY = 0, 1            # ... an item's status
_HANDOFF_MODES = {"init": HANDOFF_INIT, "hint": HANDOFF_HINT}


class SpreadStats(C.Structure):
    _fields_ = [("slots_scored", C.c_uint64), ("slots_accepted", C.c_uint64), ("slots_dropped", C.c_uint64), ("candidates_outside", C.c_uint64)]


class PriorParams(C.Structure):
    _fields_ = [("para_prior", C.c_float), ("sigma_prior", C.c_float), ("photo2geo", C.c_int32)]


class PriorStats(C.Structure):
    _fields_ = [("evals_prior", C.c_uint64), ("pixels_prior", C.c_uint64)]


class GeoParams(C.Structure):
    _fields_ = [("on", C.c_int32), ("para_tapa", C.c_float), ("para_tapa2", C.c_float), ("txthreshold", C.c_float), ("txthreshold2", C.c_float),
                ("photo2geo", C.c_int32), ("max_px", C.c_float)]


class GeoStats(C.Structure):
    _fields_ = [("evals_geo", C.c_uint64), ("pixels_geo", C.c_uint64)]


class PlanePriorParams(C.Structure):
    _fields_ = [("region_label", C.c_int32), ("conf_max", C.c_float), ("planarity_min", C.c_float), ("n_neighbors", C.c_int32), ("probability", C.c_float),
                ("min_points_div", C.c_float), ("epsilon_mul", C.c_float), ("normal_threshold", C.c_float), ("max_rounds", C.c_int32), ("seed", C.c_uint64),
                ("cluster_mul", C.c_float)]
    # int32_t refit_iters, which the C struct appends, lies in the four bytes of tail padding behind cluster_mul (the size of the struct is
    # what it was).  The field list above stays the one callers and tests of the layout were written against; the new member is a
    # property over those four bytes.  A fresh instance is all zeros: no refit
    REFIT_ITERS_OFFSET = 52

    @property
    def refit_iters(self):
        return C.c_int32.from_buffer(self, self.REFIT_ITERS_OFFSET).value

    @refit_iters.setter
    def refit_iters(self, v):
        C.c_int32.from_buffer(self, self.REFIT_ITERS_OFFSET).value = v


assert PlanePriorParams.cluster_mul.offset + 4 == PlanePriorParams.REFIT_ITERS_OFFSET and C.sizeof(PlanePriorParams) == PlanePriorParams.REFIT_ITERS_OFFSET + 4


class PlanePriorRefitStats(C.Structure):
    _fields_ = [("refit_rounds", C.c_int32), ("refit_steps", C.c_int32)]


class PriorPlane(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("n_inliers", C.c_uint32), ("centre", C.c_double * 3), ("quad", C.c_double * 8), ("box_fallback", C.c_int32),
                ("reserved", C.c_int32)]


class PlanePriorStats(C.Structure):
    _fields_ = [("region_pixels", C.c_uint64), ("samples", C.c_uint64), ("planar_samples", C.c_uint64), ("fitting_samples", C.c_uint64),
                ("avg_spacing_all", C.c_double), ("avg_spacing", C.c_double), ("eps", C.c_float), ("min_points", C.c_int32), ("rounds", C.c_int32),
                ("planes", C.c_int32), ("candidates_valid", C.c_uint64), ("prior_pixels", C.c_uint64), ("ms_device", C.c_float), ("ms_gather", C.c_float), ("ms_search", C.c_float),
                ("ms_rounds", C.c_float), ("ms_render", C.c_float), ("device_bytes", C.c_uint64), ("cluster_eps", C.c_float), ("cluster_rejects", C.c_int32),
                ("cluster_left", C.c_uint64)]


MAX_PRIOR_PLANES = 64


class FilterStats(C.Structure):
    _fields_ = [("n_processed", C.c_uint64), ("n_discarded", C.c_uint64), ("n_filtered", C.c_uint32), ("n_skipped", C.c_uint32),
                ("batch", C.c_uint32), ("ms_device", C.c_float), ("device_bytes", C.c_uint64), ("image_processed", C.POINTER(C.c_uint64)),
                ("image_discarded", C.POINTER(C.c_uint64))]


class HcmvsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hcmvs error %d: %s" % (code, msg))
        self.code = code


_lib = None

# every symbol include/hcmvs_hip.h declares
SYMBOLS = ["hcmvs_default_params", "hcmvs_create", "hcmvs_destroy", "hcmvs_last_error", "hcmvs_set_stream",
           "hcmvs_synchronize", "hcmvs_upload_view", "hcmvs_set_view_device", "hcmvs_release_view", "hcmvs_rescale_view", "hcmvs_get_view_info",
           "hcmvs_get_view_gray",
           "hcmvs_get_gradient_map", "hcmvs_estimate", "hcmvs_estimate_device", "hcmvs_estimate_batch_device", "hcmvs_get_stats",
           "hcmvs_splat_init", "hcmvs_splat_points", "hcmvs_triangulate_init", "hcmvs_triangulate_points",
           "hcmvs_triangulate_init_device", "hcmvs_splat_init_device", "hcmvs_get_init_stats", "hcmvs_set_depthmap", "hcmvs_set_depthmap_device", "hcmvs_get_depthmap",
           "hcmvs_set_neighbors", "hcmvs_filter", "hcmvs_filter_sequence", "hcmvs_set_fuse_order", "hcmvs_fuse", "hcmvs_fuse_cloud", "hcmvs_estimate_point_colors",
           "hcmvs_estimate_point_normals", "hcmvs_point_cloud_filter", "hcmvs_sample_mesh", "hcmvs_default_view_select_params", "hcmvs_select_views",
           "hcmvs_postfilter", "hcmvs_postfilter_sequence", "hcmvs_resize_area_up",
           "hcmvs_handoff_maps", "hcmvs_handoff_maps_device", "hcmvs_get_handoff_stats",
           "hcmvs_remove_speckles", "hcmvs_remove_speckles_batch_device",
           "hcmvs_set_ignore_mask", "hcmvs_set_ignore_mask_device", "hcmvs_get_ignore_mask",
           "hcmvs_set_viewspread", "hcmvs_set_spread_maps_device", "hcmvs_get_spread_stats",
           "hcmvs_default_geo_params", "hcmvs_set_geo_params", "hcmvs_get_geo_stats",
           "hcmvs_default_prior_params", "hcmvs_set_prior_params", "hcmvs_set_depth_prior", "hcmvs_set_depth_prior_device",
           "hcmvs_estimate_sweeps_batch_device", "hcmvs_get_prior_stats",
           "hcmvs_default_plane_prior_params", "hcmvs_set_prior_region", "hcmvs_get_prior_region", "hcmvs_generate_plane_prior_device",
           "hcmvs_get_plane_prior_trace", "hcmvs_get_plane_prior_cluster_trace", "hcmvs_get_plane_prior_refit_trace",
           "hcmvs_get_plane_prior_refit_stats"]


def triangulate_points(w, h, K, R, Cc, points_xyz, avg_depth=0.0, add_corners=True):
    """hcmvs_triangulate_points: the triangulation initialisation without a context (pure host code)"""
    pts = np.ascontiguousarray(points_xyz, np.float32)
    depth = np.zeros((h, w), np.float32); normal = np.zeros((h, w, 3), np.float32)
    dmin = C.c_float(); dmax = C.c_float()
    Ka, Kp = _d(K); Ra, Rp = _d(R); Ca, Cp = _d(Cc)
    rc = lib().hcmvs_triangulate_points(w, h, Kp, Rp, Cp, _f(pts), len(pts), C.c_float(avg_depth), int(add_corners), _f(depth),
                                        _f(normal), C.byref(dmin), C.byref(dmax))
    if rc != 0:
        raise HcmvsError(rc, "triangulate_points failed")
    return depth, normal, dmin.value, dmax.value


def resize_area_up(src, dst_w, dst_h):
    """hcmvs_resize_area_up: cv::resize INTER_AREA enlarging an f32 map (h, w) or (h, w, channels); pure host code"""
    s = np.ascontiguousarray(src, np.float32)
    ch = 1 if s.ndim == 2 else s.shape[2]
    out = np.empty((dst_h, dst_w) if s.ndim == 2 else (dst_h, dst_w, ch), np.float32)
    rc = lib().hcmvs_resize_area_up(_f(s), s.shape[1], s.shape[0], ch, _f(out), dst_w, dst_h)
    if rc != 0:
        raise HcmvsError(rc, "resize_area_up failed")
    return out


def _handoff_items(items):
    """list of dicts (src_depth, src_normal, dst_depth, dst_normal: addresses; src_w, src_h, dst_w, dst_h[, d_min, d_max]) -> HandoffItem array"""
    arr = (HandoffItem * max(len(items), 1))()
    for a, it in zip(arr, items):
        a.src_depth = it["src_depth"] or None; a.src_normal = it["src_normal"] or None
        a.dst_depth = it["dst_depth"] or None; a.dst_normal = it["dst_normal"] or None
        a.src_w, a.src_h, a.dst_w, a.dst_h = int(it["src_w"]), int(it["src_h"]), int(it["dst_w"]), int(it["dst_h"])
        a.d_min = it.get("d_min", 0.0); a.d_max = it.get("d_max", 0.0)
        a.status = -1
    return arr


def _handoff_results(arr, n):
    return [dict(d_min=arr[i].d_min, d_max=arr[i].d_max, status=arr[i].status, n_valid=arr[i].n_valid, n_clamped=arr[i].n_clamped,
                 n_rescaled=arr[i].n_rescaled) for i in range(n)]


def _handoff_mode(mode):
    return _HANDOFF_MODES[mode] if isinstance(mode, str) else int(mode)


def handoff_maps_raw(items, mode):
    """hcmvs_handoff_maps on addresses of HOST buffers (items as Context.handoff_maps_device takes them).  Returns (status of the call,
    per-item results); nothing raises, so a refusal can be looked at"""
    arr = _handoff_items(items)
    rc = lib().hcmvs_handoff_maps(arr, len(items), _handoff_mode(mode))
    return rc, _handoff_results(arr, len(items))


def handoff_maps(maps, mode):
    """hcmvs_handoff_maps: the hand-off between two pyramid levels on host arrays, no context (pure host code; what the device form is
    pinned to).  maps: list of dicts(depth (h, w), normal (h, w, 3), dst_w, dst_h[, d_min, d_max]) -- the previous level's maps, the size
    wanted, and in mode "hint" the range to widen.  mode "init": the maps a level starts from (copied or cv::resize INTER_CUBIC, cleaned;
    d_min / d_max come out).  mode "hint": the `restore` variant's extra hypothesis (INTER_AREA enlarging; d_min / d_max are widened).
    Returns one dict per entry: depth (dst_h, dst_w), normal (dst_h, dst_w, 3), d_min, d_max, status (HANDOFF_OK, or HANDOFF_EMPTY: no
    valid depth, d_min / d_max as given), n_valid, n_clamped, n_rescaled"""
    keep, items = [], []
    for m in maps:
        d = np.ascontiguousarray(m["depth"], np.float32); n = np.ascontiguousarray(m["normal"], np.float32)
        if d.ndim != 2 or n.shape != d.shape + (3,):
            raise ValueError("handoff_maps: depth (h, w) and normal (h, w, 3) expected")
        dw, dh = int(m["dst_w"]), int(m["dst_h"])
        od = np.empty((max(dh, 0), max(dw, 0)), np.float32); on = np.empty((max(dh, 0), max(dw, 0), 3), np.float32)
        keep.append((d, n, od, on))
        items.append(dict(src_depth=d.ctypes.data, src_normal=n.ctypes.data, src_w=d.shape[1], src_h=d.shape[0], dst_depth=od.ctypes.data,
                          dst_normal=on.ctypes.data, dst_w=dw, dst_h=dh, d_min=m.get("d_min", 0.0), d_max=m.get("d_max", 0.0)))
    rc, res = handoff_maps_raw(items, mode)
    if rc != 0:
        raise HcmvsError(rc, "handoff_maps: refused (null pointer, size, overlap, shrinking hint, NaN range or unknown mode)")
    for r, (_, _, od, on) in zip(res, keep):
        r["depth"] = od; r["normal"] = on
    return res


def _speckle_stats(st):
    return {k: getattr(st, k) for k, _ in SpeckleStats._fields_}


def remove_speckles_raw(w, h, depth, normal, conf, labels, thr, speckle_size):
    """hcmvs_remove_speckles on addresses of HOST buffers (0 / None: not given).  Returns (status of the call, stats dict); nothing raises,
    so a refusal can be looked at"""
    st = SpeckleStats()
    rc = lib().hcmvs_remove_speckles(int(w), int(h), depth or None, normal or None, conf or None, labels or None, C.c_float(thr), int(speckle_size),
                                     C.byref(st))
    return rc, _speckle_stats(st)


def remove_speckles(depth, normal=None, conf=None, thr=None, speckle_size=100, want_labels=True):
    """hcmvs_remove_speckles: the speckle filter on host arrays, no context (pure host code; what the device form is pinned to).  Segments
    of valid depths (4-neighbours joined when similar within thr from both sides) with fewer than speckle_size pixels lose depth, normal
    and conf.  thr None: upstream's 0.01f * 0.7f.  The arrays given are left alone; returns dict(depth, normal, conf (None where not
    given), labels (the canonical label of every pixel before the removal, -1 where not valid; None when not wanted), stats)"""
    d = np.array(depth, np.float32, order="C")
    if d.ndim != 2:
        raise ValueError("remove_speckles: depth (h, w) expected")
    n = None if normal is None else np.array(normal, np.float32, order="C")
    c = None if conf is None else np.array(conf, np.float32, order="C")
    if (n is not None and n.shape != d.shape + (3,)) or (c is not None and c.shape != d.shape):
        raise ValueError("remove_speckles: normal (h, w, 3) and conf (h, w) expected")
    lab = np.empty(d.shape, np.int32) if want_labels else None
    rc, st = remove_speckles_raw(d.shape[1], d.shape[0], d.ctypes.data, None if n is None else n.ctypes.data, None if c is None else c.ctypes.data,
                                 None if lab is None else lab.ctypes.data, SPECKLE_DIFF if thr is None else thr, speckle_size)
    if rc != 0:
        raise HcmvsError(rc, "remove_speckles: refused (size, threshold or overlapping buffers)")
    return dict(depth=d, normal=n, conf=c, labels=lab, stats=st)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libhcmvs_hip.so is not built (run __graft_entry__.build() or make -C hc-mvs_amd/csrc); "
                              "there is no CPU fallback")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7; two HIP runtimes in one process cannot both
        # open the device.  Importing torch first makes the loader resolve our NEEDED libamdhip64.so.7 to the
        # copy that is already mapped, so the process holds exactly one runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp, fp, u8p, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        u32p = C.POINTER(C.c_uint32)
        L.hcmvs_default_params.argtypes = [C.POINTER(Params)]
        L.hcmvs_default_params.restype = None
        L.hcmvs_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.hcmvs_destroy.argtypes = [vp]
        L.hcmvs_destroy.restype = None
        L.hcmvs_last_error.argtypes = [vp]
        L.hcmvs_last_error.restype = C.c_char_p
        L.hcmvs_set_stream.argtypes = [vp, vp]
        L.hcmvs_synchronize.argtypes = [vp]
        L.hcmvs_upload_view.argtypes = [vp, C.c_uint32, C.c_int32, C.c_int32, fp, u8p, dp, dp, dp]
        L.hcmvs_set_view_device.argtypes = [vp, C.c_uint32, C.c_int32, C.c_int32, vp, vp, dp, dp, dp]
        L.hcmvs_release_view.argtypes = [vp, C.c_uint32]
        L.hcmvs_rescale_view.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float]
        L.hcmvs_get_view_info.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp]
        L.hcmvs_get_view_gray.argtypes = [vp, C.c_uint32, fp]
        L.hcmvs_get_gradient_map.argtypes = [vp, C.c_uint32, u8p]
        i32p = C.POINTER(C.c_int32)
        L.hcmvs_set_ignore_mask.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint16), C.c_int32, C.c_int32, i32p, C.c_int32]
        L.hcmvs_set_ignore_mask_device.argtypes = [vp, C.c_uint32, vp, C.c_int32, C.c_int32, i32p, C.c_int32]
        L.hcmvs_get_ignore_mask.argtypes = [vp, C.c_uint32, u8p]
        L.hcmvs_estimate.argtypes = [vp, C.c_uint32, u32p, C.c_int32, C.POINTER(Params), C.c_float, C.c_float, fp, fp, fp]
        L.hcmvs_estimate_device.argtypes = [vp, C.c_uint32, u32p, C.c_int32, C.POINTER(Params), C.c_float, C.c_float,
                                            vp, vp, vp]
        L.hcmvs_estimate_batch_device.argtypes = [vp, C.POINTER(BatchItem), C.c_int32, C.POINTER(Params)]
        L.hcmvs_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.hcmvs_splat_init.argtypes = [vp, C.c_uint32, fp, C.c_int32, fp, fp, fp, fp]
        L.hcmvs_splat_points.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, fp, C.c_int32, fp, fp, fp, fp]
        L.hcmvs_triangulate_init.argtypes = [vp, C.c_uint32, fp, C.c_int32, C.c_float, C.c_int32, fp, fp, fp, fp]
        dp = C.POINTER(C.c_double)
        L.hcmvs_triangulate_points.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, fp, C.c_int32, C.c_float, C.c_int32, fp, fp, fp, fp]
        L.hcmvs_triangulate_init_device.argtypes = [vp, C.c_uint32, fp, C.c_int32, C.c_float, C.c_int32, vp, vp, fp, fp]
        L.hcmvs_splat_init_device.argtypes = [vp, C.c_uint32, fp, C.c_int32, vp, vp, fp, fp]
        L.hcmvs_get_init_stats.argtypes = [vp, C.POINTER(InitStats)]
        u64p = C.POINTER(C.c_uint64)
        L.hcmvs_set_depthmap.argtypes = [vp, C.c_uint32, fp, fp, fp, C.c_float, C.c_float]
        L.hcmvs_set_depthmap_device.argtypes = [vp, C.c_uint32, vp, vp, vp, C.c_float, C.c_float]
        L.hcmvs_get_depthmap.argtypes = [vp, C.c_uint32, fp, fp, fp]
        L.hcmvs_set_neighbors.argtypes = [vp, C.c_uint32, u32p, C.c_int32]
        L.hcmvs_set_fuse_order.argtypes = [vp, C.c_int32]
        L.hcmvs_filter.argtypes = [vp, C.c_uint32, u32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, fp, fp,
                                   u64p, u64p]
        L.hcmvs_filter_sequence.argtypes = [vp, u32p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.POINTER(FilterStats)]
        L.hcmvs_fuse.argtypes = [vp, u32p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint64,
                                 fp, fp, u8p, u32p, u64p, u64p]
        L.hcmvs_fuse_cloud.argtypes = [vp, u32p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Cloud)]
        L.hcmvs_postfilter.argtypes = [vp, C.c_uint32, u32p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, u64p]
        L.hcmvs_postfilter_sequence.argtypes = [vp, u32p, C.c_int32, u32p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, u64p]
        L.hcmvs_estimate_point_colors.argtypes = [vp, C.c_uint64, fp, u32p, u32p, u8p]
        L.hcmvs_estimate_point_normals.argtypes = [vp, C.c_uint64, fp, u32p, u32p, C.c_int32, fp]
        L.hcmvs_point_cloud_filter.argtypes = [vp, C.c_uint64, fp, u32p, u32p, C.c_uint32, C.POINTER(C.c_int32), dp, dp, dp, C.c_int32,
                                               C.POINTER(C.c_int32), u32p, u64p, C.POINTER(VisibilityStats)]
        L.hcmvs_sample_mesh.argtypes = [vp, C.c_uint32, fp, C.c_uint32, u32p, fp, u8p, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_uint64, fp, u32p, u8p,
                                        u64p, C.POINTER(MeshSampleStats)]
        L.hcmvs_default_view_select_params.argtypes = [C.POINTER(ViewSelectParams)]
        L.hcmvs_default_view_select_params.restype = None
        L.hcmvs_select_views.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32), dp, dp, dp, C.c_uint64, fp, u32p, u32p, C.POINTER(ViewSelectParams),
                                         C.POINTER(ViewSelection), C.POINTER(ViewSelectStats)]
        L.hcmvs_resize_area_up.argtypes = [fp, C.c_int32, C.c_int32, C.c_int32, fp, C.c_int32, C.c_int32]
        L.hcmvs_handoff_maps.argtypes = [C.POINTER(HandoffItem), C.c_int32, C.c_int32]
        L.hcmvs_handoff_maps_device.argtypes = [vp, C.POINTER(HandoffItem), C.c_int32, C.c_int32]
        L.hcmvs_get_handoff_stats.argtypes = [vp, C.POINTER(HandoffStats)]
        L.hcmvs_remove_speckles.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, vp, C.c_float, C.c_uint32, C.POINTER(SpeckleStats)]
        L.hcmvs_remove_speckles_batch_device.argtypes = [vp, C.POINTER(SpeckleItem), C.c_int32, C.c_float, C.c_uint32, C.POINTER(SpeckleStats)]
        L.hcmvs_set_viewspread.argtypes = [vp, C.c_int32]
        L.hcmvs_set_spread_maps_device.argtypes = [vp, C.c_uint32, vp, vp, vp]
        L.hcmvs_get_spread_stats.argtypes = [vp, C.POINTER(SpreadStats)]
        L.hcmvs_default_geo_params.argtypes = [C.POINTER(GeoParams)]
        L.hcmvs_default_geo_params.restype = None
        L.hcmvs_set_geo_params.argtypes = [vp, C.POINTER(GeoParams)]
        L.hcmvs_get_geo_stats.argtypes = [vp, C.POINTER(GeoStats)]
        L.hcmvs_default_prior_params.argtypes = [C.POINTER(PriorParams)]
        L.hcmvs_default_prior_params.restype = None
        L.hcmvs_set_prior_params.argtypes = [vp, C.POINTER(PriorParams)]
        L.hcmvs_set_depth_prior.argtypes = [vp, C.c_uint32, fp]
        L.hcmvs_set_depth_prior_device.argtypes = [vp, C.c_uint32, vp]
        L.hcmvs_estimate_sweeps_batch_device.argtypes = [vp, C.POINTER(BatchItem), C.c_int32, C.POINTER(Params), C.c_int32, C.c_int32]
        L.hcmvs_get_prior_stats.argtypes = [vp, C.POINTER(PriorStats)]
        L.hcmvs_default_plane_prior_params.argtypes = [C.POINTER(PlanePriorParams)]
        L.hcmvs_default_plane_prior_params.restype = None
        L.hcmvs_set_prior_region.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint16), C.c_int32, C.c_int32, C.c_int32]
        L.hcmvs_get_prior_region.argtypes = [vp, C.c_uint32, u8p]
        L.hcmvs_generate_plane_prior_device.argtypes = [vp, C.c_uint32, vp, vp, vp, C.POINTER(PlanePriorParams), vp, vp, C.POINTER(PriorPlane),
                                                        C.POINTER(PlanePriorStats)]
        L.hcmvs_get_plane_prior_trace.argtypes = [vp, u8p, i32p, i32p, C.c_int32, i32p]
        L.hcmvs_get_plane_prior_cluster_trace.argtypes = [vp, i32p, C.c_int32, i32p]
        L.hcmvs_get_plane_prior_refit_trace.argtypes = [vp, i32p, fp, C.c_int32, i32p]
        L.hcmvs_get_plane_prior_refit_stats.argtypes = [vp, C.POINTER(PlanePriorRefitStats)]
        _lib = L
    return _lib


def default_params(**kw):
    p = Params()
    lib().hcmvs_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_prior_params(**kw):
    p = PriorParams()
    lib().hcmvs_default_prior_params(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def default_plane_prior_params(**kw):
    """hcmvs_default_plane_prior_params: the reference's values (255, 0.18, 0.3, 10, 0.01, 80, 2, 0.25), 256 rounds, seed 1, cluster_mul 0 (a
    plane's inliers are not clustered into connected components; > 0: the cell edge in average spacings, --ransac-cluster), refit_iters 0 (a
    round's winner is not refitted; 1 .. 16: least-squares steps over its inliers in the eps / 4 band, --plane-refit); then the overrides"""
    p = PlanePriorParams()
    lib().hcmvs_default_plane_prior_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def default_geo_params(**kw):
    """hcmvs_default_geo_params (off, 0.25, 0.15, 150, 160, 2, 3.0), then the overrides"""
    p = GeoParams()
    lib().hcmvs_default_geo_params(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def default_view_select_params(**kw):
    """hcmvs_default_view_select_params: the reference's defaults (DepthMap.cpp:72-86, SceneDensify.cpp:313-322), then the overrides"""
    p = ViewSelectParams()
    lib().hcmvs_default_view_select_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def _f(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _d(a):
    a = np.ascontiguousarray(a, np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


class Context:
    """One device context (hcmvs_ctx).  Host-buffer methods mirror DepthMapsData's per-image calls."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().hcmvs_create(device, C.byref(self._h))
        if rc != OK:
            raise HcmvsError(rc, "hcmvs_create failed (no usable gfx950 device?)")
        self.shapes = {}

    def close(self):
        if self._h:
            lib().hcmvs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != OK:
            raise HcmvsError(rc, lib().hcmvs_last_error(self._h).decode())

    def set_stream(self, stream_ptr):
        self._chk(lib().hcmvs_set_stream(self._h, C.c_void_p(stream_ptr)))

    def synchronize(self):
        self._chk(lib().hcmvs_synchronize(self._h))

    def upload_view(self, vid, gray, K, R, Cc, bgr=None):
        """gray None (with a colour image): a fuse-only view -- camera, colours, gradient map, no estimate"""
        Ka, Kp = _d(K); Ra, Rp = _d(R); Ca, Cp = _d(Cc)
        bp = None
        if bgr is not None:
            bgr = np.ascontiguousarray(bgr, np.uint8)
            bp = bgr.ctypes.data_as(C.POINTER(C.c_uint8))
        if gray is not None:
            gray = np.ascontiguousarray(gray, np.float32)
            h, w = gray.shape
        else:
            h, w = bgr.shape[:2]
        self._chk(lib().hcmvs_upload_view(self._h, vid, w, h, None if gray is None else _f(gray), bp, Kp, Rp, Cp))
        self.shapes[vid] = (h, w)

    def set_view_device(self, vid, w, h, d_gray_ptr, K, R, Cc, d_bgr_ptr=None):
        Ka, Kp = _d(K); Ra, Rp = _d(R); Ca, Cp = _d(Cc)
        self._chk(lib().hcmvs_set_view_device(self._h, vid, w, h, C.c_void_p(d_gray_ptr),
                                              C.c_void_p(d_bgr_ptr) if d_bgr_ptr else None, Kp, Rp, Cp))
        self.shapes[vid] = (h, w)

    def rescale_view(self, src_id, dst_id, scale):
        """DepthData::ViewData::ScaleImage: view dst_id = view src_id resampled by scale; returns (gray, K) of the new view"""
        self._chk(lib().hcmvs_rescale_view(self._h, src_id, dst_id, C.c_float(scale)))
        w = C.c_int32(); h = C.c_int32(); K = (C.c_double * 9)()
        self._chk(lib().hcmvs_get_view_info(self._h, dst_id, C.byref(w), C.byref(h), K))
        self.shapes[dst_id] = (h.value, w.value)
        g = np.empty((h.value, w.value), np.float32)
        self._chk(lib().hcmvs_get_view_gray(self._h, dst_id, _f(g)))
        return g, np.array(list(K), np.float64).reshape(3, 3)

    def release_view(self, vid):
        self._chk(lib().hcmvs_release_view(self._h, vid))
        self.shapes.pop(vid, None)

    def gradient_map(self, vid):
        h, w = self.shapes[vid]
        out = np.empty((h, w), np.uint8)
        self._chk(lib().hcmvs_get_gradient_map(self._h, vid, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def set_ignore_mask(self, vid, labels, ignore):
        """--ignore-mask-label for reference view vid: labels is a 16-bit label image of any size (None removes the mask); pixels whose
        label (resampled INTER_NEAREST to the view's size) is one of `ignore` are left out of every estimate of the view"""
        ig = np.ascontiguousarray(list(ignore) if labels is not None else [], np.int64)
        ig = np.clip(ig, -1, 1 << 20).astype(np.int32)  # (atoi values beyond int32 match nothing either)
        igp = ig.ctypes.data_as(C.POINTER(C.c_int32)) if len(ig) else None
        if labels is None:
            self._chk(lib().hcmvs_set_ignore_mask(self._h, vid, None, 0, 0, None, 0))
            return
        lab = np.ascontiguousarray(labels, np.uint16)
        assert lab.ndim == 2
        self._chk(lib().hcmvs_set_ignore_mask(self._h, vid, lab.ctypes.data_as(C.POINTER(C.c_uint16)), lab.shape[1], lab.shape[0], igp, len(ig)))

    def set_ignore_mask_device(self, vid, d_labels_ptr, lw, lh, ignore):
        """the same with the label image (u16, lh x lw) in device memory"""
        ig = np.clip(np.ascontiguousarray(list(ignore), np.int64), -1, 1 << 20).astype(np.int32)
        igp = ig.ctypes.data_as(C.POINTER(C.c_int32)) if len(ig) else None
        self._chk(lib().hcmvs_set_ignore_mask_device(self._h, vid, C.c_void_p(d_labels_ptr), lw, lh, igp, len(ig)))

    def ignore_mask(self, vid):
        """the keep-mask of view vid as the estimate uses it: (h, w) u8, 1 = estimated, 0 = ignored (all 1 without a mask)"""
        h, w = self.shapes[vid]
        out = np.empty((h, w), np.uint8)
        self._chk(lib().hcmvs_get_ignore_mask(self._h, vid, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def splat_init(self, vid, points_xyz):
        h, w = self.shapes[vid]
        pts = np.ascontiguousarray(points_xyz, np.float32)
        depth = np.zeros((h, w), np.float32); normal = np.zeros((h, w, 3), np.float32)
        dmin = C.c_float(); dmax = C.c_float()
        self._chk(lib().hcmvs_splat_init(self._h, vid, _f(pts), len(pts), _f(depth), _f(normal), C.byref(dmin),
                                         C.byref(dmax)))
        return depth, normal, dmin.value, dmax.value

    def triangulate_init(self, vid, points_xyz, avg_depth=0.0, add_corners=True):
        """TriangulatePoints2DepthMap as InitDepthMap uses it: returns (depth, normal, d_min, d_max)"""
        h, w = self.shapes[vid]
        pts = np.ascontiguousarray(points_xyz, np.float32)
        depth = np.zeros((h, w), np.float32); normal = np.zeros((h, w, 3), np.float32)
        dmin = C.c_float(); dmax = C.c_float()
        self._chk(lib().hcmvs_triangulate_init(self._h, vid, _f(pts), len(pts), C.c_float(avg_depth), int(add_corners), _f(depth),
                                               _f(normal), C.byref(dmin), C.byref(dmax)))
        return depth, normal, dmin.value, dmax.value

    def triangulate_init_device(self, vid, points_xyz, d_depth_ptr, d_normal_ptr, avg_depth=0.0, add_corners=True):
        """triangulate_init with the pixel loop on the device: points_xyz is a host array (n, 3), d_depth_ptr (h*w f32) and d_normal_ptr
        (h*w*3 f32) are device addresses, every pixel of which is written on the context's stream (not synchronised; ordered before a
        following estimate*_device).  Bit-identical to triangulate_init.  Returns (d_min, d_max)."""
        pts = np.ascontiguousarray(points_xyz, np.float32).reshape(-1, 3)
        dmin = C.c_float(); dmax = C.c_float()
        self._chk(lib().hcmvs_triangulate_init_device(self._h, vid, _f(pts), len(pts), C.c_float(avg_depth), int(add_corners),
                                                      C.c_void_p(d_depth_ptr), C.c_void_p(d_normal_ptr), C.byref(dmin), C.byref(dmax)))
        return dmin.value, dmax.value

    def splat_init_device(self, vid, points_xyz, d_depth_ptr, d_normal_ptr):
        """splat_init on the device, arguments and return value as triangulate_init_device; the normals are 0 everywhere"""
        pts = np.ascontiguousarray(points_xyz, np.float32).reshape(-1, 3)
        dmin = C.c_float(); dmax = C.c_float()
        self._chk(lib().hcmvs_splat_init_device(self._h, vid, _f(pts), len(pts), C.c_void_p(d_depth_ptr), C.c_void_p(d_normal_ptr),
                                                C.byref(dmin), C.byref(dmax)))
        return dmin.value, dmax.value

    def init_stats(self):
        """hcmvs_get_init_stats: the counters of the last *_init_device call, as a dict; waits for the context's stream"""
        st = InitStats()
        self._chk(lib().hcmvs_get_init_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in InitStats._fields_}

    def handoff_maps_device(self, items, mode):
        """hcmvs_handoff_maps_device: the hand-off between two pyramid levels (binding.handoff_maps states the two modes) for a batch of
        images of any mix of sizes in one pass on the context's stream.  items: list of dicts(src_depth, src_normal, dst_depth, dst_normal
        [DEVICE addresses], src_w, src_h, dst_w, dst_h[, d_min, d_max]); every pixel of the destination maps is written, bit-identical to
        handoff_maps.  The call waits for the stream once; it is ordered before a following estimate*_device.  Returns one dict per item:
        d_min, d_max, status (HANDOFF_OK / HANDOFF_EMPTY), n_valid, n_clamped, n_rescaled"""
        arr = _handoff_items(items)
        self._chk(lib().hcmvs_handoff_maps_device(self._h, arr, len(items), _handoff_mode(mode)))
        return _handoff_results(arr, len(items))

    def remove_speckles_device(self, items, thr=None, speckle_size=100):
        """hcmvs_remove_speckles_batch_device: the speckle filter (binding.remove_speckles states the rule) over a batch of 1..64 maps of any
        mix of sizes in DEVICE memory, in place, in one set of launches on the context's stream.  items: list of dicts(width, height,
        d_depth[, d_normal, d_conf, d_labels]): addresses, e.g. tensor.data_ptr(); d_labels (int32, width * height) receives the canonical
        labels as before the removal.  thr None: upstream's 0.01f * 0.7f.  The call waits for the stream once.  Returns the stats of the
        call, summed over its maps, as a dict"""
        arr = (SpeckleItem * max(len(items), 1))()
        for a, it in zip(arr, items):
            a.width, a.height = int(it["width"]), int(it["height"])
            a.d_depth = it.get("d_depth") or None; a.d_normal = it.get("d_normal") or None
            a.d_conf = it.get("d_conf") or None; a.d_labels = it.get("d_labels") or None
        st = SpeckleStats()
        self._chk(lib().hcmvs_remove_speckles_batch_device(self._h, arr if items is not None else None, len(items), C.c_float(SPECKLE_DIFF if thr is None else thr),
                                                           int(speckle_size), C.byref(st)))
        return _speckle_stats(st)

    def handoff_stats(self):
        """hcmvs_get_handoff_stats: counters of the last handoff_maps_device call, summed over its items, and its device time"""
        st = HandoffStats()
        self._chk(lib().hcmvs_get_handoff_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in HandoffStats._fields_}

    def estimate(self, ref_id, src_ids, params, d_min, d_max, depth, normal, conf=None):
        """EstimateDepthMap on host maps (copied); returns (depth, normal, conf)."""
        h, w = self.shapes[ref_id]
        d = np.ascontiguousarray(depth, np.float32).copy()
        n = np.ascontiguousarray(normal, np.float32).copy()
        c = np.zeros((h, w), np.float32) if conf is None else np.ascontiguousarray(conf, np.float32).copy()
        assert d.shape == (h, w) and n.shape == (h, w, 3)
        ids = (C.c_uint32 * len(src_ids))(*src_ids)
        self._chk(lib().hcmvs_estimate(self._h, ref_id, ids, len(src_ids), C.byref(params), d_min, d_max, _f(d),
                                       _f(n), _f(c)))
        return d, n, c

    def estimate_device(self, ref_id, src_ids, params, d_min, d_max, d_depth_ptr, d_normal_ptr, d_conf_ptr):
        ids = (C.c_uint32 * len(src_ids))(*src_ids)
        self._chk(lib().hcmvs_estimate_device(self._h, ref_id, ids, len(src_ids), C.byref(params), d_min, d_max,
                                              C.c_void_p(d_depth_ptr), C.c_void_p(d_normal_ptr),
                                              C.c_void_p(d_conf_ptr)))

    @staticmethod
    def _batch_items(items):
        arr = (BatchItem * len(items))()
        keep = []
        for i, it in enumerate(items):
            ids = (C.c_uint32 * len(it["src_ids"]))(*it["src_ids"]); keep.append(ids)
            arr[i].ref_id = it["ref_id"]; arr[i].src_ids = ids; arr[i].n_src = len(it["src_ids"])
            arr[i].seed_offset = it.get("seed_offset", 0); arr[i].d_min = it["d_min"]; arr[i].d_max = it["d_max"]
            arr[i].d_depth = it["d_depth"]; arr[i].d_normal = it["d_normal"]; arr[i].d_conf = it["d_conf"]
            arr[i].d_hint_depth = it.get("d_hint_depth"); arr[i].d_hint_normal = it.get("d_hint_normal")
        arr._keep = keep
        return arr

    def estimate_batch_device(self, items, params):
        """items: list of dicts (ref_id, src_ids, d_min, d_max, d_depth, d_normal, d_conf [device pointers], seed_offset)"""
        arr = self._batch_items(items)
        self._chk(lib().hcmvs_estimate_batch_device(self._h, arr, len(items), C.byref(params)))

    def estimate_sweeps_batch_device(self, items, params, first_sweep, n_sweeps):
        """the reference's extra sweeps: sweeps first_sweep .. first_sweep + n_sweeps - 1 on maps that are the state an estimate leaves
        between outer iterations (d_depth, d_normal, d_conf = the score), then the end pass as in estimate_batch_device; items as there"""
        arr = self._batch_items(items)
        self._chk(lib().hcmvs_estimate_sweeps_batch_device(self._h, arr, len(items), C.byref(params), int(first_sweep), int(n_sweeps)))

    # ---- depth priors (--n-para_prior, --sigma-prior, --n-photo2geo; DepthMap.cpp:941-954) ------------------

    def set_prior_params(self, para_prior=None, sigma_prior=None, photo2geo=None):
        """the prior term's options for the estimates that follow; None keeps the reference's default (0.5, 0.2, 2)"""
        p = default_prior_params()
        if para_prior is not None:
            p.para_prior = para_prior
        if sigma_prior is not None:
            p.sigma_prior = sigma_prior
        if photo2geo is not None:
            p.photo2geo = photo2geo
        self._chk(lib().hcmvs_set_prior_params(self._h, C.byref(p)))

    def set_depth_prior(self, vid, prior):
        """the prior depth map of view vid as a reference view: (h, w) float32 on the host, copied; None removes it"""
        if prior is None:
            self._chk(lib().hcmvs_set_depth_prior(self._h, vid, None))
            return
        a = np.ascontiguousarray(prior, np.float32)
        assert a.shape == tuple(self.shapes[vid])
        self._chk(lib().hcmvs_set_depth_prior(self._h, vid, _f(a)))

    def set_depth_prior_device(self, vid, d_prior_ptr):
        """the same in device memory (w * h floats at the view's size), caller-owned, not copied; None removes it"""
        self._chk(lib().hcmvs_set_depth_prior_device(self._h, vid, C.c_void_p(d_prior_ptr) if d_prior_ptr else None))

    def prior_stats(self):
        """counters of the prior term of the last estimate: dict(evals_prior, pixels_prior)"""
        s = PriorStats()
        self._chk(lib().hcmvs_get_prior_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in PriorStats._fields_}

    # ---- plane priors (GenerateDepthPrior, SceneDensify.cpp:1550-1950) --------------

    def set_prior_region(self, vid, labels, region_label=255):
        """the region of view vid in which planes are fitted: the pixels of the 16-bit label image (any size, resampled INTER_NEAREST to
        the view's) that equal region_label; None removes the region"""
        if labels is None:
            self._chk(lib().hcmvs_set_prior_region(self._h, vid, None, 0, 0, 0))
            return
        lab = np.ascontiguousarray(labels, np.uint16)
        assert lab.ndim == 2
        self._chk(lib().hcmvs_set_prior_region(self._h, vid, lab.ctypes.data_as(C.POINTER(C.c_uint16)), lab.shape[1], lab.shape[0], int(region_label)))

    def get_prior_region(self, vid):
        """(h, w) u8, 1 = inside the region (all 0 without one)"""
        h, w = self.shapes[vid]
        out = np.empty((h, w), np.uint8)
        self._chk(lib().hcmvs_get_prior_region(self._h, vid, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def generate_plane_prior_device(self, vid, d_depth_ptr, d_normal_ptr, d_conf_ptr, d_prior_ptr, d_prior_normal_ptr=None, params=None):
        """hcmvs_generate_plane_prior_device: the prior of view vid from its maps in device memory (the state an estimate leaves between
        outer iterations; read only) into d_prior_ptr (h*w f32, every pixel written) and, when given, d_prior_normal_ptr (h*w*3 f32).
        Blocking.  Returns (planes, stats): planes a list of dicts(normal, n_inliers, centre, quad (4, 2), box_fallback), stats a dict of
        the hcmvs_plane_prior_stats fields.  The prior feeds set_depth_prior_device unchanged"""
        p = params if params is not None else default_plane_prior_params()
        tab = (PriorPlane * MAX_PRIOR_PLANES)()
        st = PlanePriorStats()
        self._chk(lib().hcmvs_generate_plane_prior_device(self._h, vid, C.c_void_p(d_depth_ptr) if d_depth_ptr else None,
                                                          C.c_void_p(d_normal_ptr) if d_normal_ptr else None, C.c_void_p(d_conf_ptr) if d_conf_ptr else None,
                                                          C.byref(p), C.c_void_p(d_prior_ptr) if d_prior_ptr else None,
                                                          C.c_void_p(d_prior_normal_ptr) if d_prior_normal_ptr else None, tab, C.byref(st)))
        planes = [dict(normal=np.array(list(t.normal), np.float32), n_inliers=int(t.n_inliers), centre=np.array(list(t.centre), np.float64),
                       quad=np.array(list(t.quad), np.float64).reshape(4, 2), box_fallback=int(t.box_fallback)) for t in tab[:st.planes]]
        rs = PlanePriorRefitStats()                      # the refit's counters are a struct of their own in the C-ABI; here they join the dict
        self._chk(lib().hcmvs_get_plane_prior_refit_stats(self._h, C.byref(rs)))
        out = {k: getattr(st, k) for k, _ in PlanePriorStats._fields_}
        out.update(refit_rounds=int(rs.refit_rounds), refit_steps=int(rs.refit_steps))
        return planes, out

    def plane_prior_trace(self, vid):
        """the decisions of the last generate_plane_prior_device (of view vid's size): dict(stage (h, w) u8: 0 outside the region, 1 region,
        2 sample, 3 planar, 4 fitting set; assignment (h, w) i32: plane or -1; rounds (n, 6) i32: winner or -1, cnt_0 .. cnt_3, valid candidates)"""
        h, w = self.shapes[vid]
        stage = np.empty((h, w), np.uint8); asg = np.empty((h, w), np.int32); n = C.c_int32()
        i32p = C.POINTER(C.c_int32)
        self._chk(lib().hcmvs_get_plane_prior_trace(self._h, stage.ctypes.data_as(C.POINTER(C.c_uint8)), asg.ctypes.data_as(i32p), None, 0, C.byref(n)))
        rounds = np.zeros((max(n.value, 1), 6), np.int32)
        self._chk(lib().hcmvs_get_plane_prior_trace(self._h, None, None, rounds.ctypes.data_as(i32p), n.value, C.byref(n)))
        return dict(stage=stage, assignment=asg, rounds=rounds[:n.value])

    def plane_prior_cluster_trace(self):
        """what the clustering (cluster_mul) decided in every round of the last generate_plane_prior_device: (n, 4) i32 -- occupied cells,
        components, size of the largest component, accepted 0 / 1; zeros for a round without a winner, 0, 0, cnt_0, 1 with clustering off"""
        n = C.c_int32()
        i32p = C.POINTER(C.c_int32)
        self._chk(lib().hcmvs_get_plane_prior_cluster_trace(self._h, None, 0, C.byref(n)))
        rows = np.zeros((max(n.value, 1), 4), np.int32)
        self._chk(lib().hcmvs_get_plane_prior_cluster_trace(self._h, rows.ctypes.data_as(i32p), n.value, C.byref(n)))
        return rows[:n.value]

    def get_plane_prior_refit_trace(self):
        """what the refit (refit_iters) decided in every round of the last generate_plane_prior_device: (steps (n, 6) i32 -- steps solved,
        steps kept, cnt_0 .. cnt_3 of the round's final plane --, planes (n, 4) f32 -- the final n, d); zeros for a round without a winner,
        0, 0, the candidate's counts and the candidate's plane with refit_iters = 0"""
        n = C.c_int32()
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        self._chk(lib().hcmvs_get_plane_prior_refit_trace(self._h, None, None, 0, C.byref(n)))
        steps = np.zeros((max(n.value, 1), 6), np.int32); planes = np.zeros((max(n.value, 1), 4), np.float32)
        self._chk(lib().hcmvs_get_plane_prior_refit_trace(self._h, steps.ctypes.data_as(i32p), planes.ctypes.data_as(f32p), n.value, C.byref(n)))
        return steps[:n.value], planes[:n.value]

    def stats(self):
        s = Stats()
        self._chk(lib().hcmvs_get_stats(self._h, C.byref(s)))
        return s

    # ---- geometric consistency (--geo-consistency) -------------------------------

    def set_geo_params(self, on=True, **kw):
        """the geometric-consistency term for the estimates that follow: on, para_tapa, para_tapa2, txthreshold, txthreshold2, photo2geo,
        max_px; a missing key keeps its default (hcmvs_default_geo_params).  The source views' maps are the ones registered with
        set_spread_maps_device."""
        p = default_geo_params(on=int(bool(on)), **kw)
        self._chk(lib().hcmvs_set_geo_params(self._h, C.byref(p)))

    def get_geo_stats(self):
        """counters of the term of the last estimate: dict(evals_geo, pixels_geo)"""
        s = GeoStats()
        self._chk(lib().hcmvs_get_geo_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in GeoStats._fields_}

    # ---- view spread (--n-viewspread, DepthMap.cpp:1504-1608) ----------------------------------------------

    def set_viewspread(self, on):
        """switch view spread on or off for the estimates that follow (default off)"""
        self._chk(lib().hcmvs_set_viewspread(self._h, int(bool(on))))

    def set_spread_maps_device(self, vid, d_depth_ptr, d_normal_ptr, d_conf_ptr):
        """the maps view vid offers as a source view: device memory of the view's size, caller-owned, not copied; all None removes them"""
        self._chk(lib().hcmvs_set_spread_maps_device(self._h, vid, C.c_void_p(d_depth_ptr) if d_depth_ptr else None,
                                                     C.c_void_p(d_normal_ptr) if d_normal_ptr else None, C.c_void_p(d_conf_ptr) if d_conf_ptr else None))

    def spread_stats(self):
        """counters of the view spread of the last estimate: dict(slots_scored, slots_accepted, slots_dropped, candidates_outside)"""
        s = SpreadStats()
        self._chk(lib().hcmvs_get_spread_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in SpreadStats._fields_}

    # ---- filter / fuse (SceneDensify.h:69-70) -----------------------------------------------------------

    def set_depthmap(self, vid, depth, normal, conf, d_min, d_max):
        d = np.ascontiguousarray(depth, np.float32); c = np.ascontiguousarray(conf, np.float32)
        n = None if normal is None else np.ascontiguousarray(normal, np.float32)
        self._chk(lib().hcmvs_set_depthmap(self._h, vid, _f(d), None if n is None else _f(n), _f(c), d_min, d_max))

    def set_depthmap_device(self, vid, d_depth_ptr, d_normal_ptr, d_conf_ptr, d_min, d_max):
        """maps that already live in device memory (caller-owned; fusion mutates the depth map, SceneDensify.cpp:3447-3449)"""
        self._chk(lib().hcmvs_set_depthmap_device(self._h, vid, C.c_void_p(d_depth_ptr), C.c_void_p(d_normal_ptr) if d_normal_ptr else None,
                                                  C.c_void_p(d_conf_ptr), d_min, d_max))

    def get_depthmap(self, vid, with_normal=False):
        h, w = self.shapes[vid]
        d = np.empty((h, w), np.float32); c = np.empty((h, w), np.float32)
        n = np.empty((h, w, 3), np.float32) if with_normal else None
        self._chk(lib().hcmvs_get_depthmap(self._h, vid, _f(d), None if n is None else _f(n), _f(c)))
        return (d, n, c) if with_normal else (d, c)

    def set_neighbors(self, vid, ids):
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        self._chk(lib().hcmvs_set_neighbors(self._h, vid, arr, len(ids)))

    def set_fuse_order(self, mode):
        """0: raster order (bit-exact with the reference's sequential fusion), 1: hashed order (few rounds)"""
        self._chk(lib().hcmvs_set_fuse_order(self._h, int(mode)))

    def filter(self, ref_id, neighbor_ids, adjust=True, n_min_views=2, n_min_views_adjust=1, depth_diff_threshold=0.01):
        """FilterDepthMap: returns (new_depth, new_conf, n_processed, n_discarded)"""
        h, w = self.shapes[ref_id]
        d = np.empty((h, w), np.float32); c = np.empty((h, w), np.float32)
        ids = (C.c_uint32 * len(neighbor_ids))(*neighbor_ids)
        npr = C.c_uint64(); nd = C.c_uint64()
        self._chk(lib().hcmvs_filter(self._h, ref_id, ids, len(neighbor_ids), int(adjust), n_min_views, n_min_views_adjust,
                                     depth_diff_threshold, _f(d), _f(c), C.byref(npr), C.byref(nd)))
        return d, c, npr.value, nd.value

    def filter_sequence(self, ids, max_neighbors=8, adjust=True, n_min_views=2, n_min_views_adjust=1, depth_diff_threshold=0.01):
        """The filter stage (Scene::DenseReconstructionFilter, SceneDensify.cpp:4100-4185): every image of ids that has registered maps is
        filtered against the first max_neighbors entries of its neighbour list that have maps, all from the maps as they stand now; depth
        and confidence are then updated in place (get_depthmap reads them back).  Returns dict(n_processed, n_discarded, n_filtered,
        n_skipped, batch, ms_device, device_bytes, image_processed, image_discarded): the last two per entry of ids (0 for a skipped image)"""
        ids = [int(i) for i in ids]
        arr = (C.c_uint32 * max(len(ids), 1))(*ids)
        per = np.zeros((2, max(len(ids), 1)), np.uint64)
        st = FilterStats()
        st.image_processed = per[0].ctypes.data_as(C.POINTER(C.c_uint64)); st.image_discarded = per[1].ctypes.data_as(C.POINTER(C.c_uint64))
        self._chk(lib().hcmvs_filter_sequence(self._h, arr, len(ids), int(max_neighbors), int(bool(adjust)), int(n_min_views), int(n_min_views_adjust),
                                              C.c_float(depth_diff_threshold), C.byref(st)))
        out = {k: getattr(st, k) for k, _ in FilterStats._fields_[:7]}
        out["image_processed"] = [int(x) for x in per[0][:len(ids)]]; out["image_discarded"] = [int(x) for x in per[1][:len(ids)]]
        return out

    def fuse(self, order, capacity, n_min_views_fuse=2, depth_diff_threshold=0.01, normal_diff_deg=25.0, depthweight=1.0,
             normalweight=1.0, with_normals=True, with_colors=True):
        """FuseDepthMaps: returns dict(xyz, normal, bgr, n_views, n_points, n_depths)"""
        xyz = np.empty((capacity, 3), np.float32)  # only the first n_points rows are written and returned
        nrm = np.empty((capacity, 3), np.float32) if with_normals else None
        bgr = np.empty((capacity, 3), np.uint8) if with_colors else None
        nv = np.empty(capacity, np.uint32)
        ids = (C.c_uint32 * len(order))(*order)
        npts = C.c_uint64(); nd = C.c_uint64()
        self._chk(lib().hcmvs_fuse(self._h, ids, len(order), n_min_views_fuse, depth_diff_threshold, normal_diff_deg,
                                   depthweight, normalweight, capacity, _f(xyz), None if nrm is None else _f(nrm),
                                   None if bgr is None else bgr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   nv.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(npts), C.byref(nd)))
        k = npts.value
        return dict(xyz=xyz[:k], normal=None if nrm is None else nrm[:k], bgr=None if bgr is None else bgr[:k],
                    n_views=nv[:k], n_points=k, n_depths=nd.value)

    def fuse_count(self, order, n_min_views_fuse=2, depth_diff_threshold=0.01, normal_diff_deg=25.0, depthweight=1.0, normalweight=1.0):
        """hcmvs_fuse_cloud without buffers: the fusion runs (with its side effect, the invalidated depths) and only counts.  A fusion
        repeated on the maps it has left makes the same decisions, so buffers of exactly (n_points, n_view_entries) hold the cloud of the
        fusion that follows.  Returns (n_points, n_depths, n_view_entries)."""
        cl = Cloud()
        ids = (C.c_uint32 * len(order))(*order)
        self._chk(lib().hcmvs_fuse_cloud(self._h, ids, len(order), n_min_views_fuse, depth_diff_threshold, normal_diff_deg, depthweight, normalweight,
                                         C.byref(cl)))
        return cl.n_points, cl.n_depths, cl.n_view_entries

    def fuse_cloud(self, order, capacity, views_capacity, n_min_views_fuse=2, depth_diff_threshold=0.01, normal_diff_deg=25.0, depthweight=1.0,
                   normalweight=1.0):
        """hcmvs_fuse_cloud: the complete PointCloud (points, view lists + weights as CSR, colours, normals)"""
        xyz = np.empty((capacity, 3), np.float32); nrm = np.empty((capacity, 3), np.float32); bgr = np.empty((capacity, 3), np.uint8)
        nv = np.empty(capacity, np.uint32); vids = np.empty(max(views_capacity, 1), np.uint32); vwts = np.empty(max(views_capacity, 1), np.float32)
        cl = Cloud()
        cl.capacity = capacity; cl.xyz = _f(xyz); cl.normal = _f(nrm); cl.bgr = bgr.ctypes.data_as(C.POINTER(C.c_uint8))
        cl.n_views = nv.ctypes.data_as(C.POINTER(C.c_uint32)); cl.views_capacity = views_capacity
        cl.view_ids = vids.ctypes.data_as(C.POINTER(C.c_uint32)); cl.view_weights = _f(vwts)
        ids = (C.c_uint32 * len(order))(*order)
        self._chk(lib().hcmvs_fuse_cloud(self._h, ids, len(order), n_min_views_fuse, depth_diff_threshold, normal_diff_deg, depthweight, normalweight,
                                         C.byref(cl)))
        k, ne = cl.n_points, cl.n_view_entries
        return dict(xyz=xyz[:k], normal=nrm[:k], bgr=bgr[:k], n_views=nv[:k], n_points=k, n_depths=cl.n_depths, view_ids=vids[:ne],
                    view_weights=vwts[:ne])

    def estimate_point_colors(self, xyz, n_views, view_ids):
        x = np.ascontiguousarray(xyz, np.float32); nv = np.ascontiguousarray(n_views, np.uint32); vi = np.ascontiguousarray(view_ids, np.uint32)
        out = np.empty((len(x), 3), np.uint8)
        self._chk(lib().hcmvs_estimate_point_colors(self._h, len(x), _f(x), nv.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    vi.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def estimate_point_normals(self, xyz, n_views, view_ids, n_neighbors=16):
        x = np.ascontiguousarray(xyz, np.float32); nv = np.ascontiguousarray(n_views, np.uint32); vi = np.ascontiguousarray(view_ids, np.uint32)
        out = np.empty((len(x), 3), np.float32)
        self._chk(lib().hcmvs_estimate_point_normals(self._h, len(x), _f(x), nv.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                     vi.ctypes.data_as(C.POINTER(C.c_uint32)), n_neighbors, _f(out)))
        return out

    def point_cloud_filter(self, xyz, n_views, view_ids, cameras, th_remove=-1):
        """Scene::PointCloudFilter on the device: cameras = one dict per image (K, R, C at width x height; width 0 or a missing K =
        uncalibrated).  Returns (visibility int32 per point, kept uint32 indices in the reference's output order); the counters of the
        call are left in self.visibility_stats"""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nv = np.ascontiguousarray(n_views, np.uint32); vi = np.ascontiguousarray(view_ids, np.uint32)
        m = len(cameras)
        wh = np.zeros((max(m, 1), 2), np.int32); K = np.zeros((max(m, 1), 9)); R = np.zeros((max(m, 1), 9)); Cc = np.zeros((max(m, 1), 3))
        for j, cam in enumerate(cameras):
            if cam is None or cam.get("K") is None or not cam.get("width"):
                continue
            wh[j] = cam["width"], cam["height"]
            K[j] = np.asarray(cam["K"], np.float64).ravel(); R[j] = np.asarray(cam["R"], np.float64).ravel(); Cc[j] = np.asarray(cam["C"], np.float64)
        vis = np.empty(len(x), np.int32); kept = np.empty(max(len(x), 1), np.uint32)
        nk = C.c_uint64(); st = VisibilityStats()
        u32 = C.POINTER(C.c_uint32); dp = C.POINTER(C.c_double)
        self._chk(lib().hcmvs_point_cloud_filter(self._h, len(x), _f(x), nv.ctypes.data_as(u32), vi.ctypes.data_as(u32), m,
                                                 wh.ctypes.data_as(C.POINTER(C.c_int32)), K.ctypes.data_as(dp), R.ctypes.data_as(dp),
                                                 Cc.ctypes.data_as(dp), int(th_remove), vis.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 kept.ctypes.data_as(u32), C.byref(nk), C.byref(st)))
        self.visibility_stats = {k: getattr(st, k) for k, _ in VisibilityStats._fields_}
        return vis, kept[:nk.value].copy()

    def sample_mesh(self, vertices, faces, sample, seed=0, texcoords=None, texture_bgr=None, count_only=False):
        """Mesh::SamplePoints on the device (DensifyPointCloud --sample-mesh): sample > 0 points per square unit, < 0 minus the number of
        points; texcoords (n_faces, 3, 2) and texture_bgr (h, w, 3) both or neither.  Returns (xyz (n, 3) f32, face_ids (n,) u32, bgr (n, 3)
        u8 or None, stats); count_only: no cloud is produced, xyz and face_ids are None and stats["n_points"] says how many points it has"""
        V = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
        Fc = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        tc = None if texcoords is None else np.ascontiguousarray(texcoords, np.float32).reshape(-1, 6)
        tex = None if texture_bgr is None else np.ascontiguousarray(texture_bgr, np.uint8)
        if tc is not None and len(tc) != len(Fc):
            raise ValueError("texcoords: 6 values per face expected")
        if tex is not None and (tex.ndim != 3 or tex.shape[2] != 3):
            raise ValueError("texture_bgr: (h, w, 3) expected")
        th, tw = (0, 0) if tex is None else tex.shape[:2]
        head = (self._h, len(V), _f(V), len(Fc), Fc.ctypes.data_as(u32), None if tc is None else _f(tc), None if tex is None else tex.ctypes.data_as(u8),
                tw, th, C.c_float(sample), C.c_uint64(seed))
        n = C.c_uint64(); st = MeshSampleStats()
        self._chk(lib().hcmvs_sample_mesh(*head, 0, None, None, None, C.byref(n), C.byref(st)))
        if count_only or n.value == 0:
            stats = {k: getattr(st, k) for k, _ in MeshSampleStats._fields_}
            if count_only:
                return None, None, None, stats
            return np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), None if tex is None else np.zeros((0, 3), np.uint8), stats
        cap = n.value
        xyz = np.empty((cap, 3), np.float32); fid = np.empty(cap, np.uint32)
        bgr = None if tex is None else np.empty((cap, 3), np.uint8)
        self._chk(lib().hcmvs_sample_mesh(*head, cap, _f(xyz), fid.ctypes.data_as(u32), None if bgr is None else bgr.ctypes.data_as(u8), C.byref(n), C.byref(st)))
        assert n.value == cap
        return xyz, fid, bgr, {k: getattr(st, k) for k, _ in MeshSampleStats._fields_}

    def select_views_raw(self, cameras, sizes, xyz, n_views, view_ids, number_views=5, with_points=True, **params):
        """hcmvs_select_views as arrays: dict(status, n_seen, avg_depth, n_candidates, n_neighbors, n_srcs (n_images each), nb_id, nb_points,
        nb_scale, nb_angle, nb_area, nb_score, src_scale ((n_images, n_max_views) each), points_first, point_ids (with_points), stats)"""
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        nv = np.ascontiguousarray(n_views, np.uint32); vi = np.ascontiguousarray(view_ids, np.uint32)
        if len(nv) != len(x) or int(nv.sum(dtype=np.uint64)) != len(vi):
            raise ValueError("select_views: n_views does not describe view_ids")
        if len(sizes) != len(cameras):
            raise ValueError("select_views: one size per camera expected")
        p = default_view_select_params(number_views=int(number_views), **params)
        m = len(cameras)
        wh = np.zeros((max(m, 1), 2), np.int32); K = np.zeros((max(m, 1), 9)); R = np.zeros((max(m, 1), 9)); Cc = np.zeros((max(m, 1), 3))
        for j, cam in enumerate(cameras):
            if cam is None or cam.get("K") is None or sizes[j] is None or not sizes[j][0]:
                continue
            wh[j] = sizes[j][0], sizes[j][1]
            K[j] = np.asarray(cam["K"], np.float64).ravel(); R[j] = np.asarray(cam["R"], np.float64).ravel(); Cc[j] = np.asarray(cam["C"], np.float64)
        M = max(int(p.n_max_views), 1)
        res = dict(status=np.zeros(max(m, 1), np.int32))
        for k in ("n_seen", "n_candidates", "n_neighbors", "n_srcs"):
            res[k] = np.zeros(max(m, 1), np.uint32)
        res["avg_depth"] = np.zeros(max(m, 1), np.float32)
        for k in ("nb_id", "nb_points"):
            res[k] = np.zeros((max(m, 1), M), np.uint32)
        for k in ("nb_scale", "nb_angle", "nb_area", "nb_score", "src_scale"):
            res[k] = np.zeros((max(m, 1), M), np.float32)
        if with_points:
            res["points_first"] = np.zeros(m + 1, np.uint64); res["point_ids"] = np.zeros(max(len(vi), 1), np.uint32)
        sel = ViewSelection()
        for k, a in res.items():
            setattr(sel, k, a.ctypes.data_as(dict(ViewSelection._fields_)[k]))
        st = ViewSelectStats()
        u32, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
        self._chk(lib().hcmvs_select_views(self._h, m, wh.ctypes.data_as(C.POINTER(C.c_int32)), K.ctypes.data_as(dp), R.ctypes.data_as(dp), Cc.ctypes.data_as(dp),
                                           len(x), _f(x), nv.ctypes.data_as(u32), vi.ctypes.data_as(u32), C.byref(p), C.byref(sel), C.byref(st)))
        n_ids = int(res["points_first"][m]) if with_points else 0
        res = {k: a[:n_ids] if k == "point_ids" else a if k == "points_first" else a[:m] for k, a in res.items()}
        res["stats"] = {k: getattr(st, k) for k, _ in ViewSelectStats._fields_}
        return res

    def select_views(self, cameras, sizes, xyz, n_views, view_ids, number_views=5, **params):
        """DepthMapsData::SelectViews (SceneDensify.cpp:307-327) + the cut of DepthMapsData::InitViews (:362-367) for every image of a scene, on
        the device (hcmvs_select_views).  cameras: one dict(K, R, C) per image at the image's size (None = uncalibrated); sizes: (width, height)
        per image; the sparse cloud as CSR (xyz (n, 3) f32, n_views (n,), view_ids ascending per point); params: the fields of
        hcmvs_view_select_params (n_max_views, min_angle_deg, ...).  Returns one entry per image: None when no views could be selected, else
        dict(points [indices into xyz], neighbors [dict(id, points, scale, angle, area, score)] in decreasing score, srcs [(id, scale)],
        avg_depth, status).  The counters and the per-image status / n_seen / n_candidates arrays are left in self.view_select_stats"""
        r = self.select_views_raw(cameras, sizes, xyz, n_views, view_ids, number_views=number_views, with_points=True, **params)
        self.view_select_stats = dict(r["stats"], status=r["status"], n_seen=r["n_seen"], n_candidates=r["n_candidates"], avg_depth=r["avg_depth"])
        out = []
        pf = r["points_first"]
        for i in range(len(cameras)):
            if r["status"][i] != 0:
                out.append(None)
                continue
            nn, ns = int(r["n_neighbors"][i]), int(r["n_srcs"][i])
            nbs = [dict(id=int(r["nb_id"][i, k]), points=int(r["nb_points"][i, k]), scale=float(r["nb_scale"][i, k]), angle=float(r["nb_angle"][i, k]),
                        area=float(r["nb_area"][i, k]), score=float(r["nb_score"][i, k])) for k in range(nn)]
            out.append(dict(points=[int(q) for q in r["point_ids"][int(pf[i]):int(pf[i + 1])]], neighbors=nbs,
                            srcs=[(int(r["nb_id"][i, k]), float(r["src_scale"][i, k])) for k in range(ns)], avg_depth=float(r["avg_depth"][i]), status=0))
        return out

    def postfilter(self, vid, order, n_min_views_fuse=2, depth_diff_threshold=0.01, normal_diff_deg=25.0, gap_size=7):
        """RemoveSmallSegments (fork version) + GapInterpolation on the registered device maps of view vid; returns pixels filled"""
        ids = (C.c_uint32 * len(order))(*order)
        nf = C.c_uint64()
        self._chk(lib().hcmvs_postfilter(self._h, vid, ids, len(order), n_min_views_fuse, depth_diff_threshold, normal_diff_deg, gap_size, C.byref(nf)))
        return nf.value

    def postfilter_sequence(self, vids, order, n_min_views_fuse=2, depth_diff_threshold=0.01, normal_diff_deg=25.0, gap_size=7):
        """the post-filters for the images vids one after the other (= postfilter(v) for v in vids); returns the pixels filled in total"""
        ids = (C.c_uint32 * len(vids))(*vids)
        ords = (C.c_uint32 * len(order))(*order)
        nf = C.c_uint64()
        self._chk(lib().hcmvs_postfilter_sequence(self._h, ids, len(vids), ords, len(order), n_min_views_fuse, depth_diff_threshold, normal_diff_deg,
                                                  gap_size, C.byref(nf)))
        return nf.value

"""The speckle filter stated in numpy: the edge masks from the two float32 expressions, the segments as the
connected components of the undirected graph they span (scipy.sparse.csgraph), the canonical label as the smallest raster index of a
segment.  Written from the rule alone; hc-mvs_amd/csrc/speckle_host.h (a flood fill) and the kernels (a union-find) are pinned to it."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

THR = np.float32(0.01) * np.float32(0.7)   # upstream's threshold, the product taken in float32
assert THR.dtype == np.float32


def _joined(dp, dq, thr):
    """both ways: |dp - dq| / dp < thr and |dp - dq| / dq < thr, float32 throughout"""
    with np.errstate(all="ignore"):
        diff = np.abs(dp - dq)
        assert diff.dtype == np.float32
        return (diff / dp < thr) & (diff / dq < thr)


def segments(depth, thr=THR):
    """(labels (h, w) int32: the smallest raster index of the pixel's segment, -1 where the depth is not valid; sizes (h, w) int64: the
    pixel count of the pixel's segment, 0 where not valid)"""
    d = np.ascontiguousarray(depth, np.float32)
    thr = np.float32(thr)
    h, w = d.shape
    n = h * w
    with np.errstate(invalid="ignore"):
        valid = d > 0          # NaN: False
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    eh = valid[:, :-1] & valid[:, 1:] & _joined(d[:, :-1], d[:, 1:], thr)
    ev = valid[:-1, :] & valid[1:, :] & _joined(d[:-1, :], d[1:, :], thr)
    a = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    b = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    # the smallest raster index of every component, and its count over valid pixels
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, np.arange(n, dtype=np.int64))
    count = np.bincount(comp[valid.ravel()], minlength=len(first))
    labels = np.where(valid.ravel(), first[comp], -1).astype(np.int32).reshape(h, w)
    sizes = np.where(valid.ravel(), count[comp], 0).astype(np.int64).reshape(h, w)
    return labels, sizes


def remove_speckles(depth, normal=None, conf=None, thr=THR, speckle_size=100):
    """dict(depth, normal, conf (None where not given), labels (before the removal), stats (the counters of hcmvs_speckle_stats))"""
    d = np.array(depth, np.float32)
    labels, sizes = segments(d, thr)
    valid = labels >= 0
    gone = valid & (sizes < int(speckle_size))
    roots = valid & (labels == np.arange(d.size, dtype=np.int64).reshape(d.shape))
    d[gone] = 0
    n = c = None
    if normal is not None:
        n = np.array(normal, np.float32); n[gone] = 0
    if conf is not None:
        c = np.array(conf, np.float32); c[gone] = 0
    stats = dict(n_valid=int(valid.sum()), n_removed=int(gone.sum()), n_segments=int(roots.sum()), n_small=int((roots & gone).sum()),
                 largest=int(sizes.max()) if sizes.size else 0)
    return dict(depth=d, normal=n, conf=c, labels=labels, stats=stats)


COUNTERS = ("n_valid", "n_removed", "n_segments", "n_small", "largest")


def same_bits(a, b):
    """bit for bit, a NaN's payload included"""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))

"""Reference of hcmvs_estimate_point_normals (hc-mvs_amd/csrc/cloud_kernels.hip) in numpy: what the kernel documents, not how it
searches.

Neighbours: for point i the min(k, n) points with the smallest (d, original index), the point itself among them, d = dx*dx + dy*dy +
dz*dz in float64 from the float32 coordinates -- brute force over all pairs, no spatial structure of any kind.  PCA: centroid, 3 x 3
scatter about it, eigenvector of the smallest eigenvalue (numpy.linalg.eigh).  Orientation: tc = float32(centre of the point's first
view) - p and the dot product with the float32 normal, both in float32; negative flips (DepthMap.cpp:2262-2265).

Next to the normals come, per point, the reasons a point is not comparable with another implementation, each its own boolean array:
  near_tie         the k-th and the (k+1)-th squared distance differ, but by no more than 1e-9 of the larger: a compiler that contracts
                   the three-term sum into FMAs may order them the other way.  EQUAL distances are no exclusion: the index decides
  ill_conditioned  (l1 - l0) / l2 < 1e-4 for the eigenvalues l0 <= l1 <= l2 of the scatter: the smallest eigenvector is not determined
                   (l2 == 0, all neighbours in one place, counts as such)
  grazing          |n . tc| / |tc| < 1e-4 in float64: the sign of the float32 dot product is not determined"""
import numpy as np

NEAR_TIE_REL = 1e-9
ILL_CONDITIONED = 1e-4
GRAZING = 1e-4


def neighbour_table(xyz, kmax, rows=512):
    """the min(kmax + 1, n) nearest points of every point, ascending by (d, index): indices (n, m) int64 and squared distances
    (n, m) float64.  The first k columns are the neighbour set for any k <= kmax; column k is the first point left out."""
    X = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(X)
    m = min(kmax + 1, n)
    idx = np.empty((n, m), np.int64)
    dist = np.empty((n, m), np.float64)
    for r0 in range(0, n, rows):
        P = X[r0:r0 + rows]
        dx = P[:, None, 0] - X[None, :, 0]
        d = dx * dx
        dx = P[:, None, 1] - X[None, :, 1]
        d += dx * dx
        dx = P[:, None, 2] - X[None, :, 2]
        d += dx * dx
        # everything up to the m-th smallest distance of the row, its ties included; then the exact (d, index) order among those
        thr = np.partition(d, m - 1, axis=1)[:, m - 1]
        rr, cc = np.nonzero(d <= thr[:, None])
        dd = d[rr, cc]
        order = np.lexsort((cc, dd, rr))
        rr, cc, dd = rr[order], cc[order], dd[order]
        start = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=len(P)))[:-1]])
        take = start[:, None] + np.arange(m)[None, :]
        idx[r0:r0 + rows] = cc[take]
        dist[r0:r0 + rows] = dd[take]
    return idx, dist


def pca(xyz, nbr):
    """eigenvalues (n, 3) ascending and the eigenvector of the smallest (n, 3), float64, of the scatter of the points nbr (n, m)"""
    X = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    P = X[nbr]
    Pc = P - P.mean(1, keepdims=True)
    w, v = np.linalg.eigh(np.einsum("nki,nkj->nij", Pc, Pc))
    return w, v[:, :, 0].copy()


def orient(xyz, normal64, centres, first):
    """the flip towards the first view in float32, as the kernel does it; returns the float32 normal and the float64 cosine between
    the normal and the direction to the camera"""
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nn = normal64.astype(np.float32)
    tc = np.asarray(centres, np.float64)[first].astype(np.float32) - p
    dot = (nn[:, 0] * tc[:, 0] + nn[:, 1] * tc[:, 1]) + nn[:, 2] * tc[:, 2]
    assert tc.dtype == np.float32 and dot.dtype == np.float32
    nn[dot < 0] *= -1
    tc64 = tc.astype(np.float64)
    cosang = (normal64 * tc64).sum(1) / np.linalg.norm(tc64, axis=1)
    return nn, cosang


def reference(xyz, centres, first, k, table=None):
    """normal (n, 3) float32, the masks, and what they were computed from.  table: neighbour_table(xyz, kmax >= k) when the caller
    keeps one for several k"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    idx, dist = neighbour_table(xyz, k) if table is None else table
    m = min(k, n)
    assert idx.shape[1] >= min(k + 1, n)
    w, v = pca(xyz, idx[:, :m])
    normal, cosang = orient(xyz, v, centres, np.asarray(first, np.int64))
    if n > k:
        dk, dk1 = dist[:, k - 1], dist[:, k]
        near_tie = (dk1 != dk) & (dk1 - dk <= NEAR_TIE_REL * dk1)
    else:
        near_tie = np.zeros(n, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    return dict(normal=normal, normal64=v, eigenvalues=w, gap=gap, cosang=cosang, neighbours=idx[:, :m], near_tie=near_tie,
                ill_conditioned=gap < ILL_CONDITIONED, grazing=np.abs(cosang) < GRAZING)

"""The plane-prior rule (hcmvs_generate_plane_prior_device) stated in numpy, from the text of the rule alone:
brute-force neighbour search, numpy's eigen-solver, Python integers for the fixed-point sums, and for S4c a plain flood fill over a dict of
cells.  What the device must reproduce: every integer decision, the two averages, eps, the plane table and the prior map bit for bit; S2's
planarity up to the eigen-solver's rounding, for which `flags["S2"]` marks the samples whose decision a last-ulp difference could turn
(|p - planarity_min| < 1e-6).  tests/golden/plane_prior_statement.json holds what generate() returns, with S4c and without."""
import copy

import numpy as np

F32 = np.float32
M = 256                      # candidates of a round
MAX_PLANES = 64
SPACING_SHIFT, COORD_SHIFT = 40, 32
MASK = (1 << 64) - 1
CELL_CAP = 1 << 30           # S4c: the largest cell coordinate

DEFAULTS = dict(conf_max=0.18, planarity_min=0.3, n_neighbors=10, probability=0.01, min_points_div=80.0, epsilon_mul=2.0, normal_threshold=0.25,
                max_rounds=256, seed=1)


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(a, k):
    return float(mix64((a + k * 0xD1B54A32D192ED03) & MASK) >> 11) * 2.0 ** -53


def draw_below(a, k, n):
    return min(int(draw(a, k) * float(n)), n - 1)


def kinv(K):
    """the six entries of the inverse of a K whose last row is 0 0 1, in double, or None"""
    K = np.asarray(K, np.float64).reshape(9)
    if K[6] != 0 or K[7] != 0 or K[8] != 1:
        return None
    det = K[0] * K[4] - K[1] * K[3]
    if not (abs(det) > 0 and np.isfinite(det)):
        return None
    i = np.zeros(6)
    i[0] = K[4] / det; i[1] = -K[1] / det; i[3] = -K[3] / det; i[4] = K[0] / det
    i[2] = -(i[0] * K[2] + i[1] * K[5])
    i[5] = -(i[3] * K[2] + i[4] * K[5])
    return i if np.all(np.isfinite(i)) else None


def rays(K, w, h):
    i = kinv(K)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return np.stack([((i[0] * xs + i[1] * ys) + i[2]).astype(F32), ((i[3] * xs + i[4] * ys) + i[5]).astype(F32), np.ones((h, w), F32)], -1)


def levels(w, h):
    top = max(w, h) // 2
    out, l = [], 2
    while l <= top and len(out) < 16:
        out.append(l); l *= 2
    return out or [2]


def min_points(n0, div):
    return max(3, int(np.floor(float(n0) / float(F32(div)))))


def fail_limit(probability, minp, n0, max_rounds):
    share = float(minp) / float(n0)
    cands = 1.0
    if share < 1.0:
        cands = np.ceil(np.log(float(F32(probability))) / np.log(1.0 - share))
    rounds = np.ceil(cands / M)
    if not rounds >= 1.0:
        rounds = 1.0
    return int(min(rounds, float(max_rounds)))


def fixed_mean(values, n, shift, limit):
    """the mean of the doubles `values` as the device sums them: round(v * 2^shift) as integers, v saturated inside (-limit, limit)"""
    v = np.asarray(values, np.float64)
    v = np.where(v < limit, np.where(v > -limit, v, -(limit - 1.0)), limit - 1.0)
    q = np.rint(v * 2.0 ** shift).astype(np.int64)
    total = (int((q >> 32).sum()) << 32) + int((q & 0xffffffff).sum())
    return float(total) / (float(n) * 2.0 ** shift)


def nearest(pts, k, exclude_self, chunk=512):
    """(n, k) indices and squared distances of the k nearest by (squared distance in double, index), brute force"""
    P = pts.astype(np.float64)
    n = len(P)
    idx = np.empty((n, k), np.int64); dst = np.empty((n, k), np.float64)
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        dx = P[None, :, 0] - P[s:e, None, 0]; dy = P[None, :, 1] - P[s:e, None, 1]; dz = P[None, :, 2] - P[s:e, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        if exclude_self:
            d2[np.arange(e - s), np.arange(s, e)] = np.inf
        part = np.argpartition(d2, k - 1, axis=1)[:, :k]
        kth = np.take_along_axis(d2, part, 1).max(1)
        for r in range(e - s):
            c = np.nonzero(d2[r] <= kth[r])[0]            # ascending index: a stable sort breaks ties by index
            c = c[np.argsort(d2[r, c], kind="stable")][:k]
            idx[s + r] = c; dst[s + r] = d2[r, c]
    return idx, dst


def planarity(pts, k):
    nb, _ = nearest(pts, k, False)
    P = pts.astype(np.float64)
    mean = np.zeros((len(P), 3))
    for t in range(k):
        mean += P[nb[:, t]]
    mean /= float(k)
    cov = np.zeros((len(P), 3, 3))
    for t in range(k):
        d = P[nb[:, t]] - mean
        cov += d[:, :, None] * d[:, None, :]
    l = np.linalg.eigvalsh(cov)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(l[:, 2] > 0, (l[:, 1] - l[:, 0]) / l[:, 2], 0.0)


def spacing(pts, k):
    _, d2 = nearest(pts, k, True)
    s = np.zeros(len(pts))
    for t in range(k):
        s += np.sqrt(d2[:, t])
    return s / float(k)


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def frame(n):
    n = np.asarray(n, F32).astype(np.float64)
    k = 0
    if abs(n[1]) < abs(n[k]):
        k = 1
    if abs(n[2]) < abs(n[k]):
        k = 2
    a = [np.array([0.0, n[2], -n[1]]), np.array([-n[2], 0.0, n[0]]), np.array([n[1], -n[0], 0.0])][k]
    ln = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    b1 = a / ln
    b2 = np.array([n[1] * b1[2] - n[2] * b1[1], n[2] * b1[0] - n[0] * b1[2], n[0] * b1[1] - n[1] * b1[0]])
    return b1, b2


def quad(K, c, b1, b2, uv, box):
    """(quad (4, 2), fall-back flag)"""
    K = np.asarray(K, np.float64).reshape(9)
    us = [uv[0], uv[1], uv[1], uv[0]]; vs = [uv[2], uv[2], uv[3], uv[3]]
    q = np.zeros((4, 2)); ok = True
    for i in range(4):
        X = (c + us[i] * b1) + vs[i] * b2
        if not X[2] > 0:
            ok = False; break
        with np.errstate(all="ignore"):
            q[i, 0] = ((K[0] * X[0] + K[1] * X[1]) + K[2] * X[2]) / X[2]
            q[i, 1] = ((K[3] * X[0] + K[4] * X[1]) + K[5] * X[2]) / X[2]
        if not np.all(np.isfinite(q[i])):
            ok = False; break
    if ok:
        return q, 0
    x0, x1, y0, y1 = box[0] - 0.5, box[1] + 0.5, box[2] - 0.5, box[3] + 0.5
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64), 1


def fitting_set(depth, normal, conf, region, K, **params):
    """S1 .. S3, which do not depend on the seed: the state generate() continues from (pass it as generate(..., state=...))"""
    p = dict(DEFAULTS); p.update(params)
    depth = np.asarray(depth, F32); normal = np.asarray(normal, F32); conf = np.asarray(conf, F32); region = np.asarray(region, bool)
    h, w = depth.shape
    k = int(p["n_neighbors"])
    out = dict(prior=np.zeros((h, w), F32), prior_normal=np.zeros((h, w, 3), F32), planes=[], rounds=np.zeros((0, 6), np.int32),
               assignment=np.full((h, w), -1, np.int32), flags=dict(S2=np.zeros(0, bool)))
    st = dict(region_pixels=int(region.sum()), samples=0, planar_samples=0, fitting_samples=0, avg_spacing_all=0.0, avg_spacing=0.0, eps=F32(0), min_points=0,
              rounds=0, planes=0, candidates_valid=0, prior_pixels=0)
    out["stats"] = st
    stage = region.astype(np.uint8)
    out["stage"] = stage
    state = dict(out=out, fit=None, depth=depth, region=region, ray=rays(K, w, h), K=K)
    ray = state["ray"]
    # S1
    with np.errstate(invalid="ignore"):
        smp = region & np.isfinite(depth) & (depth > 0) & (conf < F32(p["conf_max"]))
    with np.errstate(all="ignore"):              # a point that is not finite in float32 is no sample
        smp &= np.isfinite((ray * np.where(smp, depth, F32(0))[..., None]).astype(F32)).all(-1)
    stage[smp] = 2
    pix = np.nonzero(smp.reshape(-1))[0]          # raster order
    st["samples"] = len(pix)
    if len(pix) < k + 1:
        return state
    P = (ray.reshape(-1, 3)[pix] * depth.reshape(-1)[pix][:, None]).astype(F32)
    N = normal.reshape(-1, 3)[pix]
    # S2
    pl = planarity(P, k)
    pmin = float(F32(p["planarity_min"]))
    out["flags"]["S2"] = np.abs(pl - pmin) < 1e-6
    keep = pl >= pmin
    pix, P, N = pix[keep], P[keep], N[keep]
    stage.reshape(-1)[pix] = 3
    st["planar_samples"] = len(pix)
    if len(pix) < k + 1:
        return state
    # S3
    s = spacing(P, k)
    avg_all = fixed_mean(s, len(s), SPACING_SHIFT, 8388608.0)
    st["avg_spacing_all"] = avg_all
    keep = ~(s > avg_all)
    pix, P, N = pix[keep], P[keep], N[keep]
    stage.reshape(-1)[pix] = 4
    n0 = len(pix)
    st["fitting_samples"] = n0
    if n0 < k + 1:
        return state
    st["avg_spacing"] = fixed_mean(spacing(P, k), n0, SPACING_SHIFT, 8388608.0)
    state["fit"] = (pix, P, N)
    return state


def cluster_cell(avg, mul):
    """float32(avg * float32(mul)) as a double"""
    with np.errstate(all="ignore"):
        return float(F32(float(avg) * float(F32(mul))))


def largest_component(P, n, cell):
    """S4c steps 2 .. 4 on the inliers P (m, 3) f32 of the plane with normal n: (indices into P of the winning component, occupied cells,
    components, its size)"""
    b1, b2 = frame(n)
    P64 = P.astype(np.float64)
    u = (P64[:, 0] * b1[0] + P64[:, 1] * b1[1]) + P64[:, 2] * b1[2]
    v = (P64[:, 0] * b2[0] + P64[:, 1] * b2[1]) + P64[:, 2] * b2[2]
    with np.errstate(all="ignore"):
        cu = np.minimum(np.floor((u - u.min()) / cell), float(CELL_CAP))
        cv = np.minimum(np.floor((v - v.min()) / cell), float(CELL_CAP))
    cells = {}
    for i in range(len(P)):
        cells.setdefault((int(cv[i]), int(cu[i])), []).append(i)
    label, comps = {}, []          # comps: (size, smallest (cv, cu) cell, members)
    for start in sorted(cells):     # ascending (cv, cu): a component is met at its smallest cell first
        if start in label:
            continue
        label[start] = len(comps)
        stack, members = [start], []
        while stack:
            c = stack.pop()
            members += cells[c]
            for dv in (-1, 0, 1):
                for du in (-1, 0, 1):
                    nb = (c[0] + dv, c[1] + du)
                    if nb in cells and nb not in label:
                        label[nb] = len(comps)
                        stack.append(nb)
        comps.append((len(members), start, members))
    best = None
    for size, start, members in comps:
        if best is None or size > best[0] or (size == best[0] and start < best[1]):
            best = (size, start, members)
    return np.array(sorted(best[2]), np.int64), len(cells), len(comps), best[0]


def generate(depth, normal, conf, region, K, state=None, cluster_mul=0.0, **params):
    """region: (h, w) bool.  Returns dict(prior, prior_normal, planes, stats, stage, assignment, rounds, clusters, flags).  state: what
    fitting_set returned for the same inputs and parameters (the stages before the plane detection do not depend on the seed).
    cluster_mul > 0 applies S4c to the winner of a round before anything is assigned.  clusters: 4 int32 per round (occupied cells,
    components, size of the largest component, accepted 0 / 1); without S4c a winner's row is 0, 0, its inliers, 1"""
    p = dict(DEFAULTS); p.update(params)
    if state is None:
        state = fitting_set(depth, normal, conf, region, K, **params)
    out = copy.deepcopy(state["out"])
    st = out["stats"]
    st.update(cluster_eps=F32(0), cluster_rejects=0, cluster_left=0)
    out["clusters"] = np.zeros((0, 4), np.int32)
    if state["fit"] is None:
        return out
    depth, region, ray, K = state["depth"], state["region"], state["ray"], state["K"]
    h, w = depth.shape
    pix, P, N = state["fit"]
    n0 = len(pix)
    thr = F32(p["normal_threshold"])
    avg = st["avg_spacing"]
    eps = F32(avg * float(F32(p["epsilon_mul"])))
    minp = min_points(n0, p["min_points_div"])
    st["eps"] = eps; st["min_points"] = minp
    clustering = float(F32(cluster_mul)) > 0
    cell = cluster_cell(avg, cluster_mul) if clustering else 0.0
    cell_ok = cell > 0 and np.isfinite(cell)
    st["cluster_eps"] = F32(cell)
    # S4
    lv = levels(w, h)
    sample_at = np.full(w * h, -1, np.int64); sample_at[pix] = np.arange(n0)
    assigned = np.full(n0, -1, np.int32)
    limit = fail_limit(p["probability"], minp, n0, p["max_rounds"])
    eps_k = [eps, eps * F32(0.5), eps * F32(0.25), eps * F32(0.125)]
    found, rounds, clusters, fails, unassigned, seed = [], [], [], 0, n0, int(p["seed"]) & MASK
    Px, Py, Pz, Nx, Ny, Nz = P[:, 0], P[:, 1], P[:, 2], N[:, 0], N[:, 1], N[:, 2]
    while unassigned >= minp and len(found) < MAX_PLANES and len(rounds) < int(p["max_rounds"]) and fails < limit:
        r = len(rounds)
        cands = {}
        for c in range(M):
            a = mix64(seed ^ mix64(r * M + c))
            ia = draw_below(a, 0, n0)
            rho = lv[draw_below(a, 1, len(lv))]
            off = [draw_below(a, 2 + q, 2 * rho + 1) - rho for q in range(4)]
            ax, ay = int(pix[ia]) % w, int(pix[ia]) // w
            bx, by, cx, cy = ax + off[0], ay + off[1], ax + off[2], ay + off[3]
            if assigned[ia] >= 0 or not (0 <= bx < w and 0 <= by < h and 0 <= cx < w and 0 <= cy < h):
                continue
            ib, ic = int(sample_at[by * w + bx]), int(sample_at[cy * w + cx])
            if ib < 0 or ic < 0 or ib == ia or ic == ia or ib == ic or assigned[ib] >= 0 or assigned[ic] >= 0:
                continue
            A, B, Cc = P[ia], P[ib], P[ic]
            u, v = B - A, Cc - A
            with np.errstate(all="ignore"):
                nx = u[1] * v[2] - u[2] * v[1]; ny = u[2] * v[0] - u[0] * v[2]; nz = u[0] * v[1] - u[1] * v[0]
                ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
                if not (ln > 0 and np.isfinite(ln)):
                    continue
                nx, ny, nz = nx / ln, ny / ln, nz / ln
                d = dot3(nx, ny, nz, A[0], A[1], A[2])
                if not np.isfinite(d):
                    continue
                if not all(abs(dot3(nx, ny, nz, N[i][0], N[i][1], N[i][2])) >= thr for i in (ia, ib, ic)):
                    continue
            assert all(type(t) is F32 for t in (nx, ny, nz, d))
            cands[c] = (nx, ny, nz, d)
        best, best_key, best_counts = -1, None, (0, 0, 0, 0)
        free = assigned < 0
        for c in sorted(cands):
            nx, ny, nz, d = cands[c]
            with np.errstate(invalid="ignore"):
                facing = free & (np.abs(dot3(nx, ny, nz, Nx, Ny, Nz)) >= thr)
                res = np.abs(dot3(nx, ny, nz, Px, Py, Pz) - d)
                cnt = tuple(int((facing & (res <= e)).sum()) for e in eps_k)
            if cnt[0] >= minp and (best_key is None or sum(cnt) > best_key):
                best, best_key, best_counts = c, sum(cnt), cnt
        rounds.append([best, *best_counts, len(cands)])
        st["candidates_valid"] += len(cands)
        if best >= 0:
            nx, ny, nz, d = cands[best]
            with np.errstate(invalid="ignore"):
                inl = free & (np.abs(dot3(nx, ny, nz, Nx, Ny, Nz)) >= thr) & (np.abs(dot3(nx, ny, nz, Px, Py, Pz) - d) <= eps)
            take = np.nonzero(inl)[0]
            assert len(take) == best_counts[0]
            size, row = best_counts[0], [0, 1 if clustering else 0, best_counts[0], 1]
            if clustering and cell_ok:                                            # S4c
                keep, n_cells, n_comps, size = largest_component(P[take], np.array([nx, ny, nz], F32), cell)
                take = take[keep]
                row = [n_cells, n_comps, size, int(size >= minp)]
            clusters.append(row)
            if row[3]:
                assigned[take] = len(found)
                found.append((np.array([nx, ny, nz], F32), size))
                unassigned -= size
                st["cluster_left"] += best_counts[0] - size
                fails = 0
            else:
                st["cluster_rejects"] += 1
                fails += 1
        else:
            clusters.append([0, 0, 0, 0])
            fails += 1
    out["rounds"] = np.array(rounds, np.int32).reshape(-1, 6)
    out["clusters"] = np.array(clusters, np.int32).reshape(-1, 4)
    out["assignment"].reshape(-1)[pix] = assigned
    st["rounds"] = len(rounds); st["planes"] = len(found)
    if not found:
        return out
    # S5
    P64 = P.astype(np.float64)
    table = []
    for i, (n, cnt0) in enumerate(found):
        m = assigned == i
        c = np.array([fixed_mean(P64[m, q], int(m.sum()), COORD_SHIFT, 1073741824.0) for q in range(3)])
        b1, b2 = frame(n)
        d = P64[m] - c
        u = (d[:, 0] * b1[0] + d[:, 1] * b1[1]) + d[:, 2] * b1[2]
        v = (d[:, 0] * b2[0] + d[:, 1] * b2[1]) + d[:, 2] * b2[2]
        xs, ys = pix[m] % w, pix[m] // w
        q, fb = quad(K, c, b1, b2, [u.min(), u.max(), v.min(), v.max()], [xs.min(), xs.max(), ys.min(), ys.max()])
        n64 = n.astype(np.float64)
        table.append(dict(normal=n, n_inliers=cnt0, centre=c, quad=q, box_fallback=fb, nc=(n64[0] * c[0] + n64[1] * c[1]) + n64[2] * c[2]))
    out["planes"] = table
    # S6
    ys, xs = np.nonzero(region)
    r = ray[ys, xs].astype(np.float64)
    d = depth[ys, xs]
    with np.errstate(invalid="ignore"):
        has = np.isfinite(d) & (d > 0)
    with np.errstate(all="ignore"):
        has &= np.isfinite((ray[ys, xs] * np.where(has, d, F32(0))[:, None]).astype(F32)).all(-1)
    X = np.where(has[:, None], (ray[ys, xs] * np.where(has, d, F32(0))[:, None]).astype(F32), F32(0)).astype(np.float64)
    best = np.full(len(xs), -1); best_dist = np.zeros(len(xs))
    fx, fy = xs.astype(np.float64), ys.astype(np.float64)
    for i, t in enumerate(table):
        q = t["quad"]
        pos = np.zeros(len(xs), int); neg = np.zeros(len(xs), int)
        for e in range(4):
            a, b = q[e], q[(e + 1) & 3]
            cr = (b[0] - a[0]) * (fy - a[1]) - (b[1] - a[1]) * (fx - a[0])
            pos += cr > 0; neg += cr < 0
        inside = (pos == 4) | (neg == 4)
        n64 = t["normal"].astype(np.float64)
        dist = np.abs(((n64[0] * X[:, 0] + n64[1] * X[:, 1]) + n64[2] * X[:, 2]) - t["nc"])
        take = inside & ((best < 0) | (dist < best_dist))
        best[take] = i; best_dist[take] = dist[take]
    for i, t in enumerate(table):
        m = best == i
        n64 = t["normal"].astype(np.float64)
        den = (n64[0] * r[m, 0] + n64[1] * r[m, 1]) + n64[2] * r[m, 2]
        with np.errstate(all="ignore"):
            v = (t["nc"] / den).astype(F32)
            good = np.isfinite(v) & (v > 0)
        out["prior"][ys[m], xs[m]] = np.where(good, v, F32(0))
        sg = np.where(den > 0, F32(-1), F32(1))
        out["prior_normal"][ys[m], xs[m]] = np.where(good[:, None], sg[:, None] * t["normal"][None, :], F32(0))
    st["prior_pixels"] = int((out["prior"] > 0).sum())
    return out

"""The plane-prior rule with the clustering of a plane's inliers into connected components stated in numpy:
S4 .. S6 of tests/plane_prior_ref.py, whose helpers and fitting_set (S1 .. S3) are reused, with S4c applied to the winner of a round before
anything is assigned.  The components are a plain flood fill over a dict of cells, in Python integers.  With cluster_mul = 0 generate() is
plane_prior_ref.generate() bit for bit (tests/test_plane_prior_cluster_ref.py pins the copy); it returns `clusters` (4 int32 per round:
occupied cells, components, size of the largest component, accepted 0 / 1) and the stats cluster_eps, cluster_rejects, cluster_left on top."""
import copy

import numpy as np

import plane_prior_ref as ref
from plane_prior_ref import F32, M, MAX_PLANES, MASK, COORD_SHIFT, mix64, draw_below, dot3, frame, quad, levels, min_points, fail_limit, fixed_mean, fitting_set

CELL_CAP = 1 << 30


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
    """plane_prior_ref.generate with S4c.  Returns what it returns plus clusters (rounds, 4) i32 and three more stats"""
    p = dict(ref.DEFAULTS); p.update(params)
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

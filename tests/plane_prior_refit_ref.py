"""The plane-prior rule with the least-squares refit of a round's winner stated in numpy and plain Python.
S1 .. S3 and the helpers are those of tests/plane_prior_ref.py; S4 is restated here with S4r and S4c, then S5 and S6.  The moment sums of
S4r are Python integers, the eigen-solver is the cyclic Jacobi iteration of D13 written operation by operation in Python floats (IEEE
doubles, every operation rounded on its own).  With refit_iters = 0 generate() returns what plane_prior_ref.generate returns.  What the
device must reproduce: all of it, bit for bit.  tests/golden/plane_prior_refit_statement.json holds what generate() returns."""
import copy
import math

import numpy as np

import plane_prior_ref as ref
from plane_prior_ref import F32, M, MASK, MAX_PLANES, COORD_SHIFT, dot3, draw_below, mix64

MAX_REFIT_ITERS = 16
FIRST_SHIFT, SECOND_SHIFT = 24, 20     # a first moment is summed as rint(s * 2^24), a second as rint((s_a * s_b) * 2^20)
MOMENT_LIMIT = 1048576.0               # s is saturated inside (-2^20, 2^20)
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
STOPS = ("iters", "band", "degenerate", "fixed", "count")


def refit_scale(eps):
    """E of eps = f * 2^E, f in [0.5, 1); 0 for an eps that is not a finite number > 0"""
    e = float(F32(eps))
    if not (e > 0 and math.isfinite(e)):
        return 0
    return math.frexp(e)[1]


def moment_sums(P, O, E):
    """the nine sums of the band's samples P (m, 3) f32 about the anchor O (3 doubles) as Python integers: x y z, xx xy xz yy yz zz"""
    s = (P.astype(np.float64) - np.asarray(O, np.float64)[None, :]) * 2.0 ** -E
    s = np.where(s < MOMENT_LIMIT, np.where(s > -MOMENT_LIMIT, s, -(MOMENT_LIMIT - 1.0)), MOMENT_LIMIT - 1.0)
    out = []                            # (every addend is below 2^60 in magnitude: int64 holds it, Python adds them)
    for a in range(3):
        out.append(sum(np.rint(s[:, a] * 2.0 ** FIRST_SHIFT).astype(np.int64).tolist()))
    for a, b in PAIRS:
        out.append(sum(np.rint((s[:, a] * s[:, b]) * 2.0 ** SECOND_SHIFT).astype(np.int64).tolist()))
    return out


def split_words(total):
    """an integer sum as the device returns it: the sum of the high parts q >> 32 and of the low parts q & 0xffffffff.  Any split with
    hi * 2^32 + lo = total decodes to the same mean; this is the canonical one"""
    return total >> 32, total & 0xffffffff


def mean_of(total, n, shift):
    return float(total) / (float(n) * 2.0 ** shift)


def covariance(sums, m):
    """(mu (3), C as the six values 00 01 02 11 12 22) from the nine integer sums of m samples"""
    mu = [mean_of(sums[a], m, FIRST_SHIFT) for a in range(3)]
    C = [mean_of(sums[3 + i], m, SECOND_SHIFT) - mu[a] * mu[b] for i, (a, b) in enumerate(PAIRS)]
    return mu, C


def jacobi_smallest(C):
    """the eigenvector (3 Python floats, not normalised beyond what the rotations keep) of the smallest eigenvalue of the symmetric matrix
    C = (c00 c01 c02 c11 c12 c22), and the sweeps used: cyclic Jacobi, pairs (0,1) (0,2) (1,2), at most 16 sweeps"""
    C = [float(v) for v in C]
    a = [[C[0], C[1], C[2]], [C[1], C[3], C[4]], [C[2], C[4], C[5]]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    sweeps = 0
    while sweeps < 16 and not (a[0][1] == 0.0 and a[0][2] == 0.0 and a[1][2] == 0.0):
        sweeps += 1
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            r = 3 - p - q
            a[p][p] = a[p][p] - t * apq
            a[q][q] = a[q][q] + t * apq
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for k in range(3):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = c * vkp - s * vkq
                v[k][q] = s * vkp + c * vkq
    k = 0
    if a[1][1] < a[k][k]:
        k = 1
    if a[2][2] < a[k][k]:
        k = 2
    return [v[0][k], v[1][k], v[2][k]], sweeps


def refit_solve(sums, m, O, E, prev):
    """step 4 of S4r: the plane (nx, ny, nz, d) as four float32 from the nine sums of the m band samples, the anchor O, the scale E and
    the previous plane `prev`; None when the length is zero or not finite or d is not finite"""
    mu, C = covariance(sums, m)
    vec, _ = jacobi_smallest(C)
    with np.errstate(all="ignore"):
        x, y, z = F32(vec[0]), F32(vec[1]), F32(vec[2])
        ln = np.sqrt((x * x + y * y) + z * z)
        if not (ln > 0 and np.isfinite(ln)):
            return None
        x, y, z = x / ln, y / ln, z / ln
        if dot3(x, y, z, prev[0], prev[1], prev[2]) < 0:
            x, y, z = -x, -y, -z
        c = [float(O[a]) + mu[a] * 2.0 ** E for a in range(3)]
        d = F32((float(x) * c[0] + float(y) * c[1]) + float(z) * c[2])
    if not np.isfinite(d):
        return None
    assert all(type(t) is F32 for t in (x, y, z, d))
    return (x, y, z, d)


def same_bits(a, b):
    return np.array(a, F32).tobytes() == np.array(b, F32).tobytes()


def generate(depth, normal, conf, region, K, state=None, cluster_mul=0.0, refit_iters=0, **params):
    """plane_prior_ref.generate with S4r: `refit_iters` least-squares steps on the winner of a round before S4c and before anything is
    assigned.  On top of what plane_prior_ref.generate returns: refits (n, 6) int32 per round -- steps solved, steps kept, the final plane's
    cnt_0 .. cnt_3 --, refit_planes (n, 4) float32 per round -- the final n, d --, both all zeros for a round without a winner;
    refit_stops, per round the reason the steps ended (one of STOPS, None without a winner or with refit_iters = 0); refit_cov, of every
    step solved dict(m, sums (nine integers), O, E, prev, plane); stats refit_rounds and refit_steps"""
    p = dict(ref.DEFAULTS); p.update(params)
    R = int(refit_iters)
    assert 0 <= R <= MAX_REFIT_ITERS
    if state is None:
        state = ref.fitting_set(depth, normal, conf, region, K, **params)
    out = copy.deepcopy(state["out"])
    st = out["stats"]
    st.update(cluster_eps=F32(0), cluster_rejects=0, cluster_left=0, refit_rounds=0, refit_steps=0)
    out["clusters"] = np.zeros((0, 4), np.int32)
    out["refits"] = np.zeros((0, 6), np.int32); out["refit_planes"] = np.zeros((0, 4), F32); out["refit_stops"] = []; out["refit_cov"] = []
    if state["fit"] is None:
        return out
    depth, region, ray, K = state["depth"], state["region"], state["ray"], state["K"]
    h, w = depth.shape
    pix, P, N = state["fit"]
    n0 = len(pix)
    thr = F32(p["normal_threshold"])
    avg = st["avg_spacing"]
    eps = F32(avg * float(F32(p["epsilon_mul"])))
    minp = ref.min_points(n0, p["min_points_div"])
    st["eps"] = eps; st["min_points"] = minp
    clustering = float(F32(cluster_mul)) > 0
    cell = ref.cluster_cell(avg, cluster_mul) if clustering else 0.0
    cell_ok = cell > 0 and np.isfinite(cell)
    st["cluster_eps"] = F32(cell)
    E = refit_scale(eps)
    # S4
    lv = ref.levels(w, h)
    sample_at = np.full(w * h, -1, np.int64); sample_at[pix] = np.arange(n0)
    assigned = np.full(n0, -1, np.int32)
    limit = ref.fail_limit(p["probability"], minp, n0, p["max_rounds"])
    eps_k = [eps, eps * F32(0.5), eps * F32(0.25), eps * F32(0.125)]
    found, rounds, clusters, refits, refit_planes, fails, unassigned, seed = [], [], [], [], [], 0, n0, int(p["seed"]) & MASK
    Px, Py, Pz, Nx, Ny, Nz = P[:, 0], P[:, 1], P[:, 2], N[:, 0], N[:, 1], N[:, 2]

    def facing_and_residual(pl, free):
        with np.errstate(invalid="ignore"):
            return free & (np.abs(dot3(pl[0], pl[1], pl[2], Nx, Ny, Nz)) >= thr), np.abs(dot3(pl[0], pl[1], pl[2], Px, Py, Pz) - pl[3])

    def counts_of(pl, free):
        facing, res = facing_and_residual(pl, free)
        with np.errstate(invalid="ignore"):
            return tuple(int((facing & (res <= e)).sum()) for e in eps_k)

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
            cnt = counts_of(cands[c], free)
            if cnt[0] >= minp and (best_key is None or sum(cnt) > best_key):
                best, best_key, best_counts = c, sum(cnt), cnt
        rounds.append([best, *best_counts, len(cands)])
        st["candidates_valid"] += len(cands)
        if best < 0:
            clusters.append([0, 0, 0, 0]); refits.append([0] * 6); refit_planes.append([F32(0)] * 4); out["refit_stops"].append(None)
            fails += 1
            continue
        plane, cnt = cands[best], best_counts
        # S4r
        solved = kept = 0
        stop = None
        if R > 0:
            ia = draw_below(mix64(seed ^ mix64(r * M + best)), 0, n0)
            O = [float(P[ia][a]) for a in range(3)]
            stop = "iters"
            for t in range(1, R + 1):
                facing, res = facing_and_residual(plane, free)
                with np.errstate(invalid="ignore"):
                    band = np.nonzero(facing & (res <= eps_k[2]))[0]
                m = len(band)
                assert m == cnt[2]
                if m < 3:
                    stop = "band"; break
                sums = moment_sums(P[band], O, E)
                trial = refit_solve(sums, m, O, E, plane)
                if trial is None:
                    stop = "degenerate"; break
                solved += 1
                out["refit_cov"].append(dict(m=m, sums=sums, O=O, E=E, prev=plane, plane=trial))
                if same_bits(trial, plane):
                    stop = "fixed"; break
                tc = counts_of(trial, free)
                if tc[0] < minp:
                    stop = "count"; break
                plane, cnt = trial, tc
                kept += 1
            if kept:
                st["refit_rounds"] += 1; st["refit_steps"] += kept
        refits.append([solved, kept, *cnt]); refit_planes.append(list(plane)); out["refit_stops"].append(stop)
        nx, ny, nz, d = plane
        facing, res = facing_and_residual(plane, free)
        with np.errstate(invalid="ignore"):
            take = np.nonzero(facing & (res <= eps))[0]
        assert len(take) == cnt[0]
        size, row = cnt[0], [0, 1 if clustering else 0, cnt[0], 1]
        if clustering and cell_ok:                                            # S4c
            keep, n_cells, n_comps, size = ref.largest_component(P[take], np.array([nx, ny, nz], F32), cell)
            take = take[keep]
            row = [n_cells, n_comps, size, int(size >= minp)]
        clusters.append(row)
        if row[3]:
            assigned[take] = len(found)
            found.append((np.array([nx, ny, nz], F32), size))
            unassigned -= size
            st["cluster_left"] += cnt[0] - size
            fails = 0
        else:
            st["cluster_rejects"] += 1
            fails += 1
    out["rounds"] = np.array(rounds, np.int32).reshape(-1, 6)
    out["clusters"] = np.array(clusters, np.int32).reshape(-1, 4)
    out["refits"] = np.array(refits, np.int32).reshape(-1, 6)
    out["refit_planes"] = np.array(refit_planes, F32).reshape(-1, 4)
    out["assignment"].reshape(-1)[pix] = assigned
    st["rounds"] = len(rounds); st["planes"] = len(found)
    if not found:
        return out
    # S5
    P64 = P.astype(np.float64)
    table = []
    for i, (n, cnt0) in enumerate(found):
        m = assigned == i
        c = np.array([ref.fixed_mean(P64[m, q], int(m.sum()), COORD_SHIFT, 1073741824.0) for q in range(3)])
        b1, b2 = ref.frame(n)
        d = P64[m] - c
        u = (d[:, 0] * b1[0] + d[:, 1] * b1[1]) + d[:, 2] * b1[2]
        v = (d[:, 0] * b2[0] + d[:, 1] * b2[1]) + d[:, 2] * b2[2]
        xs, ys = pix[m] % w, pix[m] // w
        q, fb = ref.quad(K, c, b1, b2, [u.min(), u.max(), v.min(), v.max()], [xs.min(), xs.max(), ys.min(), ys.max()])
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

"""Restatement of the point-cloud kernels (csrc/pointcloud.hip, csrc/pc_grid.h) in plain numpy float64 -- test infrastructure, brute
force over all pairs, no GPU, no KD-tree.  Every function states the rule its kernel implements IN THE KERNEL'S OPERATION ORDER (the
library is built with -ffp-contract=off, so `a * b + c` is two roundings on both sides), hence most comparisons are bit for bit; written
from the kernels' own comments.  Sequential sums are `np.cumsum(...)[-1]` (numpy's `sum` adds pairwise, the kernels do not).

The tie rule of the hybrid radius / max_nn selection, written down because it is easy to get wrong: the in-radius candidates
(d^2 < r^2, strict) are ordered by (d^2, POSITION IN THE GRID'S SORTED ORDER) and the first max_nn are kept.  Not (d^2, original index):
the kernel walks the cells in key order and a tie keeps the point it visited first."""
import math

import numpy as np

KEY_MAX = (1 << 21) - 1
K_NRM_CAND, K_KNN_CAND, K_MAX_NN, K_MAX_BATCH = 224, 448, 64, 16
SORT_LDS_MAX, SORT_RUNS = 16384, 64
SETTLE = 1.0 - 1e-12
U53 = 2.0 ** -53


# ---- surface points ---------------------------------------------------------------------------------------------------------------------
def surface_points(label, depth, intr, T):
    """pixels with label != 0 and depth != 0 in raster order; p0 = (px - ppx) d / fx; row r = ((T0 p0 + T1 p1) + T2 d) + T3"""
    label, depth = np.asarray(label), np.asarray(depth)
    W = label.shape[1]
    pix = np.flatnonzero((label.reshape(-1) != 0) & (depth.reshape(-1) != 0))
    py, px = pix // W, pix % W
    d = depth.reshape(-1)[pix].astype(np.float64)
    p0 = (px.astype(np.float64) - intr["ppx"]) * d / intr["fx"]
    p1 = (py.astype(np.float64) - intr["ppy"]) * d / intr["fy"]
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    return np.stack([((T[r, 0] * p0 + T[r, 1] * p1) + T[r, 2] * d) + T[r, 3] for r in range(3)], 1).reshape(-1, 3)


# ---- grid ---------------------------------------------------------------------------------------------------------------------------------
def cell_coords(pts, origin, cell):
    """(pre-floor coordinate, clamped cell) of every point"""
    pre = (np.asarray(pts, dtype=np.float64).reshape(-1, 3) - origin) / cell
    return pre, np.clip(np.floor(pre), 0, KEY_MAX).astype(np.int64)


def pack(c):
    return ((c[..., 0].astype(np.uint64) << np.uint64(42)) | (c[..., 1].astype(np.uint64) << np.uint64(21)) | c[..., 2].astype(np.uint64))


def grid(pts, cell, shift):
    """origin = min - shift, cell = floor((p - origin) / cell) clamped to [0, 2^21), key = cx << 42 | cy << 21 | cz, stable argsort"""
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    origin = pts.min(0) - shift
    pre, c = cell_coords(pts, origin, cell)
    keys = pack(c)
    order = np.argsort(keys, kind="stable")
    return dict(pts=pts, origin=origin, keys=keys[order], order=order.astype(np.uint32), sorted=pts[order], cells=c[order], pre=pre, cell=float(cell),
                n=len(pts), hi=pts.max(0), lo=pts.min(0), shift=float(shift))


def sort_form(g):
    """which form of the hand-written sort a grid takes: (runs, index bits, cells per axis, rank bits, compact?) -- the predicate of
    seg_sort_batch: at most 64 runs of 16384 and dim0 * dim1 * dim2 <= 2^(63 - index bits), the product taken in float64"""
    n = g["n"]
    runs = (n + SORT_LDS_MAX - 1) // SORT_LDS_MAX
    ib = 1
    while (1 << ib) < n:
        ib += 1
    dim = [int(np.clip(math.floor((g["hi"][d] - (g["lo"][d] - g["shift"])) / g["cell"]), 0, KEY_MAX)) + 1 for d in range(3)]
    prod = float(dim[0]) * float(dim[1]) * float(dim[2])
    compact = runs <= SORT_RUNS and prod <= float(1 << (63 - ib))
    cells = dim[0] * dim[1] * dim[2]
    return dict(runs=runs, index_bits=ib, dim=dim, rank_bits=(cells - 1).bit_length() if cells > 1 else 0, compact=compact)


def voxel_down_sample(pts, voxel):
    """shift = voxel / 2; per-voxel sum in stable (original-index) order, accumulated sequentially, divided by the count; voxels in key order"""
    g = grid(pts, voxel, voxel * 0.5)
    if g["n"] == 0:
        return np.zeros((0, 3))
    first = np.flatnonzero(np.r_[True, g["keys"][1:] != g["keys"][:-1]])
    last = np.r_[first[1:], g["n"]]
    out = np.empty((len(first), 3))
    single = last - first == 1
    out[single] = g["sorted"][first[single]] / 1.0
    for i in np.flatnonzero(~single):
        out[i] = np.cumsum(g["sorted"][first[i]:last[i]], axis=0)[-1] / float(last[i] - first[i])
    return out


def d2_to(points, q):
    e = points - q
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def radius_count(g, q, r):
    """number of grid points with (ex^2 + ey^2) + ez^2 < r^2 (self and duplicates included); r <= cell"""
    r2 = r * r
    return np.array([int((d2_to(g["sorted"], p) < r2).sum()) for p in np.asarray(q, dtype=np.float64).reshape(-1, 3)], dtype=np.int32)


# ---- normals ------------------------------------------------------------------------------------------------------------------------------
def hybrid_selection(g, q, r, max_nn, rule="kernel"):
    """sorted positions of the selection of query q.  rule = "kernel": candidates d^2 < r^2 ordered by (d^2, sorted position), first
    max_nn.  The other rules are the WRONG ones the host test prices: "high" ties to the highest position, "inclusive" d^2 <= r^2,
    "original" ordering by (d^2, original index)"""
    d2 = d2_to(g["sorted"], q)
    cand = np.flatnonzero(d2 <= r * r if rule == "inclusive" else d2 < r * r)
    tie = {"kernel": cand, "inclusive": cand, "high": -cand, "original": g["order"][cand].astype(np.int64)}[rule]
    return cand[np.lexsort((tie, d2[cand]))][:max_nn]


def covariance(g, sel):
    """(cnt, mean, C): mean and covariance accumulated in selection order, each divided by cnt"""
    p = g["sorted"][sel]
    cnt = len(sel)
    mu = np.cumsum(p, axis=0)[-1] / float(cnt)
    e = p - mu
    C = np.cumsum(e[:, :, None] * e[:, None, :], axis=0)[-1] / float(cnt)
    return cnt, mu, C


def normal(g, sel):
    """(0, 0, 1) when cnt < 3, else the eigenvector of the smallest eigenvalue (np.linalg.eigh), flipped towards +z"""
    if len(sel) < 3:
        return np.array([0.0, 0.0, 1.0])
    _, _, C = covariance(g, sel)
    v = np.linalg.eigh(C)[1][:, 0]
    return -v if v[2] < 0 else v


# ---- k-NN mean ----------------------------------------------------------------------------------------------------------------------------
def pair_d2(pts):
    e = pts[None, :, :] - pts[:, None, :]
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def knn_mean(pts, k):
    """the k smallest d^2 (self included), sqrt of each, summed sequentially in ascending order, divided by k"""
    d2 = np.sort(pair_d2(np.asarray(pts, dtype=np.float64)), axis=1)[:, :k]
    return np.cumsum(np.sqrt(d2), axis=1)[:, -1] / float(k)


def knn_route(g, k):
    """per point in the grid's sorted order: (route, margin).  route = 1, 2, 3 (the (2R+1)^3 block that settles), "overflow" (a block of
    more than 448 candidates) or "all" (unsettled: the all-points loop).  The kernel's predicates: block count against k and 448, settle
    test d_k^2 < (R cell)^2 (1 - 1e-12).  margin = the smallest relative distance of a settle comparison it made from its bound."""
    out = []
    cells, pts, h = g["cells"], g["sorted"], g["cell"]
    for i in range(g["n"]):
        d2 = d2_to(pts, pts[i])
        cheb = np.abs(cells - cells[i]).max(1)
        route, margin = "all", np.inf
        for R in (1, 2, 3):
            inb = cheb <= R
            nc = int(inb.sum())
            if nc > K_KNN_CAND:
                route = "overflow"
                break
            if nc < k:
                continue
            dk = np.sort(d2[inb])[k - 1]
            bound = (R * h) * (R * h) * SETTLE
            margin = min(margin, abs(dk - bound) / bound)
            if dk < bound:
                route = R
                break
        out.append((route, margin))
    return out


# ---- ICP correspondence search ----------------------------------------------------------------------------------------------------------------
def nn1(g, q, max_dist):
    """nearest grid point with d^2 < max_dist^2 as (original index, d^2); ties -> lowest original index; (-1, 0) when there is none"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    idx, dist = np.full(len(q), -1, np.int32), np.zeros(len(q))
    for i, p in enumerate(q):
        d2 = d2_to(g["sorted"], p)
        ok = np.flatnonzero(d2 < max_dist * max_dist)
        if len(ok):
            best = ok[d2[ok] == d2[ok].min()]
            idx[i], dist[i] = int(g["order"][best].min()), d2[best[0]]
    return idx, dist


# ---- selection and the statistical threshold ------------------------------------------------------------------------------------------------
def select(mode, values, thr):
    """kept row indices: mode 0 count > thr, mode 1 mean > 0 and mean < thr"""
    v = np.asarray(values)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(v > thr if mode == 0 else (v > 0.0) & (v < thr))


def statistical_threshold(means, std_ratio):
    """batched.remove_statistical_outlier on the host: valid means are m >= 0, sample std with max(valid - 1, 1)"""
    m = np.asarray(means, dtype=np.float64)
    valid = m >= 0
    nv = int(valid.sum())
    cloud_mean = m[valid].sum() / max(nv, 1)
    std = math.sqrt(((m[valid] - cloud_mean) ** 2).sum() / max(nv - 1, 1))
    return cloud_mean + float(std_ratio) * std


def mahalanobis(pts, mc12):
    """s += e[a] ((C[a][0] e0 + C[a][1] e1) + C[a][2] e2) for a = 0, 1, 2, then sqrt(s);  mc12 = (mu[3], Cinv[9])"""
    mc12 = np.asarray(mc12, dtype=np.float64)
    e = np.asarray(pts, dtype=np.float64).reshape(-1, 3) - mc12[:3]
    C = mc12[3:].reshape(3, 3)
    s = np.zeros(len(e))
    with np.errstate(invalid="ignore"):
        for a in range(3):
            s = s + e[:, a] * ((C[a, 0] * e[:, 0] + C[a, 1] * e[:, 1]) + C[a, 2] * e[:, 2])
        return np.sqrt(s)


def transform(pts, T, normals=None):
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)
    if normals is None:
        return out
    a, b, c = normals[:, 0], normals[:, 1], normals[:, 2]
    return out, np.stack([(T[r, 0] * a + T[r, 1] * b) + T[r, 2] * c for r in range(3)], 1)


# ---- exact sums ----------------------------------------------------------------------------------------------------------------------------
def _exact(terms):
    """(math.fsum of every column, its bound n 2^-53 sum|term| + 2^-53 sum|term|): any summation order of n terms is within
    (n - 1) u sum|term| of the exact sum to first order, and the products inside the terms carry one rounding each"""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[0]
    tot = np.array([math.fsum(terms[:, v]) for v in range(terms.shape[1])])
    mag = np.array([math.fsum(np.abs(terms[:, v])) for v in range(terms.shape[1])])
    return tot, (n + 1) * U53 * mag


def moments_exact(pts):
    """the 9 moments: sum p[3], upper triangle of sum p_a p_b"""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    return _exact(np.stack([p[:, 0], p[:, 1], p[:, 2], p[:, 0] * p[:, 0], p[:, 0] * p[:, 1], p[:, 0] * p[:, 2], p[:, 1] * p[:, 1],
                            p[:, 1] * p[:, 2], p[:, 2] * p[:, 2]], 1))


def p2p_terms(src, tgt, corr, d2):
    ok = corr >= 0
    s, t = src[ok], tgt[corr[ok]]
    return np.concatenate([np.ones((len(s), 1)), d2[ok][:, None], s, t, (s[:, :, None] * t[:, None, :]).reshape(-1, 9)], 1)


def p2plane_terms(src, tgt, tn, corr, d2):
    ok = corr >= 0
    s, t, n = src[ok], tgt[corr[ok]], tn[corr[ok]]
    r = ((s[:, 0] - t[:, 0]) * n[:, 0] + (s[:, 1] - t[:, 1]) * n[:, 1]) + (s[:, 2] - t[:, 2]) * n[:, 2]
    J = np.stack([s[:, 1] * n[:, 2] - s[:, 2] * n[:, 1], s[:, 2] * n[:, 0] - s[:, 0] * n[:, 2], s[:, 0] * n[:, 1] - s[:, 1] * n[:, 0],
                  n[:, 0], n[:, 1], n[:, 2]], 1)
    cols = [np.ones(len(s)), d2[ok]] + [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)] + [J[:, a] * r for a in range(6)]
    return np.stack(cols, 1)


def icp_sums_exact(kind, src, tgt, tn, corr, d2):
    """(sums, bound): the 17 point-to-point / 29 point-to-plane sums; the terms are formed in the kernel's operation order"""
    terms = p2p_terms(src, tgt, corr, d2) if kind == 0 else p2plane_terms(src, tgt, tn, corr, d2)
    if len(terms) == 0:
        return np.zeros(17 if kind == 0 else 29), np.zeros(17 if kind == 0 else 29)
    tot, bound = _exact(terms)
    return tot, bound


# ---- the ICP step ---------------------------------------------------------------------------------------------------------------------------
def solve6(M):
    """Gaussian elimination with partial pivoting on the augmented 6x7 system, as the kernel; None when a pivot is exactly 0"""
    M = np.array(M, dtype=np.float64)
    for c in range(6):
        piv = c
        for r in range(c + 1, 6):
            if abs(M[r, c]) > abs(M[piv, c]):
                piv = r
        if M[piv, c] == 0.0:
            return None
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        for r in range(c + 1, 6):
            f = M[r, c] / M[c, c]
            M[r, c:] = M[r, c:] - f * M[c, c:]
    x = np.zeros(6)
    for r in range(5, -1, -1):
        v = M[r, 6]
        for k in range(r + 1, 6):
            v -= M[r, k] * x[k]
        x[r] = v / M[r, r]
    return x


def vec6_to_mat4(x):
    cx, sx, cy, sy, cz, sz = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:6]
    return T


def icp_update(kind, s):
    """the update of one step from the reduced sums: Umeyama without scaling (LAPACK SVD) / the 6x6 normal equations (identity when the
    system is exactly singular)"""
    U = np.eye(4)
    if kind == 0:
        n = s[0]
        mu_s, mu_t = s[2:5] / n, s[5:8] / n
        C = s[8:17].reshape(3, 3).T / n - np.outer(mu_t, mu_s)
        Uu, _, Vt = np.linalg.svd(C)
        S = np.eye(3)
        if np.linalg.det(Uu) * np.linalg.det(Vt) < 0:
            S[2, 2] = -1.0
        R = Uu @ S @ Vt
        U[:3, :3], U[:3, 3] = R, mu_t - R @ mu_s
    else:
        M = np.zeros((6, 7))
        k = 2
        for a in range(6):
            for b in range(a, 6):
                M[a, b] = M[b, a] = s[k]
                k += 1
        M[:, 6] = -s[23:29]
        x = solve6(M)
        if x is not None:
            U = vec6_to_mat4(x)
    return U


def icp_step(kind, s, st, ns, rel_fitness, rel_rmse, max_iteration):
    """one icp_step on the 40-word state `st` (in place).  n_corr = floor(s0 + 0.5); exits in the order converged (strict <, never on
    the first evaluation) -> iteration limit -> too few correspondences; st[37] = 1 / 3 / 2"""
    if st[0] != 0.0:
        return
    n_corr = math.floor(s[0] + 0.5)
    fitness = n_corr / float(ns)
    rmse = math.sqrt(s[1] / n_corr) if n_corr > 0 else 0.0
    first = st[1] == 0.0 and st[38] == 0.0
    pf, pr = st[2], st[3]
    st[2], st[3], st[4], st[38] = fitness, rmse, n_corr, 1.0
    if not first and abs(pf - fitness) < rel_fitness and abs(pr - rmse) < rel_rmse:
        st[0], st[37] = 1.0, 1.0
        return
    if st[1] >= max_iteration:
        st[0], st[37] = 1.0, 3.0
        return
    if n_corr < (3 if kind == 0 else 6):
        st[0], st[37] = 1.0, 2.0
        return
    U = icp_update(kind, s)
    st[5:21] = (U @ st[5:21].reshape(4, 4)).reshape(-1)
    st[21:37] = U.reshape(-1)
    st[1] += 1.0


def icp_run(kind, src, tgt, tn, cell, max_dist, init, rel_fitness, rel_rmse, max_iteration, n_iter):
    """the enqueued chain of ape_icp_run_batch_f64 for one pair: the first evaluation and step, then n_iter times (apply the pending
    update, evaluate, step) -- each a no-op once st[0] is set.  -> (state[40], moved source)"""
    g = grid(tgt, cell, cell)
    T0 = np.array(init, dtype=np.float64).reshape(4, 4)
    st = np.zeros(40)
    st[5:21] = T0.reshape(-1)
    cur = transform(np.asarray(src, dtype=np.float64), T0)
    for it in range(n_iter + 1):
        if st[0] != 0.0:
            break
        if it:
            cur = transform(cur, st[21:37].reshape(4, 4))
        corr, d2 = nn1(g, cur, max_dist)
        s, _ = icp_sums_exact(kind, cur, tgt, tn, corr, d2)
        icp_step(kind, s, st, len(cur), rel_fitness, rel_rmse, max_iteration)
    return st, cur

"""numpy / scipy restatement of the global registration of csrc/registration.hip (open3d 0.9 compute_fpfh_feature and
registration_ransac_based_on_feature_matching with the seeded sampler of pc_reconstruction/pointcloud.py) -- test infrastructure.
Neighbour lists: d^2 < r^2 with d^2 = (ex*ex + ey*ey) + ez*ez, ordered by (d^2, index), first max_nn.  Feature distances are summed
over the 33 dimensions in order, like the kernel."""
import numpy as np
from scipy.spatial import cKDTree

_M64 = (1 << 64) - 1
_GAMMA, _MUL1, _MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def splitmix64(x):
    """the standard splitmix64 step on a 64-bit value (python int, or a numpy uint64 array)"""
    if isinstance(x, np.ndarray):
        with np.errstate(over="ignore"):
            z = x.astype(np.uint64) + np.uint64(_GAMMA)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(_MUL1)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(_MUL2)
            return z ^ (z >> np.uint64(31))
    z = (x + _GAMMA) & _M64
    z = ((z ^ (z >> 30)) * _MUL1) & _M64
    z = ((z ^ (z >> 27)) * _MUL2) & _M64
    return z ^ (z >> 31)


def sample_indices(seed, iterations, ransac_n, ns):
    """[len(iterations), ransac_n] source indices: splitmix64((seed << 32) ^ (i * ransac_n + j)) mod ns"""
    it = np.asarray(iterations, dtype=np.uint64).reshape(-1, 1)
    x = (np.uint64((int(seed) << 32) & _M64)) ^ (it * np.uint64(ransac_n) + np.arange(ransac_n, dtype=np.uint64)[None, :])
    return (splitmix64(x) % np.uint64(ns)).astype(np.int64)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def pair_features(p1, n1, p2, n2):
    """open3d ComputePairFeatures, vectorised over leading axes -> [..., 4] (f0, f1, f2, |d|)"""
    p1, n1, p2, n2 = (np.asarray(a, dtype=np.float64) for a in (p1, n1, p2, n2))
    dp = p2 - p1
    ln = np.sqrt(_dot(dp, dp))
    ok = ln != 0
    safe = np.where(ok, ln, 1.0)
    a1, a2 = _dot(n1, dp) / safe, _dot(n2, dp) / safe
    swap = np.arccos(np.abs(a1)) > np.arccos(np.abs(a2))
    m1 = np.where(swap[..., None], n2, n1)
    m2 = np.where(swap[..., None], n1, n2)
    dp = np.where(swap[..., None], -dp, dp)
    f2 = np.where(swap, -a2, a1)
    v = _cross(dp, m1)
    vn = np.sqrt(_dot(v, v))
    ok &= vn != 0
    v = v / np.where(vn != 0, vn, 1.0)[..., None]
    w = _cross(m1, v)
    f = np.stack([np.arctan2(_dot(w, m2), _dot(m1, m2)), _dot(v, m2), f2, ln], -1)
    return np.where(ok[..., None], f, 0.0)


def feature_bins(f):
    """[..., 4] pair features -> [..., 3] bin indices 0..32"""
    b0 = np.clip(np.floor(11.0 * (f[..., 0] + np.pi) / (2.0 * np.pi)), 0, 10)
    b1 = np.clip(np.floor(11.0 * (f[..., 1] + 1.0) * 0.5), 0, 10) + 11
    b2 = np.clip(np.floor(11.0 * (f[..., 2] + 1.0) * 0.5), 0, 10) + 22
    return np.stack([b0, b1, b2], -1).astype(np.int64)


def neighbour_lists(pts, radius, max_nn):
    pts = np.asarray(pts, dtype=np.float64)
    tree = cKDTree(pts)
    r2 = radius * radius
    out = []
    for i, cand in enumerate(tree.query_ball_point(pts, radius * (1 + 1e-9) + 1e-12)):
        cand = np.asarray(cand, dtype=np.int64)
        e = pts[cand] - pts[i]
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        keep = d2 < r2
        cand, d2 = cand[keep], d2[keep]
        o = np.lexsort((cand, d2))[:max_nn]
        out.append((cand[o], d2[o]))
    return out


def fpfh(pts, normals, radius, max_nn):
    """[n, 33] FPFH (open3d 0.9 Feature.cpp ComputeSPFHFeature / ComputeFPFHFeature)"""
    pts, normals = np.asarray(pts, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    n = len(pts)
    lists = neighbour_lists(pts, radius, max_nn)
    spfh = np.zeros((n, 33))
    for i, (idx, _) in enumerate(lists):
        if len(idx) <= 1:
            continue
        k = idx[1:]
        b = feature_bins(pair_features(pts[i], normals[i], pts[k], normals[k]))
        incr = 100.0 / (len(idx) - 1)
        for col in range(3):
            np.add.at(spfh[i], b[:, col], incr)
    out = np.zeros((n, 33))
    for i, (idx, d2) in enumerate(lists):
        if len(idx) <= 1:
            continue
        k, d = idx[1:], d2[1:]
        use = d != 0
        F = (spfh[k[use]] / d[use, None]).sum(0)
        s = F.reshape(3, 11).sum(1)
        sc = np.where(s != 0, 100.0 / np.where(s != 0, s, 1.0), 0.0)
        out[i] = F * np.repeat(sc, 11) + spfh[i]
    return out


def feature_nn(fs, ft, chunk=512):
    """nearest target feature of every source feature: d = sum_j (a_j - b_j)^2 in j order, ties -> lowest index.  A non-finite distance
    (a NaN or an infinity in either row, or an overflowing sum) never wins; a source row without any finite distance gets -1, and no RANSAC
    iteration that draws such a row is kept (ransac_hypotheses)."""
    fs, ft = np.asarray(fs, dtype=np.float64), np.asarray(ft, dtype=np.float64)
    out = np.empty(len(fs), np.int64)
    for a in range(0, len(fs), chunk):
        blk = fs[a:a + chunk]
        d = np.zeros((len(blk), len(ft)))
        for j in range(fs.shape[1]):
            e = blk[:, j, None] - ft[None, :, j]
            d += e * e
        d = np.where(np.isfinite(d), d, np.inf)
        best = np.argmin(d, 1)                      # first minimum = lowest index
        out[a:a + chunk] = np.where(np.isfinite(d[np.arange(len(blk)), best]), best, -1)
    return out


def umeyama(s, t):
    """Eigen::umeyama without scaling, batched: s, t [..., n, 3] -> [..., 4, 4]"""
    mu_s, mu_t = s.mean(-2), t.mean(-2)
    C = np.einsum("...ka,...kb->...ab", t - mu_t[..., None, :], s - mu_s[..., None, :]) / s.shape[-2]
    U, _, Vt = np.linalg.svd(C)
    S = np.ones(C.shape[:-1])
    S[..., 2] = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
    R = U @ (S[..., :, None] * Vt)
    T = np.zeros(C.shape[:-2] + (4, 4))
    T[..., :3, :3] = R
    T[..., :3, 3] = mu_t - np.einsum("...ab,...b->...a", R, mu_s)
    T[..., 3, 3] = 1.0
    return T


def _apply(T, p):
    """T [..., 4, 4] applied to p [..., n, 3] in the kernels' operation order"""
    return np.stack([((T[..., r, 0, None] * p[..., 0] + T[..., r, 1, None] * p[..., 1]) + T[..., r, 2, None] * p[..., 2]) + T[..., r, 3, None]
                     for r in range(3)], -1)


def ransac_hypotheses(src, tgt, nn, ransac_n, seed, edge_sim, dist_thr, max_iteration, max_validation, chunk=1 << 16):
    """the first max_validation iteration indices that pass the checkers, in iteration order (edge_sim / dist_thr < 0: no checker); an
    iteration that draws a source row without a match (nn < 0 or >= len(tgt)) is refused before any checker"""
    src, tgt, nn = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64), np.asarray(nn, dtype=np.int64)
    kept = []
    for a in range(0, max_iteration, chunk):
        its = np.arange(a, min(max_iteration, a + chunk))
        s = sample_indices(seed, its, ransac_n, len(src))
        t = nn[s]
        ok = ((t >= 0) & (t < len(tgt))).all(1)
        t = np.where(ok[:, None], t, 0)
        if edge_sim >= 0:
            for i in range(ransac_n):
                for j in range(i + 1, ransac_n):
                    es, et = src[s[:, i]] - src[s[:, j]], tgt[t[:, i]] - tgt[t[:, j]]
                    ds, dt = np.sqrt(_dot(es, es)), np.sqrt(_dot(et, et))
                    ok &= ~((ds < dt * edge_sim) | (dt < ds * edge_sim))
        if dist_thr >= 0 and ok.any():
            T = umeyama(src[s[ok]], tgt[t[ok]])
            e = tgt[t[ok]] - _apply(T, src[s[ok]])
            ok[np.flatnonzero(ok)] = (np.sqrt(_dot(e, e)) <= dist_thr).all(1)
        kept.extend(its[ok].tolist())
        if len(kept) >= max_validation:
            break
    return np.asarray(kept[:max_validation], dtype=np.int64)


def evaluate(src, tgt, T, max_dist):
    """(fitness, rmse, count) of T: nearest target of every moved source point with d^2 < max_dist^2"""
    p = _apply(T, np.asarray(src, dtype=np.float64))
    _, j = cKDTree(tgt).query(p)
    e = tgt[j] - p
    d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    m = d2 < max_dist * max_dist
    c = int(m.sum())
    return c / len(src), (np.sqrt(d2[m].sum() / c) if c else 0.0), c


def ransac(src, tgt, fs, ft, max_dist, ransac_n, seed, edge_sim, dist_thr, max_iteration, max_validation):
    """-> dict(T, fitness, rmse, count, kept, winner): the whole registration_ransac_based_on_feature_matching restated"""
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    nn = feature_nn(fs, ft)
    kept = ransac_hypotheses(src, tgt, nn, ransac_n, seed, edge_sim, dist_thr, max_iteration, max_validation)
    best = dict(T=np.eye(4), fitness=0.0, rmse=0.0, count=0, kept=kept, winner=-1, nn=nn)
    if len(kept):
        s = sample_indices(seed, kept, ransac_n, len(src))
        Ts = umeyama(src[s], tgt[nn[s]])
        for k, T in enumerate(Ts):
            f, r, c = evaluate(src, tgt, T, max_dist)
            if f > best["fitness"] or (f == best["fitness"] and r < best["rmse"]):
                best.update(T=T, fitness=f, rmse=r, count=c, winner=int(kept[k]))
    return best

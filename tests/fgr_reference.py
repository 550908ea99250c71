"""numpy float64 restatement of fast global registration as pc_reconstruction.pointcloud.registration_fast_based_on_feature_matching
defines it (open3d 0.9 FastGlobalRegistration restated with a seeded tuple sampler) -- test infrastructure and the
specification of the fgr_* kernels of csrc/registration.hip.  It imports nothing from the package.

    mutual matches -> tuple test -> centring and scale -> Gauss-Newton with a 6x6 LDL^T -> back to the clouds' units -> ICP evaluation
"""
import math

import numpy as np

_M64 = (1 << 64) - 1
_GAMMA, _MUL1, _MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

DEFAULTS = dict(division_factor=1.4, use_absolute_scale=False, decrease_mu=False, maximum_correspondence_distance=0.025, iteration_number=64,
                tuple_scale=0.95, maximum_tuple_count=1000, seed=0)


def options(**kw):
    o = dict(DEFAULTS)
    assert set(kw) <= set(o), kw
    o.update(kw)
    return o


def splitmix64(x):
    """the standard splitmix64 step on a numpy uint64 array"""
    with np.errstate(over="ignore"):
        z = x.astype(np.uint64) + np.uint64(_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_MUL1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_MUL2)
        return z ^ (z >> np.uint64(31))


def draws(seed, trials, ncorr):
    """[len(trials), 3] positions of the mutual list: splitmix64((seed << 32) ^ (3 t + k)) mod ncorr"""
    t = np.asarray(trials, dtype=np.uint64).reshape(-1, 1)
    x = np.uint64((int(seed) << 32) & _M64) ^ (t * np.uint64(3) + np.arange(3, dtype=np.uint64)[None, :])
    return (splitmix64(x) % np.uint64(ncorr)).astype(np.int64)


def feature_nn(fs, ft, chunk=512):
    """nearest target feature of every source feature: d = sum_j (a_j - b_j)^2 in j order, ties -> lowest index; -1 without a finite
    distance (or without targets)"""
    fs, ft = np.asarray(fs, dtype=np.float64).reshape(-1, 33), np.asarray(ft, dtype=np.float64).reshape(-1, 33)
    out = np.full(len(fs), -1, np.int64)
    if len(ft) == 0:
        return out
    for a in range(0, len(fs), chunk):
        blk = fs[a:a + chunk]
        d = np.zeros((len(blk), len(ft)))
        for j in range(33):
            e = blk[:, j, None] - ft[None, :, j]
            d += e * e
        d = np.where(np.isfinite(d), d, np.inf)
        best = np.argmin(d, 1)
        out[a:a + chunk] = np.where(np.isfinite(d[np.arange(len(blk)), best]), best, -1)
    return out


def mutual_matches(nn_st, nn_ts):
    """[ncorr, 2]: the pairs (i, nn_st[i]) with nn_ts[nn_st[i]] == i, in ascending i"""
    nn_st, nn_ts = np.asarray(nn_st, dtype=np.int64), np.asarray(nn_ts, dtype=np.int64)
    i = np.arange(len(nn_st))
    ok = (nn_st >= 0) & (nn_st < len(nn_ts))
    ok[ok] = nn_ts[nn_st[ok]] == i[ok]
    return np.stack([i[ok], nn_st[ok]], 1)


def _norm(e):
    return np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])


def tuple_pass(src, tgt, matches, seed, trials, tuple_scale):
    """bool per trial: for the edges 0-1, 1-2, 2-0, li * tuple_scale < lj and lj * tuple_scale < li (strict)"""
    r = draws(seed, trials, len(matches))
    s, t = matches[r, 0], matches[r, 1]
    ok = np.ones(len(r), bool)
    for k in range(3):
        li = _norm(src[s[:, k]] - src[s[:, (k + 1) % 3]])
        lj = _norm(tgt[t[:, k]] - tgt[t[:, (k + 1) % 3]])
        ok &= (li * tuple_scale < lj) & (lj * tuple_scale < li)
    return ok


def kept_trials(src, tgt, matches, seed, tuple_scale, maximum_tuple_count, chunk=1 << 16):
    """the first maximum_tuple_count passing trials of 0 .. 100 * ncorr - 1, in trial order"""
    ncorr = len(matches)
    kept = []
    for a in range(0, 100 * ncorr, chunk):
        if len(kept) >= maximum_tuple_count:
            break
        trials = np.arange(a, min(100 * ncorr, a + chunk))
        kept.extend(trials[tuple_pass(src, tgt, matches, seed, trials, tuple_scale)].tolist())
    return np.asarray(kept[:max(int(maximum_tuple_count), 0)], dtype=np.int64)


def correspondences(matches, seed, kept):
    """[3 * len(kept), 2] (source, target) index pairs: every kept trial's three pairs, duplicates included"""
    if len(kept) == 0:
        return np.zeros((0, 2), np.int64)
    return matches[draws(seed, kept, len(matches)).reshape(-1)]


def vec6_to_mat4(x):
    """open3d TransformVector6dToMatrix4d: R = Rz(x[2]) Ry(x[1]) Rx(x[0]), t = x[3:6]"""
    cx, sx, cy, sy, cz, sz = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:6]
    return T


def ldlt_solve(A, b):
    """(x with A x = b by L D L^T without pivoting, the pivots) or (None, the pivots so far) at a pivot that is not finite and positive"""
    L, D = np.eye(6), np.zeros(6)
    for j in range(6):
        d = A[j, j] - float(np.sum(L[j, :j] ** 2 * D[:j]))
        if not (d > 0.0 and np.isfinite(d)):
            return None, D[:j].tolist() + [d]
        D[j] = d
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - float(np.sum(L[i, :j] * L[j, :j] * D[:j]))) / d
    y = np.zeros(6)
    for i in range(6):
        y[i] = b[i] - float(np.sum(L[i, :i] * y[:i]))
    y /= D
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = y[i] - float(np.sum(L[i + 1:, i] * x[i + 1:]))
    return x, D.tolist()


def normal_equations(p, q, par):
    """(JTJ [6, 6], JTr [6]) of the correspondences p (target) / q (moved source) at penalty par"""
    r = p - q
    s = (par / ((r * r).sum(1) + par)) ** 2
    n = len(p)
    J = np.zeros((n, 3, 6))
    J[:, 0, 1], J[:, 0, 2], J[:, 0, 3] = -q[:, 2], q[:, 1], -1.0
    J[:, 1, 0], J[:, 1, 2], J[:, 1, 4] = q[:, 2], -q[:, 0], -1.0
    J[:, 2, 0], J[:, 2, 1], J[:, 2, 5] = -q[:, 1], q[:, 0], -1.0
    JTJ, JTr = np.zeros((6, 6)), np.zeros(6)
    for k in range(3):
        JTJ += (J[:, k, :] * s[:, None]).T @ J[:, k, :]
        JTr += (J[:, k, :] * (s * r[:, k])[:, None]).sum(0)
    return JTJ, JTr


def optimize(src, tgt, corr, opt):
    """steps 3-5 on a correspondence list -> dict(T, iterations, scale, par, pivots: the last solve's)"""
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    mean_s, mean_t = src.mean(0), tgt.mean(0)
    scale = max(_norm(src - mean_s).max(), _norm(tgt - mean_t).max())
    scale_global, par = (1.0, scale) if opt["use_absolute_scale"] else (scale, 1.0)
    out = dict(T=np.eye(4), iterations=0, scale=scale, par=par, pivots=None)
    if len(corr) < 10:
        return out
    p = (tgt[corr[:, 1]] - mean_t) / scale_global
    q = (src[corr[:, 0]] - mean_s) / scale_global
    T = np.eye(4)
    it = 0
    while it < int(opt["iteration_number"]):
        if opt["decrease_mu"] and it % 4 == 0 and par > opt["maximum_correspondence_distance"]:
            par /= opt["division_factor"]
        JTJ, JTr = normal_equations(p, q, par)
        x, out["pivots"] = ldlt_solve(JTJ, JTr)
        if x is None:
            break
        delta = vec6_to_mat4(-x)
        T = delta @ T
        q = q @ delta[:3, :3].T + delta[:3, 3]
        it += 1
    R = T[:3, :3]
    res = np.eye(4)
    res[:3, :3] = R
    res[:3, 3] = scale_global * T[:3, 3] + mean_t - R @ mean_s
    out.update(T=res, iterations=it, par=par)
    return out


def evaluate(src, tgt, T, max_dist, chunk=1024):
    """(fitness, rmse, count) of T: the nearest target of every moved source point counts when d^2 < max_dist^2"""
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    p = src @ T[:3, :3].T + T[:3, 3]
    d2 = np.empty(len(p))
    for a in range(0, len(p), chunk):
        e = p[a:a + chunk, None, :] - tgt[None, :, :]
        d2[a:a + chunk] = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).min(1)
    m = d2 < max_dist * max_dist
    c = int(m.sum())
    return c / len(src), (math.sqrt(d2[m].sum() / c) if c else 0.0), c


def fgr(src, tgt, fs, ft, opt=None, reverse=False):
    """the whole registration -> dict(T, fitness, rmse, count, mutual, tuples, iterations, matches, kept, scale, par, pivots);
    reverse: the correspondence list reversed (another summation order, the same sums)"""
    opt = options() if opt is None else opt
    src, tgt = np.asarray(src, dtype=np.float64).reshape(-1, 3), np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    if len(src) == 0 or len(tgt) == 0:
        return dict(T=np.eye(4), fitness=0.0, rmse=0.0, count=0, mutual=0, tuples=0, iterations=0, matches=np.zeros((0, 2), np.int64),
                    kept=np.zeros(0, np.int64), scale=0.0, par=0.0, pivots=None)
    matches = mutual_matches(feature_nn(fs, ft), feature_nn(ft, fs))
    kept = kept_trials(src, tgt, matches, opt["seed"], opt["tuple_scale"], opt["maximum_tuple_count"]) if len(matches) else np.zeros(0, np.int64)
    corr = correspondences(matches, opt["seed"], kept)
    out = optimize(src, tgt, corr[::-1] if reverse else corr, opt)
    mcd = opt["maximum_correspondence_distance"]
    out["fitness"], out["rmse"], out["count"] = evaluate(src, tgt, out["T"], mcd) if mcd > 0 else (0.0, 0.0, 0)
    out.update(mutual=len(matches), tuples=len(kept), matches=matches, kept=kept)
    return out

"""Edge-shape inputs for the global-registration kernels (csrc/registration.hip) with the guards that make them well-posed -- test
infrastructure, plain numpy, seeded, no GPU.  tests/test_registration_host.py proves on the CPU that every case builds, holds its guards
and reaches the path it is named for; tests/test_gpu_registration_edges.py feeds the same inputs to the kernels and compares with the
restatement (tests/registration_reference.py).

Guards (conditions on the INPUTS, computed from the restatement alone; a case that misses one gets another seed, never a looser bound):
  bin margin        every pre-floor bin coordinate of every pair feature that is not the all-zero one is >= MARGIN from an integer
  swap margin       |acos|a1| - acos|a2|| of every pair is exactly 0 or >= MARGIN
  rank guard        a hypothesis is well-posed when sigma_2 > 1e-6 sigma_1 of its covariance; transformations are compared for those only
  threshold guards  no edge ratio / checker distance within MARGIN (relative) of its threshold, no validation distance within MARGIN of
                    max_dist -- except where a case puts a point exactly on a threshold with exactly representable coordinates
Normals are random unit vectors (never axis-aligned: atan2(+-0, +-0) would decide a bin), except in the vn == 0 row whose features are
all zero on both sides."""
import functools
import math

import numpy as np
from scipy.spatial import cKDTree

import registration_reference as R

MARGIN = 1e-9
WELL_POSED = 1e-6
cached = functools.lru_cache(maxsize=None)


def unit_normals(n, seed, positive_x=False):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if positive_x:
        v[:, 0] = np.abs(v[:, 0])
    return v


def lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    return g.reshape(-1, 3).astype(np.float64)


def rigid(seed, angle=1.1, t=(0.3, -0.2, 0.1)):
    a = np.random.default_rng(seed).standard_normal(3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    T[:3, 3] = t
    return T


# ---- FPFH ---------------------------------------------------------------------------------------------------------------------------
def _fcase(name, pts, normals, radius, max_nns, zero_only=False):
    return dict(name=name, pts=np.ascontiguousarray(pts, dtype=np.float64), normals=np.ascontiguousarray(normals, dtype=np.float64),
                radius=float(radius), max_nns=tuple(max_nns), zero_only=zero_only)


@cached
def fpfh_cases():
    """name -> case; every cloud with its injected normals, its radius and the max_nn values to run"""
    out = []
    lat9 = lattice(9, 9, 3)
    out.append(_fcase("lattice9_r2.5", lat9, unit_normals(243, 1), 2.5, (1, 2, 7, 27, 100, 128)))
    out.append(_fcase("lattice9_r2", lat9, unit_normals(243, 1), 2.0, (1, 2, 7, 27, 100, 128)))      # d^2 == 4 neighbours excluded
    out.append(_fcase("lattice7_r6", lattice(7, 7, 7), unit_normals(343, 2), 6.0, (128, 5)))          # listed and re-walk routes
    rng = np.random.default_rng(3)
    clusters = np.r_[rng.uniform(0, 0.5, (256, 3)), rng.uniform(0, 0.5, (257, 3)) + 100.0]            # every pair of a cluster < radius 1
    out.append(_fcase("clusters_256_257", clusters, unit_normals(513, 4), 1.0, (128, 100)))
    base, generic = rng.uniform(0, 10, (20, 3)), rng.uniform(-1, 11, (100, 3))
    out.append(_fcase("triples", np.r_[base, generic[:50], base, generic[50:], base], unit_normals(160, 5), 3.0, (128, 10, 3)))
    out.append(_fcase("isolated", np.r_[rng.uniform(0, 5, (40, 3)), [[1000.0, -1000.0, 500.0]]], unit_normals(41, 6), 2.0, (100, 2)))
    for n in (1, 2, 7, 8, 9):
        out.append(_fcase("n%d" % n, rng.uniform(0, 1, (n, 3)), unit_normals(n, 10 + n), 2.0, (100, 2)))
    row = np.zeros((6, 3))
    row[:, 0] = np.arange(6)
    out.append(_fcase("vn0_row", row, np.tile([1.0, 0.0, 0.0], (6, 1)), 2.5, (100, 3), zero_only=True))
    # all-zero normals among generic ones; the generic ones point to +x so that m1 . 0 is +0 whatever the signs (atan2(+-0, +0) = +-0)
    zn = unit_normals(60, 7, positive_x=True)
    zn[[0, 7, 8, 30]] = 0.0
    out.append(_fcase("zero_normals", rng.uniform(0, 6, (60, 3)), zn, 2.5, (100, 16)))
    return {c["name"]: c for c in out}


@cached
def full_lists(name):
    """the restatement's complete (uncut) neighbour lists of a case"""
    c = fpfh_cases()[name]
    return R.neighbour_lists(c["pts"], c["radius"], 1 << 30)


def candidate_counts(name):
    return np.array([len(i) for i, _ in full_lists(name)])


def fpfh_margins(name):
    """(bin margin, swap margin, non-zero pair features seen) over every (point, list entry >= 1) pair of the case's longest lists"""
    c = fpfh_cases()[name]
    pts, nrm, top = c["pts"], c["normals"], max(c["max_nns"])
    bin_m, swap_m, seen = np.inf, np.inf, 0
    for i, (idx, _) in enumerate(full_lists(name)):
        k = idx[:top][1:]
        if len(k) == 0:
            continue
        f = R.pair_features(pts[i], nrm[i], pts[k], nrm[k])
        nz = np.any(f != 0, -1)
        seen += int(nz.sum())
        co = np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5, 11.0 * (f[:, 2] + 1.0) * 0.5], -1)[nz]
        if len(co):
            bin_m = min(bin_m, float(np.abs(co - np.rint(co)).min()))
        dp = pts[k] - pts[i]
        ln = np.sqrt((dp * dp).sum(1))
        ok = ln != 0
        a1, a2 = (nrm[i] * dp).sum(1)[ok] / ln[ok], (nrm[k] * dp).sum(1)[ok] / ln[ok]
        sw = np.abs(np.arccos(np.abs(a1)) - np.arccos(np.abs(a2)))
        sw = sw[sw != 0]
        if len(sw):
            swap_m = min(swap_m, float(sw.min()))
    return bin_m, swap_m, seen


@cached
def fpfh_expected(name, max_nn):
    c = fpfh_cases()[name]
    return R.fpfh(c["pts"], c["normals"], c["radius"], max_nn)


BATCH_RADIUS, BATCH_MAX_NN = 2.5, 100


def fpfh_batch_list():
    """names for one batched call: None is the empty cloud; more than 16 clouds, so the list spans two launches"""
    names = [n for n in fpfh_cases() if n != "lattice9_r2"]
    return [None] + names + ["n7", "lattice9_r2.5", "triples", "n1", "vn0_row"]


# ---- matching -----------------------------------------------------------------------------------------------------------------------
MATCH_SHAPES = ((1, 1), (1, 1000), (128, 64), (129, 65), (300, 1), (257, 4097))


def _features(rng, n):
    return rng.uniform(0.0, 200.0, (n, 33))


@cached
def matching_case(ns, nt):
    """random features with exact copies of a source row's winner planted on both sides of every 64-row border named in BORDERS (the
    tile border of the kernel; a slice border too, alone or in a 16-pair launch) and in the last row.  -> fs, ft, {row: lowest planted}"""
    rng = np.random.default_rng(1000 * ns + nt)
    fs, ft = _features(rng, ns), _features(rng, nt)
    planted = {}
    borders = [b for b in (64, 128, 192, 4096) if b < nt]
    rows = sorted(set(int(r) for r in np.linspace(0, ns - 1, len(borders) + 1)))
    for k, b in enumerate(borders):
        r = rows[k % len(rows)]
        ft[b - 1] = ft[b] = fs[r] + 0.25                      # exactly equal rows: distance 33 / 16 against ~2e5 for a random row
        planted.setdefault(r, []).append(b - 1)
    used = {p for b in borders for p in (b - 1, b)}
    free = [p for p in range(1, nt) if p not in used]
    r = rows[-1]
    if free and r in planted:                                 # one more copy far behind: the last slice must not replace the winner
        ft[free[-1]] = ft[planted[r][0]]
    elif free and 0 not in used:                              # a tie between the first row and the last free one
        ft[0] = ft[free[-1]] = fs[r] + 0.25
        planted[r] = [0]
    return fs, ft, {r: min(p) for r, p in planted.items()}


@cached
def nan_case():
    """features with one all-NaN and one partly-NaN source row and two NaN target rows (one of them row 0), and a point pair for a RANSAC
    run over the resulting nn"""
    rng = np.random.default_rng(77)
    fs, ft = _features(rng, 130), _features(rng, 70)
    fs[5] = np.nan
    fs[6, 3] = np.nan
    ft[0] = np.nan
    ft[64, 32] = np.nan
    ft[1] = ft[65] = fs[4] + 0.25                             # the neighbours of the NaN rows still find their (tied) winner
    return dict(fs=fs, ft=ft, src=rng.uniform(-50, 50, (130, 3)), tgt=rng.uniform(-50, 50, (70, 3)), no_match=(5, 6), nan_targets=(0, 64))


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------------
EDGE, DIST, MAX_DIST = 0.9, 0.05, 0.1
CHECKERS = ((-1.0, -1.0), (EDGE, -1.0), (-1.0, DIST), (EDGE, DIST))


@cached
def ransac_pair(ns=300, seed=0, wrong=0.25):
    """a random source in a unit cube, the target a rigid move of it plus 1e-2 noise (never an exact copy: with one every hypothesis has
    fitness 1 and rmse noise decides), nn the identity with a fraction `wrong` of the rows re-drawn, and features that give this nn.
    Coordinates of order 1 against residuals of order 1e-2: an rmse is a difference of coordinates, so one rounding of a coordinate
    moves it by about 2^-53 / 1e-2 ~ 1e-14 relative, two orders inside the 1e-12 the kernels are held to (a 100 mm cube with the same
    noise would sit AT that bound)"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-0.5, 0.5, (ns, 3))
    T = rigid(seed + 1)
    tgt = src @ T[:3, :3].T + T[:3, 3] + 1e-2 * rng.standard_normal((ns, 3))
    nn = np.arange(ns)
    bad = rng.random(ns) < wrong
    nn[bad] = rng.integers(0, ns, int(bad.sum()))
    ft = _features(rng, ns)
    fs = ft[nn] + 0.01 * rng.standard_normal((ns, 33))
    return dict(src=src, tgt=tgt, nn=nn, fs=fs, ft=ft, T=T)


@cached
def tiny_pair(ns):
    rng = np.random.default_rng(500 + ns)
    return dict(src=rng.uniform(-5, 5, (ns, 3)), tgt=rng.uniform(-5, 5, (5, 3)), nn=rng.integers(0, 5, ns))


@cached
def far_pair():
    """a 60-point target in a unit cube; the source is a rigid move of it (1e-2 noise, matched row by row) plus 240 points spread over
    a hundred times that with arbitrary matches: every hypothesis moves most of the source far outside the cells of the target's grid
    (cell = max_dist = 0.1), on both sides of its origin, and the ones drawn from the first 60 rows still find their matches"""
    rng = np.random.default_rng(900)
    tgt = rng.uniform(0, 1, (60, 3)) + [0.4, -0.3, 0.2]
    T = rigid(901)
    near = (tgt - T[:3, 3]) @ T[:3, :3] + 1e-2 * rng.standard_normal((60, 3))
    return dict(src=np.r_[near, rng.uniform(-50, 50, (240, 3))], tgt=tgt, nn=np.r_[np.arange(60), rng.integers(0, 60, 240)], T=T)


def exact_pair():
    """integer coordinates: the iterations that draw one source point only have a zero covariance, so T is the exact translation onto
    its match, and the OTHER source point then lies exactly max_dist = 5 from its nearest target ((3, 4, 0) away): not counted.  Mixed
    draws are refused by the edge-length checker (10 against sqrt(185)), so every kept hypothesis has (fitness, rmse) = (0.5, 0)."""
    return dict(src=np.array([[0.0, 0, 0], [10.0, 0, 0]]), tgt=np.array([[100.0, 0, 0], [113.0, 4, 0]]), nn=np.array([0, 1]), max_dist=5.0)


def hypothesis_report(src, tgt, nn, ransac_n, seed, its, edge_sim=-1.0, dist_thr=-1.0):
    """for the given iterations: sigma [n, 3] (singular values of the covariance), drawn (the iteration has a match for every draw),
    edge_margin / dist_margin [n] (smallest relative distance of an edge comparison / a checker distance from its threshold; inf where
    the checker is off, the iteration is refused before it, or both sides of the comparison are exactly 0)"""
    src, tgt, nn = np.asarray(src, np.float64), np.asarray(tgt, np.float64), np.asarray(nn, np.int64)
    its = np.asarray(its, np.int64)
    s = R.sample_indices(seed, its, ransac_n, len(src))
    t = nn[s]
    drawn = ((t >= 0) & (t < len(tgt))).all(1)
    t = np.where(drawn[:, None], t, 0)
    ps, pt = src[s], tgt[t]
    C = np.einsum("...ka,...kb->...ab", pt - pt.mean(-2, keepdims=True), ps - ps.mean(-2, keepdims=True)) / ransac_n
    sigma = np.linalg.svd(C, compute_uv=False)
    edge_m = np.full(len(its), np.inf)
    edge_ok = np.ones(len(its), bool)
    if edge_sim >= 0:
        for i in range(ransac_n):
            for j in range(i + 1, ransac_n):
                ds, dt = np.linalg.norm(ps[:, i] - ps[:, j], axis=1), np.linalg.norm(pt[:, i] - pt[:, j], axis=1)
                for a, b in ((ds, dt * edge_sim), (dt, ds * edge_sim)):
                    big = np.maximum(a, b)
                    edge_m = np.minimum(edge_m, np.where(big > 0, np.abs(a - b) / np.where(big > 0, big, 1.0), np.inf))
                edge_ok &= ~((ds < dt * edge_sim) | (dt < ds * edge_sim))
    dist_m = np.full(len(its), np.inf)
    if dist_thr >= 0:
        e = pt - R._apply(R.umeyama(ps, pt), ps)
        d = np.sqrt((e * e).sum(-1))
        dist_m = np.where(edge_ok, (np.abs(d - dist_thr) / dist_thr).min(1), np.inf)
    edge_m[~drawn] = np.inf
    dist_m[~drawn] = np.inf
    return dict(sigma=sigma, drawn=drawn, edge_margin=edge_m, dist_margin=dist_m)


def hypotheses_in_range(p, ransac_n, seed, edge_sim, dist_thr, it_begin, n_it):
    """the passing iterations of [it_begin, it_begin + n_it) of pair p: R.ransac_hypotheses restated for a window that does not start at
    0 (the sampler is a pure function of the iteration index); test_registration_host.py checks the two agree for it_begin = 0"""
    src, tgt, nn = p["src"], p["tgt"], np.asarray(p["nn"], np.int64)
    its = np.arange(it_begin, it_begin + n_it)
    s = R.sample_indices(seed, its, ransac_n, len(src))
    t = nn[s]
    ok = ((t >= 0) & (t < len(tgt))).all(1)
    t = np.where(ok[:, None], t, 0)
    if edge_sim >= 0:
        for i in range(ransac_n):
            for j in range(i + 1, ransac_n):
                es, et = src[s[:, i]] - src[s[:, j]], tgt[t[:, i]] - tgt[t[:, j]]
                ds, dt = np.sqrt(R._dot(es, es)), np.sqrt(R._dot(et, et))
                ok &= ~((ds < dt * edge_sim) | (dt < ds * edge_sim))
    if dist_thr >= 0 and ok.any():
        T = R.umeyama(src[s[ok]], tgt[t[ok]])
        e = tgt[t[ok]] - R._apply(T, src[s[ok]])
        ok[np.flatnonzero(ok)] = (np.sqrt(R._dot(e, e)) <= dist_thr).all(1)
    return its[ok]


def well_posed(sigma):
    sigma = np.asarray(sigma)
    return sigma[..., 1] > WELL_POSED * sigma[..., 0]


def validation_margin(src, tgt, T, max_dist):
    """smallest |d - max_dist| over the nearest-target distances of the source moved by T ([4, 4] or [k, 4, 4])"""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    tree = cKDTree(tgt)
    return min(float(np.abs(tree.query(R._apply(t, np.asarray(src, np.float64)))[0] - max_dist).min()) for t in T)


def kept_transforms(src, tgt, nn, ransac_n, seed, kept):
    s = R.sample_indices(seed, kept, ransac_n, len(src))
    return R.umeyama(np.asarray(src)[s], np.asarray(tgt)[np.asarray(nn)[s]])


def ransac_from_nn(src, tgt, nn, max_dist, ransac_n, seed, edge_sim, dist_thr, max_iteration, max_validation):
    """R.ransac for a given nn (no features)"""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    kept = R.ransac_hypotheses(src, tgt, nn, ransac_n, seed, edge_sim, dist_thr, max_iteration, max_validation)
    best = dict(T=np.eye(4), fitness=0.0, rmse=0.0, count=0, kept=kept, winner=-1, position=-1)
    for k, T in enumerate(kept_transforms(src, tgt, nn, ransac_n, seed, kept) if len(kept) else ()):
        f, r, c = R.evaluate(src, tgt, T, max_dist)
        if f > best["fitness"] or (f == best["fitness"] and r < best["rmse"]):
            best.update(T=T, fitness=f, rmse=r, count=c, winner=int(kept[k]), position=k)
    return best


# the winner comparisons: (name, ransac_n, edge_sim, dist_thr, max_dist, seed, max_iteration, max_validation)
WINNER_RUNS = (("move_n3", 3, EDGE, DIST, MAX_DIST, 11, 3000, 100), ("move_n4", 4, EDGE, DIST, MAX_DIST, 12, 3000, 100),
               ("nothing_matches", 3, EDGE, DIST, 1e-4, 13, 3000, 20), ("far_target", 3, EDGE, -1.0, MAX_DIST, 14, 20000, 100))


@cached
def winner_run(name):
    """the restatement's whole result of a winner run plus its guards: dict(pair, args, want, sigma (of the winner), margins)"""
    _, rn, edge, dist, max_dist, seed, max_it, max_val = next(r for r in WINNER_RUNS if r[0] == name)
    pair = far_pair() if name == "far_target" else ransac_pair()
    src, tgt, nn = pair["src"], pair["tgt"], pair["nn"]
    want = ransac_from_nn(src, tgt, nn, max_dist, rn, seed, edge, dist, max_it, max_val)
    its = np.arange(int(want["kept"][-1]) + 1 if len(want["kept"]) >= max_val else max_it)
    rep = hypothesis_report(src, tgt, nn, rn, seed, its, edge, dist)
    sigma = hypothesis_report(src, tgt, nn, rn, seed, [max(want["winner"], 0)])["sigma"][0]
    vm = validation_margin(src, tgt, kept_transforms(src, tgt, nn, rn, seed, want["kept"]), max_dist) if len(want["kept"]) else np.inf
    return dict(pair=pair, ransac_n=rn, edge=edge, dist=dist, max_dist=max_dist, seed=seed, max_it=max_it, max_val=max_val, want=want,
                sigma=sigma, edge_margin=float(rep["edge_margin"].min()), dist_margin=float(rep["dist_margin"].min()), validation_margin=vm)

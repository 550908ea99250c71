"""Edge-shape inputs for the point-cloud kernels (csrc/pointcloud.hip) with the guards that make a failure mean a wrong kernel -- test
infrastructure, plain numpy, seeded, no GPU.  tests/test_pointcloud_host.py proves on the CPU that every case builds, holds its guards and
reaches the branch it is named for; tests/test_gpu_pointcloud_edges.py feeds the same inputs to the kernels and compares with the
restatement (tests/pointcloud_reference.py).

Input rules:
  exact cases   where a case puts something exactly ON a threshold (a distance tie, d == radius, a point on a cell or voxel border,
                d == max_dist) every coordinate, cell size, voxel size and radius in it is a small multiple of a power of two (`exact=True`):
                (p - origin) / cell and every d^2 are exact on both sides.
  margins       everywhere else no d^2 lies within MARGIN (relative) of r^2 or max_dist^2, no pre-floor cell coordinate within MARGIN of an
                integer (but the point that sets the lower bound: it sits at `shift / cell` by construction, and the subtraction and the
                division are correctly rounded on both sides), no k-NN settle comparison within MARGIN of its bound.  A case that misses a
                margin gets another seed, never a looser bound.
  no exclusions the normals comparison covers every point of every case."""
import functools
import math

import numpy as np

import pointcloud_reference as R

MARGIN = 1e-9
cached = functools.lru_cache(maxsize=None)


def lattice(nx, ny, nz):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1)
    return g.reshape(-1, 3).astype(np.float64)


SHEAR = np.array([[1.0, 0.25, 0.0], [0.0, 1.0, 0.25], [0.0, 0.0, 0.75]])      # dyadic: a sheared lattice keeps exact coordinates and its
                                                                             # +-offset ties, and its covariances are not isotropic


def shuffled(pts, seed):
    """original order != sorted order, so that (d^2, original index) and (d^2, sorted position) are different rules"""
    return np.ascontiguousarray(pts[np.random.default_rng(seed).permutation(len(pts))])


def unit(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rigid(rx, ry, rz, t):
    return R.vec6_to_mat4([rx, ry, rz, *t])


def pre_floor_margin(g):
    """smallest distance of a pre-floor cell coordinate from an integer, the points that set the lower bound of an axis left out"""
    pre = g["pre"]
    frac = np.abs(pre - np.round(pre))
    frac[g["pts"] == g["lo"]] = 1.0
    return float(frac.min()) if frac.size else 1.0


def radius_margin(d2, r):
    """smallest relative distance of a d^2 from r^2"""
    return float((np.abs(np.asarray(d2) - r * r) / (r * r)).min()) if np.size(d2) else 1.0


# ---- surface points -----------------------------------------------------------------------------------------------------------------------
SURFACE_SHAPES = ((1, 1), (45, 91), (64, 64), (17, 241), (5, 7))              # H * W of 1, 4095, 4096, 4097 and an odd-width image


def _mask(kind, n, rng):
    m = np.zeros(n, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "first_last":
        m[[0, n - 1]] = 255
    elif kind == "wave":                                 # the last pixel of a wave's 256 and the first of the next
        m[[i for i in (255, 256) if i < n]] = 255
    elif kind == "chunk":                                # the last pixel of the compaction's 4096-chunk and the first of the next
        m[[i for i in (4095, 4096) if i < n]] = 1
    elif kind == "random":
        m[:] = rng.choice(np.array([0, 1, 255], np.uint8), n)
    return m


@cached
def surface_batch(shape):
    """views of one image size: [(label, depth, robot2cam, intr)] with their mask kinds; 17 views (16 + 1 batches) for the 17 x 241 image"""
    H, W = shape
    n = H * W
    rng = np.random.default_rng(100 + n)
    kinds = ["all", "zero", "first_last", "wave", "chunk", "random"]
    if shape == (17, 241):
        kinds += ["random"] * 11
    views = []
    for v, kind in enumerate(kinds):
        label = _mask(kind, n, rng)
        depth = rng.integers(1, 65536, n).astype(np.uint16)
        depth[0], depth[n - 1] = 1, 65535
        if kind in ("all", "random") and n > 2:
            depth[n // 2] = 0                            # depth 0 under a set label
            label[n // 2] = 255
        intr = {"fx": 600.0 + 3.7 * v, "fy": 590.0 - 1.3 * v, "ppx": W / 2 - 0.3 * v, "ppy": H / 2 + 0.7 * v}
        T = rigid(0.1 * v, -0.07 * v, 0.3 + 0.05 * v, (100.0 + v, -20.0 * v, 300.0))
        views.append((label.reshape(H, W), depth.reshape(H, W), T, intr))
    return views, kinds


# ---- sort / grid build --------------------------------------------------------------------------------------------------------------------
def _uni(seed, n, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3))


def _thin(seed, n, xmax):
    p = _uni(seed, n, 0.0, 0.5)
    p[:, 0] = np.random.default_rng(seed + 1).uniform(0.0, xmax, n)
    return p


def _alternating(seed, n):
    p = _uni(seed, n, 0.0, 0.25)
    p[1::2, 0] += 1.25
    return p


def _wide(n, zdim, seed):
    """integer + 0.5 coordinates with a point at the origin and one at the far corner: cells per axis exactly 2^18, 2^18, zdim"""
    rng = np.random.default_rng(seed)
    far = np.array([(1 << 18) - 2, (1 << 18) - 2, zdim - 2], dtype=np.float64)
    p = np.floor(rng.uniform(0, 1, (n, 3)) * far) + 0.5
    p[0], p[1] = 0.0, far + 0.5
    return p


BEYOND_64_RUNS = (1 << 20) + 1                          # the size of the more-than-64-runs case (measured time)
SORT_CASES = {                                           # name -> (points, cell, exact, expected sort_form fields)
    "one_cell_16384": (lambda: _uni(1, 16384, 0.0, 0.5), 1.0, False, dict(runs=1, compact=True)),
    "two_cells_alternating_16384": (lambda: _alternating(2, 16384), 1.0, False, dict(runs=1, compact=True)),
    "rank_bits_4": (lambda: _thin(3, 2000, 3.0), 1.0, False, dict(rank_bits=4, dim=[4, 2, 2])),
    "rank_bits_5": (lambda: _thin(4, 2000, 4.0), 1.0, False, dict(rank_bits=5, dim=[5, 2, 2])),
    "rank_bits_7": (lambda: _uni(5, 3000, 0.0, 4.0), 1.0, False, dict(rank_bits=7, dim=[5, 5, 5])),
    "n1": (lambda: _uni(6, 1, 0.0, 10.0), 1.0, False, dict(runs=1)),
    "n2": (lambda: _uni(7, 2, 0.0, 10.0), 1.0, False, dict(runs=1)),
    "n1023": (lambda: _uni(8, 1023, 0.0, 10.0), 1.0, False, dict(runs=1)),
    "n1024": (lambda: _uni(9, 1024, 0.0, 10.0), 1.0, False, dict(runs=1)),
    "n1025": (lambda: _uni(10, 1025, 0.0, 10.0), 1.0, False, dict(runs=1)),
    "n32769_three_runs": (lambda: _uni(11, 32769, 0.0, 20.0), 1.0, False, dict(runs=3, compact=True)),
    "runs_share_cells_40000": (lambda: _uni(12, 40000, 0.0, 3.0), 1.0, False, dict(runs=3, compact=True, dim=[4, 4, 4])),
    "runs_64": (lambda: _uni(13, 1 << 20, 0.0, 100.0), 1.0, False, dict(runs=64, compact=True)),
    "cells_at_2^53": (lambda: _wide(1000, 1 << 17, 14), 1.0, True, dict(index_bits=10, rank_bits=53, compact=True)),
    "cells_above_2^53_general_n1000": (lambda: _wide(1000, (1 << 17) + 1, 15), 1.0, True, dict(index_bits=10, compact=False)),
    "beyond_64_runs": (lambda: _uni(16, BEYOND_64_RUNS, 0.0, 100.0), 1.0, False, dict(runs=65, compact=False)),
}
SORT_LARGE = ("runs_64", "beyond_64_runs")


def sort_case(name):
    make, cell, exact, want = SORT_CASES[name]
    return np.ascontiguousarray(make()), cell, exact, want


# ---- voxel down-sample --------------------------------------------------------------------------------------------------------------------
def _line(n):
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n)
    return p


VOXEL_CASES = {                                          # name -> (points, voxel, exact)
    "borders": (lambda: np.random.default_rng(20).integers(-8, 8, (300, 3)) * 0.25, 0.5, True),
    "one_point": (lambda: _uni(21, 1, -5.0, 5.0), 0.5, False),
    "identical_100": (lambda: np.tile(_uni(22, 1, -5.0, 5.0), (100, 1)), 0.5, False),
    "own_voxel_4095": (lambda: _line(4095), 0.5, True),
    "own_voxel_4096": (lambda: _line(4096), 0.5, True),
    "own_voxel_4097": (lambda: _line(4097), 0.5, True),
    "one_voxel_4095": (lambda: _uni(23, 4095, 0.0, 0.2), 1.0, False),
    "one_voxel_4096": (lambda: _uni(24, 4096, 0.0, 0.2), 1.0, False),
    "one_voxel_4097": (lambda: _uni(25, 4097, 0.0, 0.2), 1.0, False),
    "negative": (lambda: _uni(26, 500, -50.0, -10.0), 3.0, False),
}


def voxel_case(name):
    make, voxel, exact = VOXEL_CASES[name]
    return np.ascontiguousarray(make(), dtype=np.float64), voxel, exact


# ---- radius count + selection ---------------------------------------------------------------------------------------------------------------
_OUTSIDE = np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1], [3, 1, 1], [1, 3, 1], [1, 1, 3], [-10, 1, 1], [1, -10, 1], [1, 1, -10],
                     [12, 1, 1], [1, 12, 1], [1, 1, 12], [-0.25, -0.25, -0.25], [2.25, 2.25, 2.25]])
RADIUS_CASES = {                                         # name -> (points, radius = cell, queries (None: the cloud itself), exact)
    "lattice_d_eq_r": (lambda: shuffled(lattice(5, 5, 5), 30), 1.0, None, True),       # axis neighbours at exactly d == r: every count 1
    "lattice_r1.5": (lambda: shuffled(lattice(5, 5, 5), 31), 1.5, None, True),         # face and edge neighbours
    "duplicates": (lambda: shuffled(np.repeat(lattice(3, 3, 3), 3, axis=0), 32), 1.5, None, True),
    "nq1": (lambda: _uni(33, 1, 0.0, 2.0), 1.0, None, False),
    "nq8": (lambda: _uni(34, 8, 0.0, 2.0), 1.0, None, False),
    "nq9": (lambda: _uni(35, 9, 0.0, 2.0), 1.0, None, False),
    "one_point_grid": (lambda: np.array([[1.0, 1.0, 1.0]]), 1.5, np.array([[1.0, 1, 1], [2, 1, 1], [2.5, 1, 1], [1, 1, -0.25]]), True),
    "queries_outside": (lambda: shuffled(lattice(3, 3, 3), 36), 1.5, _OUTSIDE, True),
}


def radius_case(name):
    make, r, q, exact = RADIUS_CASES[name]
    return np.ascontiguousarray(make(), dtype=np.float64), r, q, exact


# ---- normals --------------------------------------------------------------------------------------------------------------------------------
def _clusters_224_225():
    rng = np.random.default_rng(40)
    return np.r_[rng.uniform(0, 0.5, (224, 3)), rng.uniform(0, 0.5, (225, 3)) + 100.0]    # every pair of a cluster is < radius 1 apart


def _few():
    rng = np.random.default_rng(41)
    return np.concatenate([rng.uniform(0, 0.3, (m, 3)) + 50.0 * m for m in (1, 2, 3, 4)])  # groups of 1, 2, 3, 4 points, far apart


def _coplanar():
    p = lattice(5, 4, 1)
    p[:, 0] += 0.25 * p[:, 1]
    p[:, 2] = 0.5
    return p


def _collinear():
    p = np.zeros((6, 3))
    p[:, 0] = 0.5 * np.arange(6)
    p[:, 1] = 0.25 * np.arange(6)
    return p


NORMAL_CASES = {   # name -> (points, radius, max_nns, exact, wrong rules that must cost, expected candidate counts or None)
    "cand_224_225": (_clusters_224_225, 1.0, (30, 64), False, ("max_nn+1", "max_nn-1"), (224, 225)),
    "tie_cut": (lambda: shuffled(lattice(5, 5, 5) @ SHEAR.T, 42), 2.5, (30, 64), True, ("high", "original", "max_nn+1", "max_nn-1"), None),
    "d_eq_r": (lambda: shuffled(lattice(5, 5, 5) @ SHEAR.T, 43), 1.25, (30,), True, ("inclusive",), None),
    "few_neighbours": (_few, 1.0, (30,), False, (), (1, 2, 3, 4)),
    "coplanar": (lambda: shuffled(_coplanar(), 44), 1.5, (30, 5), True, (), None),
    "collinear": (_collinear, 1.25, (30,), True, (), None),
    "coincident": (lambda: np.tile(np.array([[0.5, -0.25, 2.0]]), (10, 1)), 1.0, (30, 4), True, (), (10,)),
    "n1": (lambda: _uni(45, 1, 0.0, 1.0), 1.0, (30,), False, (), None),
    "n2": (lambda: _uni(46, 2, 0.0, 1.0), 1.0, (30,), False, (), None),
    "n7": (lambda: _uni(47, 7, 0.0, 1.0), 1.0, (30,), False, (), None),
    "n8": (lambda: _uni(48, 8, 0.0, 1.0), 1.0, (30,), False, (), None),
    "n9": (lambda: _uni(49, 9, 0.0, 1.0), 1.0, (30, 3), False, (), None),
}


@cached
def normal_case(name):
    make, r, max_nns, exact, rules, counts = NORMAL_CASES[name]
    pts = np.ascontiguousarray(make(), dtype=np.float64)
    return dict(pts=pts, radius=r, max_nns=max_nns, exact=exact, rules=rules, counts=counts, grid=R.grid(pts, r, r))


@cached
def normal_expected(name, max_nn):
    """per point (original order): (selection, cnt, C, eigenvalues ascending)"""
    c = normal_case(name)
    out = []
    for p in c["pts"]:
        sel = R.hybrid_selection(c["grid"], p, c["radius"], max_nn)
        if len(sel) < 3:
            out.append((sel, len(sel), None, None))
        else:
            cnt, _, C = R.covariance(c["grid"], sel)
            out.append((sel, cnt, C, np.linalg.eigvalsh(C)))
    return out


# ---- k-NN mean distance ---------------------------------------------------------------------------------------------------------------------
def _with_isolated():
    return np.r_[_uni(50, 50, 0.0, 1.0), [[100.0, 100.0, 100.0]]]


KNN_CASES = {      # name -> (points, cell, ks, exact, route that must occur (None: any))
    "settles_R1": (lambda: _uni(51, 1000, 0.0, 10.0), 2.0, (4,), False, 1),
    "settles_R2": (lambda: _uni(52, 1000, 0.0, 10.0), 1.0, (8,), False, 2),
    "settles_R3": (lambda: _uni(53, 1000, 0.0, 10.0), 0.5, (8,), False, 3),
    "overflow_first_block": (lambda: np.r_[_uni(54, 500, 0.0, 0.4), _uni(55, 20, 5.0, 9.0)], 1.0, (8,), False, "overflow"),
    "isolated_point": (_with_isolated, 1.0, (4,), False, "all"),
    "k1": (lambda: _uni(56, 100, 0.0, 3.0), 1.0, (1,), False, 1),
    "k_eq_n": (lambda: _uni(57, 40, 0.0, 2.0), 0.5, (40,), False, None),
    "k64": (lambda: _uni(58, 300, 0.0, 3.0), 1.0, (64,), False, None),
    "lattice_ties": (lambda: shuffled(lattice(5, 5, 5), 59), 1.0, (4, 7, 27), True, None),
    "duplicates": (lambda: shuffled(np.repeat(_uni(60, 30, 0.0, 2.0), 3, axis=0), 61), 1.0, (2, 3, 5), False, None),
}
for _n in (127, 128, 129, 255, 256, 257):               # all-points route: a cell far below the spacing, k >= 2 never fits a block
    KNN_CASES["all_points_n%d" % _n] = ((lambda n=_n: _uni(62 + n, n, 0.0, 1.0)), 2.0 ** -10, (3,), False, "all")


@cached
def knn_case(name):
    make, cell, ks, exact, route = KNN_CASES[name]
    pts = np.ascontiguousarray(make(), dtype=np.float64)
    return dict(pts=pts, cell=cell, ks=ks, exact=exact, route=route, grid=R.grid(pts, cell, cell))


# ---- statistical filter ---------------------------------------------------------------------------------------------------------------------
def stat_cases():
    """[(points, nb_neighbors, std_ratio, kept indices expected or None: from the restatement)]"""
    cube = lattice(2, 2, 2)                              # k = 4: every mean is (0 + 1 + 1 + 1) / 4: std 0, threshold = mean, none kept
    rng = np.random.default_rng(70)
    blob = np.r_[rng.uniform(0, 5, (200, 3)), rng.uniform(20, 30, (5, 3))]
    big = rng.uniform(0, 40, (300, 3))
    return [(cube, 4, 1.0, []), (np.array([[1.0, 2.0, 3.0]]), 20, 1.0, []), (blob, 8, float("nan"), []), (blob, 8, 1.0, None),
            (big, 5, 0.5, None), (blob[:60], 100, 2.0, None)]


# ---- moments / Mahalanobis / transform --------------------------------------------------------------------------------------------------------
MOMENT_SIZES = (1, 255, 256, 257, 131072, 131073)        # the 512-block cap turns the reduction into a grid-stride loop above 131072 rows


@cached
def moment_case(n):
    return np.random.default_rng(80 + n % 97).uniform(-300.0, 500.0, (n, 3))


def mahalanobis_clouds(count):
    rng = np.random.default_rng(81)
    sizes = [1, 255, 256, 257, 1000, 3, 64, 65, 2] + [10 + 7 * i for i in range(8)]
    return [rng.uniform(-10, 30, (n, 3)) for n in sizes[:count]], rng.uniform(-2, 2, (count, 12))


# ---- ICP: correspondence search -----------------------------------------------------------------------------------------------------------------
NN1_MAX_DIST, NN1_CELL = 0.5, 1.0
NN1_TARGET = np.array([[0.0, 0.0, 0.0], [5.75, 5.5, 5.5], [5.25, 5.5, 5.5],      # 1, 2: one cell, equally far from (5.5, 5.5, 5.5)
                       [9.25, 5.5, 5.5], [8.75, 5.5, 5.5],                        # 3, 4: two cells, 3 in the LATER one, equally far from (9, ..)
                       [12.0, 12.0, 12.0]])
NN1_QUERIES = np.array([[5.5, 5.5, 5.5], [9.0, 5.5, 5.5], [12.5, 12.0, 12.0], [12.0, 11.5, 12.0], [12.25, 12.0, 12.0],
                        [-3.0, 0, 0], [0, -3.0, 0], [0, 0, -3.0], [20.0, 12, 12], [12, 20.0, 12], [12, 12, 20.0], [-0.25, 0, 0], [0, 0, -0.25]])
NN1_EXPECT = [1, 3, -1, -1, 5, -1, -1, -1, -1, -1, -1, 0, 0]
NN1_ONE_TARGET = (np.array([[1.0, 2.0, 3.0]]), np.array([[1.25, 2.0, 3.0], [1.5, 2.0, 3.0], [1.0, 2.0, 2.75], [-5.0, 2.0, 3.0]]), [0, -1, 0, -1])

SUM_SIZES = (256, 257, 131072, 131073)


@cached
def sums_case(n):
    rng = np.random.default_rng(90 + n % 89)
    nt = 1000
    src, tgt = rng.uniform(-50, 80, (n, 3)), rng.uniform(-50, 80, (nt, 3))
    corr = rng.integers(-1, nt, n).astype(np.int32)
    corr[rng.random(n) < 0.1] = -1
    corr[0], corr[n - 1] = 7, -1
    return dict(src=src, tgt=tgt, tn=unit(nt, 91), corr=corr, d2=rng.uniform(0, 4, n))


# ---- ICP: exits of the step ---------------------------------------------------------------------------------------------------------------------
ICP_MAX_DIST = 0.5


def _pair(seed, nt, m, init, parallel_normals=False, copy=False):
    """a target of nt points and a source of which exactly m land within ICP_MAX_DIST of a target point once moved by `init`; the rest
    are 100 away"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(0, 10, (nt, 3))
    tn = np.tile([0.0, 0.0, 1.0], (nt, 1)) if parallel_normals else unit(nt, seed + 1)
    small = rigid(0.01, -0.008, 0.012, (0.02, -0.015, 0.01))
    moved = tgt.copy() if copy else (tgt - small[:3, 3]) @ small[:3, :3]
    moved[m:] += 100.0
    inv = np.linalg.inv(init)
    return dict(src=np.ascontiguousarray(moved @ inv[:3, :3].T + inv[:3, 3]), tgt=tgt, tn=tn, init=np.array(init, dtype=np.float64))


INIT = rigid(0.1, 0.2, 0.3, (1.0, 2.0, 3.0))
ICP_CASES = {      # name -> (kind, pair, (rel_fitness, rel_rmse, max_iteration), expect dict)
    "p2p_2_corr": (0, lambda: _pair(200, 12, 2, INIT), (1e-6, 1e-6, 30), dict(n_corr=2, status=2, updates=0, T_is_init=True)),
    "p2p_3_corr": (0, lambda: _pair(201, 12, 3, INIT), (0.0, 0.0, 1), dict(n_corr=3, status=3, updates=1)),
    "plane_5_corr": (1, lambda: _pair(202, 12, 5, INIT), (1e-6, 1e-6, 30), dict(n_corr=5, status=2, updates=0, T_is_init=True)),
    "plane_6_corr": (1, lambda: _pair(203, 12, 6, INIT), (0.0, 0.0, 1), dict(n_corr=6, status=3, updates=1)),
    "max_iteration_0": (0, lambda: _pair(204, 12, 12, INIT), (1e-6, 1e-6, 0), dict(n_corr=12, status=3, updates=0, T_is_init=True)),
    "max_iteration_1": (0, lambda: _pair(205, 12, 12, np.eye(4)), (0.0, 0.0, 1), dict(n_corr=12, status=3, updates=1)),
    "criteria_0_never_converge": (0, lambda: _pair(206, 20, 20, np.eye(4), copy=True), (0.0, 0.0, 4), dict(n_corr=20, status=3, updates=4)),
    "parallel_normals_singular": (1, lambda: _pair(207, 12, 10, INIT, parallel_normals=True), (0.0, 0.0, 2),
                                  dict(n_corr=10, status=3, updates=2, T_is_init=True)),
}


@cached
def icp_case(name):
    kind, make, crit, expect = ICP_CASES[name]
    return dict(kind=kind, crit=crit, expect=expect, **make())


def icp_expected(name):
    c = icp_case(name)
    return R.icp_run(c["kind"], c["src"], c["tgt"], c["tn"], ICP_MAX_DIST, ICP_MAX_DIST, c["init"], *c["crit"], n_iter=c["crit"][2])


# ---- the singular-covariance batch of get_surface_batch ---------------------------------------------------------------------------------------
def singular_views():
    """8 x 8 views for get_surface_batch(min_friends=0, min_dist=5, nb_neighbors=4, voxel_size=1): [0] a 5 x 4 block at constant depth
    seen through fx = fy = 1, ppx = ppy = 0 -- an integer lattice at constant z, covariance exactly singular; [2] one pixel -- zero
    covariance; the others generic.  -> (views, positions of the bad ones)"""
    rng = np.random.default_rng(300)
    flat = {"fx": 1.0, "fy": 1.0, "ppx": 0.0, "ppy": 0.0}
    generic = {"fx": 2.3, "fy": 2.1, "ppx": 3.6, "ppy": 4.2}
    views = []
    for v in range(5):
        label, depth = np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint16)
        if v == 0:
            label[1:6, 2:6], depth[:] = 255, 2
            views.append((label, depth, np.eye(4), flat))
        elif v == 2:
            label[3, 4], depth[:] = 1, 7
            views.append((label, depth, np.eye(4), flat))
        else:
            label[:], depth[:] = 1, rng.integers(4, 9, (8, 8))
            views.append((label, depth, rigid(0.1 * v, 0.2, -0.1, (5.0, v, 2.0)), generic))
    return views, (0, 2)

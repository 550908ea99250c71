"""Inputs, expected values and guards of the fast-global-registration tests (tests/test_fgr_host.py proves the guards on the CPU,
tests/test_gpu_fgr.py runs the kernels on the same inputs).  Expected values come from tests/fgr_reference.py, computed once per case.

Features are injected, not computed: row i of a feature set is (id_i, 0, ..., 0), so the nearest feature of a row is the row with the
nearest id, an equal id is an exact match at distance 0, and ties are equal ids.  The correspondence list of a pair always has three
entries per kept trial, so its length is a multiple of three: 255 and 258 bracket the optimisation kernel's 256 threads (255 leaves the
last thread idle, 258 gives two threads a second entry), 12 is the smallest list that is optimised and 3000 the largest the kernel holds."""
import functools

import numpy as np

import fgr_reference as F

BLOCK = 256                      # threads of the optimisation kernel's workgroup and of a tuple-test block
T_ATOL = 1e-9                    # transformations against the restatement (the project's bound for the registration kernels)
EVAL_MARGIN = 1e-7               # no evaluated distance this close to maximum_correspondence_distance: the counts are exact at T_ATOL
TUPLE_FILL = 300                 # a kept list this long fills after 405 trials of the base pair: inside the second block of a chunk
REVERSE_ATOL = 1e-10             # the restatement against itself with the list reversed: a case compared at T_ATOL must be this stable


def feature_rows(ids):
    f = np.zeros((len(ids), 33))
    f[:, 0] = np.asarray(ids, dtype=np.float64)
    return f


def rigid(deg=25.0, axis=(0.3, -0.5, 0.8), t=(0.7, -0.4, 0.5)):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def lattice_bump(nx=12, ny=12, nz=3):
    """an nx x ny x nz unit lattice whose z rises over a bump off the centre: no symmetry maps it onto itself"""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    g[:, 2] += 1.5 * np.exp(-((g[:, 0] - 4.0) ** 2 + (g[:, 1] - 7.0) ** 2) / 9.0)
    return g


def recover_case():
    """the host test's pair: exact one-to-one features, target = M . source"""
    src = lattice_bump()
    M = rigid()
    tgt = src @ M[:3, :3].T + M[:3, 3]
    ids = np.arange(len(src))
    return dict(src=src, tgt=tgt, fs=feature_rows(ids), ft=feature_rows(ids), M=M,
                opt=F.options(decrease_mu=True, maximum_correspondence_distance=1e-6))


@functools.lru_cache(maxsize=None)
def base_pair():
    """the lattice against its moved, slightly noisy, shuffled copy; every tenth source row carries another row's id, so its mutual match
    is a wrong pair that the tuple test has to refuse"""
    rng = np.random.default_rng(11)
    src = lattice_bump()
    n = len(src)
    M = rigid()
    perm = rng.permutation(n)                                   # target row j is source row perm[j]
    tgt = (src @ M[:3, :3].T + M[:3, 3])[perm] + rng.normal(0.0, 0.01, (n, 3))
    ids_s = np.arange(n)
    wrong = np.arange(0, n, 10)
    ids_s[wrong] = np.roll(wrong, 1)                            # swap ids among the wrong rows: still one-to-one, still mutual
    return dict(src=src, tgt=tgt, fs=feature_rows(ids_s), ft=feature_rows(perm), M=M, wrong=wrong)


def _opt_case(**kw):
    p = base_pair()
    return dict(src=p["src"], tgt=p["tgt"], fs=p["fs"], ft=p["ft"], opt=F.options(maximum_correspondence_distance=0.05, **kw))


def line_case():
    """all points on the x axis: q_y = q_z = 0 exactly, so JTJ[0][0] is an exact zero and the first pivot fails in the first iteration"""
    x = np.array([0.0, 1.0, 2.0, 4.0, 7.0, 8.0, 11.0, 13.0])
    src = np.stack([x, np.zeros(8), np.zeros(8)], 1)
    tgt = src + np.array([3.0, 0.0, 0.0])
    ids = np.arange(8)
    return dict(src=src, tgt=tgt, fs=feature_rows(ids), ft=feature_rows(ids), opt=F.options(maximum_correspondence_distance=0.5))


def triangle_case(tuple_scale):
    """source edges 1, sqrt 2, 1; the target is the source doubled: the edge pair (1, 2) with tuple_scale 0.5 gives 2 * 0.5 < 1, false"""
    src = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    ids = np.arange(3)
    return dict(src=src, tgt=2.0 * src, fs=feature_rows(ids), ft=feature_rows(ids), opt=F.options(tuple_scale=tuple_scale, maximum_correspondence_distance=0.5))


def small_pair():
    """five matches: 500 trials, most of them with a repeated draw.  The target is a rigid move plus 1e-2 noise, not an exact copy: the
    rmse of an exact copy is rounding noise and cannot be compared"""
    src = np.array([[0.0, 0, 0], [2.0, 0, 0], [0, 3.0, 0], [0, 0, 5.0], [1.0, 1.0, 1.0]])
    M = rigid(40.0)
    ids = np.arange(5)
    return dict(src=src, tgt=src @ M[:3, :3].T + M[:3, 3] + np.random.default_rng(3).normal(0.0, 1e-2, (5, 3)), fs=feature_rows(ids), ft=feature_rows(ids), opt=F.options(maximum_correspondence_distance=0.5))


def _pts(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


def matching_cases():
    """name -> (case, expected matches): the mutual filter's branches on hand-made ids"""
    nan = feature_rows([0, 1, 2])
    nan[:, 5] = np.nan
    return {
        # no source row has a finite distance: nn_st = -1 everywhere
        "ncorr0": (dict(src=_pts(3, 1), tgt=_pts(3, 2), fs=nan, ft=feature_rows([0, 1, 2]), opt=F.options()), np.zeros((0, 2), np.int64)),
        # one target: every source row points at it, it points back at the nearest (source 1)
        "ncorr1": (dict(src=_pts(3, 3), tgt=_pts(1, 4), fs=feature_rows([0, 5, 9]), ft=feature_rows([6]), opt=F.options()), np.array([[1, 0]])),
        # source 2 (id 4.4) points at target 1 (id 4), which points back at source 1 (id 4.1): broken in one direction only
        "one_way": (dict(src=_pts(3, 5), tgt=_pts(2, 6), fs=feature_rows([0, 4.1, 4.4]), ft=feature_rows([0, 4]), opt=F.options()),
                    np.array([[0, 0], [1, 1]])),
        # equal ids: sources 0 and 1 both point at target 0 (the lowest of the two copies), which points back at source 0 only
        "ties": (dict(src=_pts(3, 7), tgt=_pts(3, 8), fs=feature_rows([2, 2, 7]), ft=feature_rows([2, 2, 7]), opt=F.options()),
                 np.array([[0, 0], [2, 2]])),
    }


def optimisation_cases():
    """name -> case; every one is compared with the restatement at T_ATOL, so every one must pass the reversed-list check"""
    return {
        "n9_identity": _opt_case(maximum_tuple_count=3),
        "n12": _opt_case(maximum_tuple_count=4),
        "n255": _opt_case(maximum_tuple_count=85),
        "n258": _opt_case(maximum_tuple_count=86),
        "n3000": _opt_case(maximum_tuple_count=1000),
        "n255_absolute": _opt_case(maximum_tuple_count=85, use_absolute_scale=True),
        "n255_decrease": _opt_case(maximum_tuple_count=85, decrease_mu=True),
        "n255_absolute_decrease": _opt_case(maximum_tuple_count=85, use_absolute_scale=True, decrease_mu=True),
        "n255_floor": dict(_opt_case(maximum_tuple_count=85), opt=F.options(maximum_tuple_count=85, decrease_mu=True, maximum_correspondence_distance=2.0)),
        "n255_iter0": _opt_case(maximum_tuple_count=85, iteration_number=0),
        "n258_iter1": _opt_case(maximum_tuple_count=86, iteration_number=1),
        "n3000_iter1": _opt_case(maximum_tuple_count=1000, iteration_number=1),
        "line": line_case(),
        "small_never_full": small_pair(),
    }


CORR_COUNTS = {"n9_identity": 9, "n12": 12, "n255": 255, "n258": 258, "n3000": 3000, "n3000_iter1": 3000}
SINGLE_ITERATION = ("n258_iter1", "n3000_iter1")       # the sums of one iteration, through T at 1e-12 relative to T's largest entry


@functools.lru_cache(maxsize=None)
def expected(name):
    cases = optimisation_cases()
    c = cases[name] if name in cases else matching_cases()[name][0]
    return F.fgr(c["src"], c["tgt"], c["fs"], c["ft"], c["opt"])


@functools.lru_cache(maxsize=None)
def expected_reversed(name):
    c = optimisation_cases()[name]
    return F.fgr(c["src"], c["tgt"], c["fs"], c["ft"], c["opt"], reverse=True)


def check_guards(name):
    """every optimisation case reaches the branch its name says"""
    c, e = optimisation_cases()[name], expected(name)
    o = c["opt"]
    assert evaluation_margin(c, e["T"]) > EVAL_MARGIN
    if name in CORR_COUNTS:
        assert 3 * e["tuples"] == CORR_COUNTS[name] and e["tuples"] == o["maximum_tuple_count"]
    if name == "n9_identity":
        assert np.array_equal(e["T"], np.eye(4)) and e["iterations"] == 0
    elif name == "line":
        assert 3 * e["tuples"] >= 10 and e["iterations"] == 0 < o["iteration_number"] and e["pivots"] == [0.0]
        assert np.isfinite(e["T"]).all() and np.array_equal(e["T"][:3, :3], np.eye(3)) and np.array_equal(e["T"][:3, 3], [3.0, 0.0, 0.0])
    elif name == "small_never_full":
        assert 4 <= e["tuples"] < o["maximum_tuple_count"] and e["mutual"] == 5 and e["iterations"] == o["iteration_number"]
    else:
        assert 3 * e["tuples"] >= 10 and e["iterations"] == o["iteration_number"]
    if name.startswith("n") and name != "n9_identity":
        p = base_pair()
        assert e["mutual"] == len(p["src"])                                  # the wrong rows are mutual matches too ...
        used = e["matches"][F.draws(o["seed"], e["kept"], e["mutual"]).reshape(-1), 0]
        assert not np.isin(used, p["wrong"]).all()
        if o["iteration_number"] == 64:                                      # ... and the optimisation lands on the true motion all the same
            assert np.abs(e["T"] - p["M"]).max() < 0.05
    if name == "n255_floor":                                                 # par starts at 1, below the floor of 2: never divided
        assert e["par"] == 1.0 and np.array_equal(e["T"][:3, :3], expected("n255")["T"][:3, :3])
    if "decrease" in name:
        assert e["par"] < (e["scale"] if o["use_absolute_scale"] else 1.0)
    if "absolute" in name:
        assert e["scale"] > 5.0                                              # not the unit scale: the two settings differ
    if name.endswith("iter0"):
        assert np.array_equal(e["T"][:3, :3], np.eye(3)) and np.abs(e["T"][:3, 3]).max() > 0.1     # I in normalised units = the means' offset


def evaluation_margin(c, T):
    """the smallest | nearest distance - maximum_correspondence_distance | over the moved source points"""
    p = c["src"] @ T[:3, :3].T + T[:3, 3]
    d = np.sqrt(((p[:, None, :] - c["tgt"][None, :, :]) ** 2).sum(-1).min(1))
    return np.abs(d - c["opt"]["maximum_correspondence_distance"]).min()


def repeated_draws(seed, trials, ncorr):
    r = F.draws(seed, trials, ncorr)
    return (r[:, 0] == r[:, 1]) | (r[:, 1] == r[:, 2]) | (r[:, 2] == r[:, 0])


SHARED_CHUNK = (256, 1024)       # the tuple-test chunk schedule the lock-step test runs with: 256, 512, 1024, 1024, ... trials
# (source points, unmatched extra target points, share of source rows with another row's id, degrees, seed) or None: an empty cloud
SHARED_SPECS = ((432, 0, 0.1, 25.0, 0), (5, 3, 0.0, 40.0, 1), None, (64, 10, 0.0, 10.0, 2), (2, 0, 0.0, 5.0, 3), (12, 0, 0.0, 70.0, 4), (300, 50, 0.7, 25.0, 5),
                (3, 1, 0.0, 15.0, 6), (150, 0, 0.3, 120.0, 7), None, (4, 0, 0.0, 33.0, 8), (257, 7, 0.5, 60.0, 9), (1, 2, 0.0, 0.0, 10), (33, 0, 0.2, 45.0, 11),
                (100, 100, 0.0, 90.0, 12), (8, 0, 0.0, 12.0, 13), (432, 20, 0.6, 150.0, 14), (20, 5, 0.1, 80.0, 15), None, (6, 0, 0.0, 28.0, 16),
                (200, 0, 0.4, 100.0, 17), (16, 16, 0.0, 55.0, 18))


def _shared_pair(n, extra, wrong_share, deg, seed):
    rng = np.random.default_rng(100 + seed)
    src = lattice_bump()[np.sort(rng.choice(432, n, replace=False))]
    M = rigid(deg, axis=rng.standard_normal(3), t=rng.uniform(-2.0, 2.0, 3))
    perm = rng.permutation(n)
    tgt = np.concatenate([(src @ M[:3, :3].T + M[:3, 3])[perm] + rng.normal(0.0, 0.01, (n, 3)), rng.uniform(-20.0, 20.0, (extra, 3))])
    ids_s = np.arange(n)
    wrong = np.flatnonzero(rng.uniform(size=n) < wrong_share)
    if len(wrong) > 1:
        ids_s[wrong] = np.roll(wrong, 1)
    return dict(src=src, tgt=tgt, fs=feature_rows(ids_s), ft=feature_rows(np.concatenate([perm, 10000 + np.arange(extra)])),
                opt=F.options(maximum_correspondence_distance=0.05, seed=seed))


@functools.lru_cache(maxsize=None)
def shared_option_list():
    """more than 16 pairs with ONE option set (the seed apart), so that one group of batched.registration_fast spans two launches; they
    differ in cloud sizes, in ns != nt, in the number of mutual matches, in the length of the kept list and in the chunk at which the
    list fills or the pair runs out of trials; None: an empty cloud"""
    return tuple(None if sp is None else _shared_pair(*sp) for sp in SHARED_SPECS)


@functools.lru_cache(maxsize=None)
def shared_expected():
    return tuple(None if c is None else F.fgr(c["src"], c["tgt"], c["fs"], c["ft"], c["opt"]) for c in shared_option_list())


def chunk_index(trials, schedule=SHARED_CHUNK):
    """the 0-based chunk of the doubling schedule in which trial number `trials` (a count) is drawn"""
    k, done, c = 0, 0, schedule[0]
    while done + c < trials:
        done += c
        c = min(2 * c, schedule[1])
        k += 1
    return k


def batch_list():
    """names of more than 16 pairs (None: an empty cloud on one side or both) that differ in size, options and branch"""
    return [None, "n12", "ncorr0", "n255", "line", "ncorr1", "n258", None, "n255_absolute", "one_way", "n255_decrease", "ties", "n9_identity",
            "n255_iter0", "small_never_full", "n3000", "n258_iter1", None, "n255_floor", "n12"]

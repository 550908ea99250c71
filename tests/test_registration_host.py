"""CPU checks of the global registration (FPFH + RANSAC): the library exports its entry points (and no one-pair ones), the recorded
one-pair fixture is complete, the seeded sampler and the pair
feature of the restatement (tests/registration_reference.py) are pinned on hand-made values, the restatement's own invariants hold,
and unsupported checkers / estimators are refused before any device work."""
import ctypes
import math
import os

import numpy as np
import pytest

import registration_reference as R

_SYMS = ["ape_fpfh_batch_workspace_bytes", "ape_fpfh_batch_f64", "ape_feature_nn1_batch_workspace_bytes", "ape_feature_nn1_batch_f64",
         "ape_ransac_batch_workspace_bytes", "ape_ransac_hypotheses_batch_f64", "ape_ransac_validate_batch_f64"]
# the one-pair entry points that existed up to ABI 21: a single pair is a call of the ones above with nb = 1
_REMOVED = ["ape_fpfh_workspace_bytes", "ape_fpfh_f64", "ape_feature_nn1_workspace_bytes", "ape_feature_nn1_f64",
            "ape_ransac_workspace_bytes", "ape_ransac_hypotheses_f64", "ape_ransac_validate_f64"]


def test_library_exports_registration_and_abi_3():
    from autoposeestimation_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for s in _SYMS:
        assert hasattr(h, s), s
        assert s in _lib.SIGNATURES, s
    for s in _REMOVED:
        assert not hasattr(h, s), s
        assert s not in _lib.SIGNATURES, s
    h.ape_abi_version.restype = ctypes.c_int
    assert h.ape_abi_version() >= 3


def test_recorded_one_pair_fixture_holds_every_group_and_field():
    """what test_gpu_registration.py::test_one_pair_api_equals_the_recorded_parent reads is all there (tests/registration_golden.py)"""
    import registration_golden as G
    z = G.load()
    want = {G.key(g, case, f) for g, cases in G.GROUPS.items() for case, fields, _ in cases() for f in fields}
    assert len(want) > 100 and want <= set(z), sorted(want - set(z))
    assert set(z) - want == {"abi"} and int(z["abi"]) == 21          # recorded at the last ABI with one-pair entry points
    assert os.path.getsize(G.FIXTURE) < 300 * 1024
    assert z[G.key("ransac", "crit20000_17000_checkers0", "validated")].dtype == np.int64
    assert all(z[G.key("fpfh", c, "sha256")].shape == (32,) for c, _, _ in G.fpfh_group())


def test_splitmix64_sampler_values():
    # the standard splitmix64 sequence from state 0 (outputs 1..3)
    g = 0x9E3779B97F4A7C15
    assert R.splitmix64(0) == 0xE220A8397B1DCDAF
    assert R.splitmix64(g) == 0x6E789E6AA1B965F4
    assert R.splitmix64((2 * g) & ((1 << 64) - 1)) == 0x06C45D188009454F
    # the sampler built on it: splitmix64((seed << 32) ^ (i * ransac_n + j)) mod ns
    assert R.sample_indices(7, [0], 4, 1000)[0].tolist() == [489, 992, 685, 672]
    assert R.sample_indices(7, [123456], 4, 1000)[0].tolist() == [507, 655, 285, 440]
    assert R.sample_indices(0, [0], 4, 1 << 62)[0, 0] == 0xE220A8397B1DCDAF % (1 << 62)


def test_pair_feature_hand_cases():
    z = np.zeros(3)
    # parallel normals across a flat patch: every angle 0
    np.testing.assert_allclose(R.pair_features(z, [0, 0, 1], [1, 0, 0], [0, 0, 1]), [0, 0, 0, 1], atol=1e-15)
    # swap branch: the second normal is closer to the line -> n1/n2 swapped, d negated, f2 = -n2.d/|d|
    s = 1 / math.sqrt(2)
    np.testing.assert_allclose(R.pair_features(z, [0, 0, 1], [1, 0, 0], [s, 0, s]), [math.pi / 4, 0, -s, 1], atol=1e-15)
    # without the swap the same pair read the other way round: f2 = n1.d/|d|
    f = R.pair_features([1, 0, 0], [s, 0, s], z, [0, 0, 1])
    np.testing.assert_allclose(f[2:], [-s, 1], atol=1e-15)
    # zero cases: coincident points, and d parallel to the chosen normal (v = d x n1 = 0)
    assert np.all(R.pair_features(z, [0, 0, 1], z, [1, 0, 0]) == 0)
    assert np.all(R.pair_features(z, [0, 0, 1], [0, 0, 2], [0, 0, 1]) == 0)
    # a zero feature still lands in the middle bins (open3d adds it like any other)
    assert R.feature_bins(np.zeros(4)).tolist() == [5, 16, 27]


def _patch(n, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-30, 30, (n, 2))
    z = 4 * np.sin(xy[:, 0] / 7) * np.cos(xy[:, 1] / 9)
    p = np.c_[xy, z]
    gx = 4 / 7 * np.cos(xy[:, 0] / 7) * np.cos(xy[:, 1] / 9)
    gy = -4 / 9 * np.sin(xy[:, 0] / 7) * np.sin(xy[:, 1] / 9)
    nrm = np.c_[-gx, -gy, np.ones(n)]
    return p, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def _rigid(seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    th = 1.3
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    T[:3, 3] = [100.0, -40.0, 25.0]
    return T


def test_fpfh_restatement_invariants():
    p, nrm = _patch(600, 0)
    F = R.fpfh(p, nrm, 8.0, 100)
    lists = R.neighbour_lists(p, 8.0, 100)
    has = np.array([len(i) > 1 for i, _ in lists])
    assert has.any()
    sums = F.reshape(-1, 3, 11).sum(2)
    np.testing.assert_allclose(sums[has], 200.0, rtol=0, atol=1e-9)
    assert np.all(F[~has] == 0)
    T = _rigid(1)
    F2 = R.fpfh(p @ T[:3, :3].T + T[:3, 3], nrm @ T[:3, :3].T, 8.0, 100)
    np.testing.assert_allclose(F2, F, rtol=0, atol=1e-9)


def test_ransac_restatement_recovers_known_transform():
    p, nrm = _patch(500, 2)
    T = _rigid(3)
    q = p @ T[:3, :3].T + T[:3, 3]
    F = R.fpfh(p, nrm, 8.0, 100)
    Fq = R.fpfh(q, nrm @ T[:3, :3].T, 8.0, 100)
    res = R.ransac(p, q, F, Fq, 1.5, 4, 0, 0.9, 1.5, 20000, 50)
    assert len(res["kept"]) > 0 and np.all(np.diff(res["kept"]) > 0)
    assert res["fitness"] > 0.9
    np.testing.assert_allclose(res["T"], T, atol=1e-6)


def test_unsupported_checkers_and_estimators_are_refused():
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    f = PC.Feature(device="cpu")
    args = (None, None, f, f, 1.0)

    class CorrespondenceCheckerBasedOnNormal:
        normal_angle_threshold = 0.5

    with pytest.raises(NotImplementedError):
        PC.registration_ransac_based_on_feature_matching(*args, checkers=[CorrespondenceCheckerBasedOnNormal()])
    with pytest.raises(NotImplementedError):
        PC.registration_ransac_based_on_feature_matching(*args, estimation_method=PC.TransformationEstimationPointToPlane())
    with pytest.raises(NotImplementedError):
        PC.TransformationEstimationPointToPoint(with_scaling=True)
    # open3d's early exits: ransac_n < 3 or a non-positive distance -> the empty result
    for kw in ({"ransac_n": 2}, {}):
        r = PC.registration_ransac_based_on_feature_matching(None, None, f, f, 1.0 if kw else 0.0, **kw)
        assert np.array_equal(r.transformation, np.eye(4)) and r.fitness == 0.0 and r.inlier_rmse == 0.0
    assert f.dimension() == 33 and f.num() == 0 and f.data.shape == (33, 0)


# ---- the edge-shape cases of tests/registration_edge_cases.py: they build, hold their guards and reach the paths they are named for ------
import registration_edge_cases as EC  # noqa: E402


@pytest.mark.parametrize("name", list(EC.fpfh_cases()))
def test_fpfh_edge_case_builds_and_holds_its_margins(name):
    c = EC.fpfh_cases()[name]
    assert c["pts"].shape == c["normals"].shape == (len(c["pts"]), 3) and len(c["pts"]) <= 513
    bin_m, swap_m, seen = EC.fpfh_margins(name)
    if c["zero_only"]:
        assert seen == 0                                   # the one axis-aligned case: every pair feature is the all-zero one
    else:
        assert seen > 0 or len(c["pts"]) == 1
        assert bin_m >= EC.MARGIN and swap_m >= EC.MARGIN, (bin_m, swap_m)
        n = c["normals"]
        axis = (np.abs(n) == 1).any(1) & (np.abs(n).sum(1) == 1)
        assert not axis.any()
    for max_nn in c["max_nns"]:
        F = EC.fpfh_expected(name, max_nn)
        assert F.shape == (len(c["pts"]), 33) and np.isfinite(F).all()


def test_fpfh_edge_cases_reach_their_paths():
    cases = EC.fpfh_cases()
    # tie shells on the lattice: the 7 and 27 cuts fall between two entries of equal d^2 for some points, max_nn = 1 gives zeros
    for max_nn in (7, 27):
        inside = [len(d2) > max_nn and d2[max_nn - 1] == d2[max_nn] for _, d2 in EC.full_lists("lattice9_r2.5")]
        assert 0 < sum(inside)
    assert np.all(EC.fpfh_expected("lattice9_r2.5", 1) == 0)
    # radius exactly 2: there are pairs at d^2 == 4 and none is listed
    p = cases["lattice9_r2"]["pts"]
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1)
    assert (d2 == 4.0).sum() > 0 and all(d.max() < 4.0 for _, d in EC.full_lists("lattice9_r2"))
    assert (EC.candidate_counts("lattice9_r2") < EC.candidate_counts("lattice9_r2.5")).all()
    # 7x7x7, radius 6: both routes of the kernel (kFCand = 256) in one cloud
    nc = EC.candidate_counts("lattice7_r6")
    assert (nc > 256).sum() == 203 and (nc <= 256).sum() == 140
    # the clusters sit exactly on the two sides of the switch
    nc = EC.candidate_counts("clusters_256_257")
    assert np.all(nc[:256] == 256) and np.all(nc[256:] == 257)
    # coincident points: entry 0 is the lowest copy, not the point itself; max_nn = 3 leaves only d^2 == 0 entries
    lists = EC.full_lists("triples")
    later = [i for i, (idx, d) in enumerate(lists) if idx[0] != i]
    assert len(later) == 40 and all(lists[i][1][:3].tolist() == [0, 0, 0] for i in later)
    F3 = EC.fpfh_expected("triples", 3)
    assert all(np.flatnonzero(F3[i]).tolist() == [5, 16, 27] and np.all(F3[i, [5, 16, 27]] == 100.0) for i in later)
    # lists of length 1 (isolated point, n = 1, max_nn = 1) and 2
    assert EC.candidate_counts("isolated")[-1] == 1 and np.all(EC.fpfh_expected("isolated", 100)[-1] == 0)
    assert EC.candidate_counts("n1").tolist() == [1] and EC.candidate_counts("n2").tolist() == [2, 2]
    assert [len(cases["n%d" % n]["pts"]) for n in (1, 2, 7, 8, 9)] == [1, 2, 7, 8, 9]
    # vn == 0: zero features in the middle bins, so the FPFH is 200 in bins 5, 16 and 27
    F = EC.fpfh_expected("vn0_row", 100)
    want = np.zeros(33)
    want[[5, 16, 27]] = 200.0
    np.testing.assert_allclose(F, np.tile(want, (6, 1)), rtol=0, atol=1e-12)
    assert (np.abs(cases["zero_normals"]["normals"]).sum(1) == 0).sum() == 4
    names = EC.fpfh_batch_list()
    assert names[0] is None and len(names) > 17 and all(n in cases for n in names[1:])


@pytest.mark.parametrize("ns,nt", EC.MATCH_SHAPES)
def test_matching_edge_case_ties_resolve_to_the_lowest_index(ns, nt):
    fs, ft, planted = EC.matching_case(ns, nt)
    assert fs.shape == (ns, 33) and ft.shape == (nt, 33)
    nn = R.feature_nn(fs, ft)
    assert nn.min() >= 0 and nn.max() < nt
    assert planted or nt == 1
    for r, low in planted.items():
        d = ((ft - fs[r]) ** 2).sum(1)
        assert nn[r] == low and (d == d[low]).sum() >= 2 and np.flatnonzero(d == d[low])[0] == low
    if nt > 64:                                            # exact copies on both sides of the 64-row border (and of 128 where it exists)
        assert np.array_equal(ft[63], ft[64]) and 63 in planted.values() and (nt <= 128 or np.array_equal(ft[127], ft[128]))


def test_matching_nan_rule_of_the_restatement():
    c = EC.nan_case()
    nn = R.feature_nn(c["fs"], c["ft"])
    assert all(nn[r] == -1 for r in c["no_match"]) and (np.delete(nn, c["no_match"]) >= 0).all()
    assert not set(nn.tolist()) & set(c["nan_targets"]) and nn[4] == 1
    assert np.array_equal(R.feature_nn(np.full((2, 33), np.inf), c["ft"]), [-1, -1])
    kept = R.ransac_hypotheses(c["src"], c["tgt"], nn, 3, 5, -1.0, -1.0, 2000, 2000)
    drew = np.isin(R.sample_indices(5, np.arange(2000), 3, 130), c["no_match"]).any(1)
    assert drew.sum() > 20 and np.array_equal(kept, np.flatnonzero(~drew))


@pytest.mark.parametrize("ransac_n", [3, 4, 5, 16])
def test_hypothesis_cases_hold_their_threshold_guards(ransac_n):
    p = EC.ransac_pair()
    assert np.array_equal(R.feature_nn(p["fs"], p["ft"]), p["nn"])
    for it0 in (0, 12345):
        its = np.arange(it0, it0 + 1000)
        for edge, dist in EC.CHECKERS:
            rep = EC.hypothesis_report(p["src"], p["tgt"], p["nn"], ransac_n, 7, its, edge, dist)
            assert rep["edge_margin"].min() >= EC.MARGIN and rep["dist_margin"].min() >= EC.MARGIN
        kept = R.ransac_hypotheses(p["src"], p["tgt"], p["nn"], ransac_n, 7, EC.EDGE, EC.DIST, 200000, 5)
        assert len(kept) == 5
    if ransac_n == 3:                                      # three pairs: rank 2 at most, the u0 x u1 completion every time
        sig = EC.hypothesis_report(p["src"], p["tgt"], p["nn"], 3, 7, np.arange(1000))["sigma"]
        assert np.all(sig[:, 2] <= 1e-13 * sig[:, 0]) and EC.well_posed(sig).sum() > 900
    # without checkers every iteration passes: the kept list is the first max_validation iterations
    assert np.array_equal(R.ransac_hypotheses(p["src"], p["tgt"], p["nn"], ransac_n, 7, -1.0, -1.0, 1000, 257), np.arange(257))


def test_windowed_restatement_equals_the_reference_one():
    p = EC.ransac_pair()
    for rn, (edge, dist) in ((3, EC.CHECKERS[3]), (5, EC.CHECKERS[1]), (4, EC.CHECKERS[2]), (16, EC.CHECKERS[0])):
        want = R.ransac_hypotheses(p["src"], p["tgt"], p["nn"], rn, 7, edge, dist, 1000, 1000)
        assert np.array_equal(EC.hypotheses_in_range(p, rn, 7, edge, dist, 0, 1000), want)
    # the partly-filled-list case: both calls keep something
    assert len(EC.hypotheses_in_range(p, 3, 7, EC.EDGE, EC.DIST, 0, 600)) > 4 and len(EC.hypotheses_in_range(p, 3, 7, EC.EDGE, EC.DIST, 600, 600)) > 4
    want = R.ransac_hypotheses(p["src"], p["tgt"], p["nn"], 3, 7, EC.EDGE, EC.DIST, 65836, 65836)
    assert len(want) > 1000 and want[-1] >= 65536            # the 258-block call keeps iterations of its last two blocks
    rep = EC.hypothesis_report(p["src"], p["tgt"], p["nn"], 3, 7, np.arange(65836), EC.EDGE, EC.DIST)
    assert rep["edge_margin"].min() >= EC.MARGIN and rep["dist_margin"].min() >= EC.MARGIN


def test_tiny_cloud_cases_contain_rank_one_and_zero_covariances():
    for ns in (1, 2, 3):
        p = EC.tiny_pair(ns)
        assert p["src"].shape == (ns, 3) and p["tgt"].shape == (5, 3)
        for rn in (3, 4):
            for edge, dist in EC.CHECKERS:
                rep = EC.hypothesis_report(p["src"], p["tgt"], p["nn"], rn, 9, np.arange(500), edge, dist)
                assert rep["edge_margin"].min() >= EC.MARGIN and rep["dist_margin"].min() >= EC.MARGIN
            sig = rep["sigma"]
            zero = sig[:, 0] == 0
            rank1 = ~zero & (sig[:, 1] <= 1e-13 * sig[:, 0])
            assert zero.any() and (ns == 1 or rank1.any()) and (ns > 1 or zero.all())


@pytest.mark.parametrize("name", [r[0] for r in EC.WINNER_RUNS])
def test_winner_runs_hold_their_guards(name):
    w = EC.winner_run(name)
    want = w["want"]
    assert len(want["kept"]) > 0
    assert w["edge_margin"] >= EC.MARGIN and w["dist_margin"] >= EC.MARGIN and w["validation_margin"] >= EC.MARGIN
    if name == "nothing_matches":
        assert want["fitness"] == 0.0 and want["winner"] == -1 and np.array_equal(want["T"], np.eye(4))
        return
    assert want["winner"] >= 0 and EC.well_posed(w["sigma"]) and 0 < want["fitness"]
    if name == "far_target":                               # moved source points far beyond the target's cells, on both sides of the origin
        moved = R._apply(want["T"], w["pair"]["src"])
        lo, hi = w["pair"]["tgt"].min(0), w["pair"]["tgt"].max(0)
        assert (moved < lo - 10 * w["max_dist"]).any() and (moved > hi + 10 * w["max_dist"]).any() and want["fitness"] <= 0.2
    else:                                                  # not decided by rounding noise: the runner-up is clearly behind
        assert want["fitness"] > 0.9
        np.testing.assert_allclose(want["T"], w["pair"]["T"], atol=0.1)


def test_exact_threshold_case():
    p = EC.exact_pair()
    want = EC.ransac_from_nn(p["src"], p["tgt"], p["nn"], p["max_dist"], 3, 21, EC.EDGE, -1.0, 64, 64)
    s = R.sample_indices(21, want["kept"], 3, 2)
    assert len(want["kept"]) >= 2 and np.all(s == s[:, :1]) and set(s[:, 0].tolist()) == {0, 1}   # one-point draws only, of both points
    first = int(s[0, 0])
    T = np.eye(4)
    T[:3, 3] = p["tgt"][first] - p["src"][first]
    assert np.array_equal(want["T"], T) and want["winner"] == want["kept"][0]                    # equal (fitness, rmse): the first stands
    assert (want["fitness"], want["rmse"], want["count"]) == (0.5, 0.0, 1)
    other = p["src"][1 - first] + T[:3, 3]
    assert ((p["tgt"][1 - first] - other) ** 2).sum() == p["max_dist"] ** 2                      # exactly on the threshold: not counted
    assert R.evaluate(p["src"], p["tgt"], T, np.nextafter(p["max_dist"], 6.0))[2] == 2

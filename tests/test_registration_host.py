"""CPU checks of the global registration (FPFH + RANSAC): the library exports its entry points, the seeded sampler and the pair
feature of the restatement (tests/registration_reference.py) are pinned on hand-made values, the restatement's own invariants hold,
and unsupported checkers / estimators are refused before any device work."""
import ctypes
import math
import os

import numpy as np
import pytest

import registration_reference as R

_SYMS = ["ape_fpfh_workspace_bytes", "ape_fpfh_f64", "ape_feature_nn1_workspace_bytes", "ape_feature_nn1_f64",
         "ape_ransac_workspace_bytes", "ape_ransac_hypotheses_f64", "ape_ransac_validate_f64"]


def test_library_exports_registration_and_abi_3():
    from autoposeestimation_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for s in _SYMS:
        assert hasattr(h, s), s
        assert s in _lib.SIGNATURES, s
    h.ape_abi_version.restype = ctypes.c_int
    assert h.ape_abi_version() >= 3


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

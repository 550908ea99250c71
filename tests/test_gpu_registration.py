"""GPU checks of the global registration (csrc/registration.hip through pc_reconstruction.pointcloud / open3d_utils): FPFH, feature
matching, the RANSAC hypothesis list and the winner against the numpy restatement (tests/registration_reference.py, fed the device's
own normals), reproducibility, an end-to-end recovery of a large known motion, the drivers with global_regression=True, and the one-pair
API against the bits recorded from its former own implementation (tests/golden/registration_one_pair.npz)."""
import math
import os

import numpy as np
import pytest
import torch

import registration_golden as G
import registration_reference as R
from test_gpu_pointcloud import INTR, _render, _rot

pytestmark = pytest.mark.gpu
CENTRE = np.array([400.0, -20.0, 150.0])
VOXEL = 5.0


def _object(n, seed):
    """an asymmetric bumpy ellipsoid (semi-axes 105 / 72 / 52 mm) around CENTRE"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = 1 + 0.12 * np.sin(3 * v[:, 0] + 0.5) * np.cos(4 * v[:, 1]) + 0.08 * np.sin(5 * v[:, 2] + 1.0) + 0.05 * np.cos(7 * v[:, 0] * v[:, 1])
    return v * r[:, None] * np.array([105.0, 72.0, 52.0]) + CENTRE


def _camera(ang_x, ang_y):
    cam = _rot(math.pi, 0.0, 0.0, tuple(CENTRE + [0, 0, 600.0]))
    return _rot(0, 0, 0, tuple(CENTRE)) @ _rot(ang_x, ang_y, 0.0, (0, 0, 0)) @ _rot(0, 0, 0, tuple(-CENTRE)) @ cam


def _view(cloud, cam, voxel=VOXEL):
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    depth = _render(cloud, cam)
    label = (depth != 0).astype(np.uint8) * 255
    return PC.surface_points(label, depth, INTR, cam).voxel_down_sample(voxel)


def _axis_rot(axis, deg, t):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    T[:3, 3] = t
    return T


_CACHE = {}


def _pair():
    """two rendered, voxelised views (target, source); the source moved by 110 deg about an oblique axis + 100 mm.  Returns
    (target pts, source pts, M) with source = M . view2"""
    if "pair" not in _CACHE:
        cloud = _object(400000, 5)
        tgt = np.array(_view(cloud, _camera(0.0, 0.0)).points)
        src = np.array(_view(cloud, _camera(0.15, -0.2)).points)
        c = src.mean(0)
        M = _rot(0, 0, 0, tuple(c)) @ _axis_rot([0.4, -0.7, 0.6], 110.0, [0.0, 0.0, 100.0]) @ _rot(0, 0, 0, tuple(-c))
        src = src @ M[:3, :3].T + M[:3, 3]
        _CACHE["pair"] = (tgt, src, M)
    return _CACHE["pair"]


def _jittered(pts, seed):
    return pts + np.random.default_rng(seed).normal(0.0, 1e-3, pts.shape)


def _with_features(pts):
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    pc = PC.PointCloud(pts)
    pc.estimate_normals(PC.KDTreeSearchParamHybrid(radius=2 * VOXEL, max_nn=30))
    f = PC.compute_fpfh_feature(pc, PC.KDTreeSearchParamHybrid(radius=5 * VOXEL, max_nn=100))
    return pc, f


def _parity_clouds():
    if "parity" not in _CACHE:
        tgt, src, _ = _pair()
        tgt, src = _jittered(tgt, 1), _jittered(src, 2)
        pt, ft = _with_features(tgt)
        ps, fs = _with_features(src)
        _CACHE["parity"] = (ps, fs, pt, ft)
    return _CACHE["parity"]


def test_fpfh_and_matching_match_restatement():
    ps, fs, pt, ft = _parity_clouds()
    assert 1500 <= len(ps) <= 4000 and 1500 <= len(pt) <= 4000, (len(ps), len(pt))
    for pc, f in ((ps, fs), (pt, ft)):
        want = R.fpfh(np.array(pc.points), np.array(pc.normals), 5 * VOXEL, 100)
        got = f.data.T
        assert f.dimension() == 33 and f.num() == len(pc) and f.data.shape == (33, len(pc))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    # neighbour lists longer than the kernel's LDS candidate list (creases / dense spots) take the re-walk route: exercise it too
    want = R.fpfh(np.array(ps.points), np.array(ps.normals), 10 * VOXEL, 128)
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    got = PC.compute_fpfh_feature(ps, PC.KDTreeSearchParamHybrid(radius=10 * VOXEL, max_nn=128)).data.T
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    nn = PC.feature_nn(fs, ft).cpu().numpy()
    assert np.array_equal(nn, R.feature_nn(fs.data.T, ft.data.T))


@pytest.mark.parametrize("max_iteration,max_validation", [(1000, 1000), (200000, 500)])
def test_ransac_matches_restatement(max_iteration, max_validation):
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    ps, fs, pt, ft = _parity_clouds()
    thr = 1.5 * VOXEL
    checkers = [PC.CorrespondenceCheckerBasedOnEdgeLength(0.9), PC.CorrespondenceCheckerBasedOnDistance(thr)]
    crit = PC.RANSACConvergenceCriteria(max_iteration, max_validation)
    got = PC.registration_ransac_based_on_feature_matching(ps, pt, fs, ft, thr, PC.TransformationEstimationPointToPoint(False), 4,
                                                           checkers, crit, seed=3)
    want = R.ransac(np.array(ps.points), np.array(pt.points), fs.data.T, ft.data.T, thr, 4, 3, 0.9, thr, max_iteration, max_validation)
    assert len(want["kept"]) > 0
    assert np.array_equal(got.validated, want["kept"])
    assert got.fitness == want["fitness"] and got.correspondence_count == want["count"]
    assert abs(got.inlier_rmse - want["rmse"]) <= 1e-12 * max(want["rmse"], 1e-300)
    np.testing.assert_allclose(got.transformation, want["T"], rtol=0, atol=1e-9)
    again = PC.registration_ransac_based_on_feature_matching(ps, pt, fs, ft, thr, PC.TransformationEstimationPointToPoint(False), 4,
                                                             checkers, crit, seed=3)
    assert np.array_equal(again.transformation, got.transformation) and again.fitness == got.fitness


def _angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))


def test_icp_regression_with_global_registration_recovers_large_motion():
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    tgt, src, M = _pair()
    want = np.linalg.inv(M)                      # maps the moved source back onto the target's frame
    _, _, T = U.icp_regression(PC.PointCloud(tgt), PC.PointCloud(src), voxel_size=VOXEL, threshold=10, global_regression=True,
                               icp_point2point=True, icp_point2plane=True)
    assert _angle_deg(T[:3, :3], want[:3, :3]) < 1.0
    probe = src.mean(0)
    assert np.linalg.norm((T[:3, :3] @ probe + T[:3, 3]) - (want[:3, :3] @ probe + want[:3, 3])) < 2.0
    _, _, T0 = U.icp_regression(PC.PointCloud(tgt), PC.PointCloud(src), voxel_size=VOXEL, threshold=10, global_regression=False,
                                icp_point2point=True, icp_point2plane=True)
    assert _angle_deg(T0[:3, :3], want[:3, :3]) > 10.0
    # both ICP stages off: the RANSAC transformation itself
    _, _, Tg = U.icp_regression(PC.PointCloud(tgt), PC.PointCloud(src), voxel_size=VOXEL, threshold=10, global_regression=True,
                                icp_point2point=False, icp_point2plane=False)
    assert _angle_deg(Tg[:3, :3], want[:3, :3]) < 10.0


def test_global_registration_edge_cases():
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    ps, fs, pt, ft = _parity_clouds()
    thr = 1.5 * VOXEL
    checkers = [PC.CorrespondenceCheckerBasedOnEdgeLength(0.9), PC.CorrespondenceCheckerBasedOnDistance(thr)]
    # empty clouds
    e = PC.PointCloud()
    fe = PC.compute_fpfh_feature(e, PC.KDTreeSearchParamHybrid(radius=25, max_nn=100))
    assert fe.num() == 0
    for a, fa, b, fb in ((e, fe, pt, ft), (ps, fs, e, fe)):
        r = PC.registration_ransac_based_on_feature_matching(a, b, fa, fb, thr, None, 4, checkers, PC.RANSACConvergenceCriteria(1000, 10))
        assert np.array_equal(r.transformation, np.eye(4)) and r.fitness == 0.0
    # max_validation = 1: the first passing iteration, validated alone
    r = PC.registration_ransac_based_on_feature_matching(ps, pt, fs, ft, thr, None, 4, checkers, PC.RANSACConvergenceCriteria(200000, 1), seed=5)
    want = R.ransac_hypotheses(np.array(ps.points), np.array(pt.points), R.feature_nn(fs.data.T, ft.data.T), 4, 5, 0.9, thr, 200000, 1)
    assert len(want) == 1 and r.validated.tolist() == want.tolist() and r.iterations == int(want[0]) + 1
    # every source feature matched to one target point: no edge survives the length check -> identity, fitness 0
    flat = PC.Feature(torch.zeros(len(pt), 33, dtype=torch.float64, device="cuda"))
    r = PC.registration_ransac_based_on_feature_matching(ps, pt, fs, flat, thr, None, 4, checkers, PC.RANSACConvergenceCriteria(20000, 100))
    assert len(r.validated) == 0 and r.fitness == 0.0 and np.array_equal(r.transformation, np.eye(4))
    # the reference-shaped call with preprocess_point_cloud's None features
    down, feat = U.preprocess_point_cloud(PC.PointCloud(np.array(ps.points)), VOXEL)
    assert feat is None
    r = U.execute_global_registration(down, pt, None, ft, VOXEL)
    assert r.transformation.shape == (4, 4)


def test_drivers_with_global_regression(tmp_path):
    from autoposeestimation_amd.label_generator.create_labels import create_pose_label
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    from autoposeestimation_amd.pc_reconstruction.create_pointcloud import load_point_cloud
    from test_gpu_label_dirs import _make_tree
    root, obj = str(tmp_path), "ball"
    _make_tree(root, obj, 8)
    save_dir = os.path.join(root, "pc_reconstruction/data")
    out = load_point_cloud(obj, save_dir, root, mode="pred", n_viewpoints=4, min_friends=20, min_dist=5, nb_neighbors=20, threshold=10,
                           voxel_size=2, voxel_size_out=5, global_regression=True, icp_point2point=True, icp_point2plane=False,
                           rng=np.random.default_rng(1))
    for f in ("foreground.ply", obj + "_out.ply", obj + ".ply", obj + ".xyz"):
        assert os.path.exists(os.path.join(save_dir, obj, f)), f
    assert len(out) > 1000
    assert create_pose_label(root, obj, True, True, False) == 8
    tgt, src, _ = _pair()
    merged = U.align_point_clouds([PC.PointCloud(tgt), PC.PointCloud(src)], 10, 10, 5, global_regression=True, voxel_size=VOXEL, threshold=10)
    assert len(merged) > 0


@pytest.mark.parametrize("group", list(G.GROUPS))
def test_one_pair_api_equals_the_recorded_parent(group):
    """The one-pair functions are one-element calls into batched.py; the fixture holds what their own implementation (ABI 21, the seven
    one-pair entry points) returned for the same seeded inputs on an MI355X.  float64 kernels with fixed summation orders: exact."""
    want = G.load()
    for case, fields, run in G.GROUPS[group]():
        got = run()
        for f in fields:
            a, w = np.asarray(got[f]), want[G.key(group, case, f)]
            assert a.dtype == w.dtype and a.shape == w.shape and np.array_equal(a, w), (group, case, f)

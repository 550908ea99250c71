"""GPU checks of the lock-step global registration (pc_reconstruction/batched.py over the entry points of csrc/registration.hip): FPFH,
feature matching and RANSAC for many clouds / pairs per launch must equal the same cloud / pair as a batch of one bit for bit -- which is
what the one-pair API (pc_reconstruction.pointcloud) is: a one-element call of the same list functions, seeded and reproducible, so the
comparison is exact.  What it tests is that a result does not depend on the pair's slot, its neighbours, the chunk at which it fills its
validation list or its part of the shared workspace (that a batch of one still gives what the former one-pair implementation gave is
test_gpu_registration.py::test_one_pair_api_equals_the_recorded_parent); then the two lock-step stages and fuse_chains with
global_regression=True against their sequential forms."""
import numpy as np
import pytest
import torch

import registration_reference as R
from test_gpu_registration import VOXEL, _camera, _jittered, _object, _pair, _view, _with_features

pytestmark = pytest.mark.gpu
THR = 1.5 * VOXEL
_CACHE = {}


def _mods():
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    return B, U, PC


def _cut(pts, m, seed):
    """about m points of a cached cloud: strided, cut, jittered"""
    k = max(1, len(pts) // m)
    return _jittered(pts[::k][:m], seed)


def _with_normals(pts):
    _, _, PC = _mods()
    pc = PC.PointCloud(pts)
    pc.estimate_normals(PC.KDTreeSearchParamHybrid(radius=2 * VOXEL, max_nn=30))
    return pc


def _parity():
    """the (source, its features, target, its features) of the parity pair, computed once by the one-cloud API and never modified"""
    if "parity" not in _CACHE:
        tgt, src, _ = _pair()
        pt, ft = _with_features(_jittered(tgt, 1))
        ps, fs = _with_features(_jittered(src, 2))
        _CACHE["parity"] = (ps, fs, pt, ft)
    return _CACHE["parity"]


def test_fpfh_in_a_batch_equals_each_cloud_alone():
    B, _, PC = _mods()
    tgt, src, _ = _pair()
    sizes = [1000, 1400, 3000, 1700, 2200, 1100, 2600, 1900, 1300, 2900, 1500, 2400, 1200, 2000, 2800, 1600]
    clouds = [PC.PointCloud(), _with_normals(_cut(tgt, 1, 3)), _with_normals(_cut(src, 300, 4))]
    clouds += [_with_normals(_cut(tgt if i % 2 else src, m, 10 + i)) for i, m in enumerate(sizes)]
    assert len(clouds) == 19 and len(clouds[1]) == 1 and 250 <= len(clouds[2]) <= 400
    assert all(1000 <= len(c) <= 3000 for c in clouds[3:]), [len(c) for c in clouds]
    for radius, max_nn in ((5 * VOXEL, 100), (10 * VOXEL, 128)):          # the second: more than 256 in-radius candidates, the re-walk route
        got = B.compute_fpfh_feature(clouds, radius, max_nn)
        assert len(got) == 19 and got[0].num() == 0
        for c, f in zip(clouds, got):
            want = PC.compute_fpfh_feature(c, PC.KDTreeSearchParamHybrid(radius=radius, max_nn=max_nn))
            assert f.t.shape == (len(c), 33) and torch.equal(f.t, want.t), len(c)
        assert float(got[-1].t.abs().sum()) > 0


def test_matching_in_a_batch_equals_each_pair_alone():
    B, _, PC = _mods()
    _, fs, _, ft = _parity()
    n = min(2500, fs.num(), ft.num())
    assert n >= 1500
    f = lambda feat, m: PC.Feature(feat.t[:m].contiguous())  # noqa: E731
    pairs = [(f(fs, 0), f(ft, n)), (f(fs, n), f(ft, 0)), (f(fs, 1), f(ft, 1)), (f(fs, 300), f(ft, n)), (f(fs, n), f(ft, 300)), (f(fs, n), f(ft, n))]
    tie = (f(fs, 500), PC.Feature(torch.cat([ft.t[:600], ft.t[:600]], 0).contiguous()))       # every target row twice: exact ties
    pairs.append(tie)
    got = B.feature_nn([p[0] for p in pairs], [p[1] for p in pairs])
    assert len(got) == len(pairs)
    for (a, b), nn in zip(pairs, got):
        want = PC.feature_nn(a, b)
        assert nn.dtype == torch.int32 and nn.shape == (a.num(),) and torch.equal(nn, want), (a.num(), b.num())
    tie_nn = got[-1].cpu().numpy()
    assert np.array_equal(tie_nn, R.feature_nn(tie[0].data.T, tie[1].data.T)) and tie_nn.max() < 600


def _ransac_alone(PC, pair, seed, crit):
    ps, pt, fs, ft = pair
    checkers = [PC.CorrespondenceCheckerBasedOnEdgeLength(0.9), PC.CorrespondenceCheckerBasedOnDistance(THR)]
    return PC.registration_ransac_based_on_feature_matching(ps, pt, fs, ft, THR, PC.TransformationEstimationPointToPoint(False), 4, checkers,
                                                            PC.RANSACConvergenceCriteria(*crit), seed=seed)


def _ransac_batch(B, PC, pairs, seeds, crit):
    return B.registration_ransac([p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs], [p[3] for p in pairs], THR, 4, 0.9, THR,
                                 PC.RANSACConvergenceCriteria(*crit), seeds)


def _same_result(a, b):
    return (np.array_equal(a.transformation, b.transformation) and a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and
            a.correspondence_count == b.correspondence_count and np.array_equal(a.validated, b.validated) and a.validated.dtype == b.validated.dtype and
            a.iterations == b.iterations)


def test_ransac_pairs_that_finish_at_different_chunks():
    B, _, PC = _mods()
    ps, fs, pt, ft = _parity()
    crit = (200000, 50)
    M = np.linalg.inv(_pair()[2])
    copy = PC.PointCloud(np.array(pt.points) @ M[:3, :3].T + M[:3, 3])
    flat = PC.Feature(torch.zeros(len(pt), 33, dtype=torch.float64, device="cuda"))
    e = PC.PointCloud()
    fe = PC.Feature(device="cuda")
    A = (copy, pt, ft, ft)                   # an exact rigid copy with identical features: every iteration passes, full in the first chunk
    Bp = (ps, pt, fs, ft)                    # the parity pair
    C = (ps, pt, fs, flat)                   # every source matched to target 0: nothing passes, runs to max_iteration
    D = (e, pt, fe, ft)                      # an empty source
    pairs, seeds = [A, Bp, C, D, Bp], [0, 1, 2, 3, 4]
    alone = [_ransac_alone(PC, p, s, crit) for p, s in zip(pairs, seeds)]
    assert len(alone[0].validated) == 50 and alone[0].iterations <= 16384 and alone[0].fitness == 1.0
    assert len(alone[2].validated) == 0 and alone[2].iterations == 200000
    assert len(alone[3].validated) == 0 and alone[3].iterations == 0 and len(alone[1].validated) > 0
    got = _ransac_batch(B, PC, pairs, seeds, crit)
    for k, (g, w) in enumerate(zip(got, alone)):
        assert _same_result(g, w), k
    # a full batch of 16 with the parity pair in its first and last slot, then the same pairs in another order
    full = [Bp, A, C, Bp, A, C, D, Bp, A, C, Bp, A, C, A, C, Bp]
    fseeds = [1, 0, 2, 4, 5, 6, 3, 7, 8, 9, 10, 11, 12, 13, 14, 1]
    res = _ransac_batch(B, PC, full, fseeds, crit)
    assert len(res) == 16 and _same_result(res[0], alone[1]) and _same_result(res[15], alone[1]) and _same_result(res[3], alone[4])
    assert _same_result(res[1], alone[0]) and _same_result(res[2], alone[2]) and _same_result(res[6], alone[3])
    perm = [15, 4, 9, 0, 13, 2, 7, 11, 6, 1, 14, 3, 8, 12, 5, 10]
    res_p = _ransac_batch(B, PC, [full[j] for j in perm], [fseeds[j] for j in perm], crit)
    for k, j in enumerate(perm):
        assert _same_result(res_p[k], res[j]), (k, j)
    # one slot against the numpy restatement, as test_gpu_registration.test_ransac_matches_restatement
    got = _ransac_batch(B, PC, [A, Bp, C], [0, 3, 2], (1000, 1000))[1]
    want = R.ransac(np.array(ps.points), np.array(pt.points), fs.data.T, ft.data.T, THR, 4, 3, 0.9, THR, 1000, 1000)
    assert len(want["kept"]) > 0
    assert np.array_equal(got.validated, want["kept"])
    assert got.fitness == want["fitness"] and got.correspondence_count == want["count"]
    assert abs(got.inlier_rmse - want["rmse"]) <= 1e-12 * max(want["rmse"], 1e-300)
    np.testing.assert_allclose(got.transformation, want["T"], rtol=0, atol=1e-9)


def test_ransac_batch_argument_checks():
    B, _, PC = _mods()
    ps, fs, pt, ft = _parity()
    crit = PC.RANSACConvergenceCriteria(1000, 10)
    with pytest.raises(ValueError):
        B.registration_ransac([ps], [pt], [fs], [ft], THR, 17, 0.9, THR, crit, [0])
    with pytest.raises(ValueError):
        B.registration_ransac([ps], [pt], [fs], [ft], THR, 4, 0.9, THR, PC.RANSACConvergenceCriteria(1000, 65536), [0])
    with pytest.raises(ValueError):
        B.registration_ransac([ps], [pt], [PC.Feature(fs.t[:-1].contiguous())], [ft], THR, 4, 0.9, THR, crit, [0])
    r = B.registration_ransac([ps], [pt], [fs], [ft], THR, 2, 0.9, THR, crit, [0])[0]
    assert np.array_equal(r.transformation, np.eye(4)) and r.fitness == 0.0 and r.iterations == 0 and len(r.validated) == 0
    from autoposeestimation_amd import _lib
    assert _lib.lib().ape_fpfh_batch_f64(17, *([None] * 5), 1.0, None, None, 1.0, 10, None, None, 0, None) == -1          # nb beyond kMaxBatch
    assert _lib.lib().ape_feature_nn1_batch_f64(0, None, None, None, None, None, None, 0, None) == -1


def _icp_pairs():
    tgt, src, _ = _pair()
    return [(tgt, src), (_cut(tgt, len(tgt) // 2, 21), _cut(src, len(src) // 2, 22)), (_jittered(tgt[:1500], 23), _cut(src, len(src) // 3, 24))]


@pytest.mark.parametrize("stages", [True, False])
def test_icp_regression_batch_with_global_regression(stages):
    B, U, PC = _mods()
    pairs = _icp_pairs()
    assert len({len(t) for t, _ in pairs}) == 3
    got = B.icp_regression_batch([PC.PointCloud(t) for t, _ in pairs], [PC.PointCloud(s) for _, s in pairs], VOXEL, 10, icp_point2point=stages,
                                 icp_point2plane=stages, global_regression=True)
    assert len(got) == 3
    for (t, s), T in zip(pairs, got):
        want = U.icp_regression(PC.PointCloud(t), PC.PointCloud(s), voxel_size=VOXEL, threshold=10, global_regression=True, icp_point2point=stages,
                                icp_point2plane=stages)[2]
        assert np.array_equal(T, want), (len(t), len(s))
    assert not np.array_equal(got[0], np.eye(4))


def test_fuse_surfaces_batch_with_global_regression():
    B, U, PC = _mods()
    cloud = _object(200000, 7)
    views = [np.array(_view(cloud, _camera(ax, ay)).points) for ax, ay in ((0.0, 0.0), (0.15, -0.2), (-0.2, 0.15))]
    assert all(1200 <= len(v) <= 4000 for v in views), [len(v) for v in views]
    shapes = [[views[0], views[1], views[2]], [views[2], views[0]], [np.zeros((0, 3))]]
    mk = lambda: [[PC.PointCloud(p) if len(p) else PC.PointCloud() for p in ch] for ch in shapes]  # noqa: E731
    got = B.fuse_surfaces_batch(mk(), voxel_size=VOXEL, threshold=10, global_regression=True)
    assert len(got) == 3 and got[2][0] is None and got[2][1] == [None]
    for ch, (acc, tfs) in zip(mk()[:2], got[:2]):
        want_acc, want_tfs = U.fuse_surfaces(ch, voxel_size=VOXEL, threshold=10, global_regression=True)
        assert len(tfs) == len(want_tfs) and all(np.array_equal(a, b) for a, b in zip(tfs, want_tfs))
        assert torch.equal(acc._p, want_acc._p) and len(acc) > len(ch[0])


def test_fuse_chains_with_global_regression_takes_the_lock_step_route(monkeypatch):
    from autoposeestimation_amd import synthetic as S
    B, U, _ = _mods()
    cloud = S.bumpy_sphere(120000, 21)
    chains = [S.label_views(3, seed=c, cloud=cloud) for c in range(2)]
    assert all(v[0].shape == (480, 640) for ch in chains for v in ch)
    calls = []
    inner = B.registration_ransac

    def counted(*a, **k):
        calls.append(len(a[0]))
        return inner(*a, **k)

    monkeypatch.setattr(B, "registration_ransac", counted)
    kw = dict(voxel_size=2, threshold=10, icp_point2point=True, icp_point2plane=False, global_regression=True)
    assert U.USE_BATCHED
    got = U.fuse_chains(chains, S.LABEL_INTR, **kw)
    assert len(calls) >= 1 and max(calls) == 2                # the lock-step route: both chains' registrations in one call
    n_calls = len(calls)
    monkeypatch.setattr(U, "USE_BATCHED", False)
    want = U.fuse_chains(chains, S.LABEL_INTR, **kw)
    assert len(calls) > n_calls and set(calls[n_calls:]) == {1}      # the sequential route: further registrations, every one a batch of one
    assert sorted(got) == sorted(want) == [0, 1]
    for c in (0, 1):
        assert torch.equal(got[c][0]._p, want[c][0]._p) and len(got[c][0]) > 500
        assert len(got[c][1]) == 3 and all(np.array_equal(a, b) for a, b in zip(got[c][1], want[c][1]))

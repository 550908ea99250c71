"""GPU checks of fast global registration (the fgr_* kernels of csrc/registration.hip behind pointcloud.
registration_fast_based_on_feature_matching and batched.registration_fast) against the numpy restatement tests/fgr_reference.py on the
inputs of tests/fgr_cases.py, whose guards tests/test_fgr_host.py proves on the CPU.

Bounds, the project's own for the registration kernels: match lists, kept lists, counts, fitness and iterations exact; transformations
atol 1e-9; rmse 1e-12 relative; the transformation after ONE iteration (the 27 sums and one solve) 1e-12 relative to its largest entry.

Sizes: 432-point clouds at most; the optimisation kernel's workgroup has 256 threads and a correspondence list is a multiple of three
long, so the lists are 12, 255, 258 and 3000 entries long (9: the identity)."""
import numpy as np
import pytest
import torch

import fgr_cases as C
import fgr_reference as F

pytestmark = pytest.mark.gpu
_D = torch.float64


def _mods():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    return _lib, B, PC


def _dev(a, dtype=_D):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def _inputs(c):
    _, _, PC = _mods()
    opt = None if c["opt"] == F.options() else PC.FastGlobalRegistrationOption(**c["opt"])
    return PC.PointCloud(c["src"]), PC.PointCloud(c["tgt"]), PC.Feature(_dev(c["fs"])), PC.Feature(_dev(c["ft"])), opt


def _run(c):
    _, _, PC = _mods()
    return PC.registration_fast_based_on_feature_matching(*_inputs(c))


def _check(got, want, single_iteration=False):
    assert np.array_equal(got.matches, want["matches"]) and got.mutual == want["mutual"]
    assert np.array_equal(got.kept, want["kept"]) and got.tuples == want["tuples"]
    assert got.iterations == want["iterations"]
    T = got.transformation
    assert T.shape == (4, 4) and np.isfinite(T).all() and np.array_equal(T[3], [0, 0, 0, 1])
    err = np.abs(T - want["T"]).max()
    print("max |T - T_ref| = %.3e" % err)
    assert err <= C.T_ATOL
    if single_iteration:                                     # relative to T's largest entry, not entry by entry
        assert err <= 1e-12 * np.abs(want["T"]).max()
    assert got.fitness == want["fitness"] and got.correspondence_count == want["count"]
    assert abs(got.inlier_rmse - want["rmse"]) <= 1e-12 * max(want["rmse"], 1e-300)


def _same(a, b):
    return (np.array_equal(a.transformation, b.transformation) and a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse
            and a.correspondence_count == b.correspondence_count and np.array_equal(a.matches, b.matches) and np.array_equal(a.kept, b.kept)
            and (a.mutual, a.tuples, a.iterations) == (b.mutual, b.tuples, b.iterations))


# ---- mutual matches -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.matching_cases()))
def test_mutual_matches(name):
    """ncorr = 0 (no finite distance), ncorr = 1, a match broken in one direction only, ties to the lowest index"""
    c, want = C.matching_cases()[name]
    got = _run(c)
    assert np.array_equal(got.matches, want)
    _check(got, C.expected(name))
    assert np.array_equal(got.transformation, np.eye(4)) and got.tuples == 0 and got.iterations == 0


def test_mutual_list_through_a_block_border_with_guarded_buffers():
    """the base pair's 432 matches cross the 256-thread step of the one-block compaction; the entries behind the count stay untouched"""
    _lib, B, PC = _mods()
    p = C.base_pair()
    nn_st, nn_ts = F.feature_nn(p["fs"], p["ft"]), F.feature_nn(p["ft"], p["fs"])
    nn_st[300] = 7                                           # one broken match past the border: the list has a gap there
    want = F.mutual_matches(nn_st, nn_ts)
    assert len(want) == 431 and 300 not in want[:, 0]
    a, b = _dev(nn_st, torch.int32), _dev(nn_ts, torch.int32)
    ms = torch.full((440,), -7, dtype=torch.int32, device="cuda")
    mt = torch.full((440,), -7, dtype=torch.int32, device="cuda")
    n = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    _lib.call.ape_fgr_mutual_batch(1, B._ptrs([a]), B._ints([432]), B._ptrs([b]), B._ints([432]), B._ptrs([ms]), B._ptrs([mt]), _lib.dptr(n[1:]),
                                   _lib.stream_ptr())
    assert n.cpu().tolist() == [-7, 431, -7]
    ms, mt = ms.cpu().numpy(), mt.cpu().numpy()
    assert np.array_equal(ms[:431], want[:, 0]) and np.array_equal(mt[:431], want[:, 1]) and (ms[431:] == -7).all() and (mt[431:] == -7).all()


# ---- the tuple test -------------------------------------------------------------------------------------------------------------------
def _tuples(c, matches, calls, max_tuples, seed=0):
    """ape_fgr_tuples_batch_f64 for every (trial_begin, n_trials) of `calls` onto one kept list -> the kept trials (host); the entries
    behind the count, and the words around the list and the counter, must be untouched"""
    _lib, B, _ = _mods()
    L = _lib.lib()
    s, t = _dev(c["src"]), _dev(c["tgt"])
    ms, mt = _dev(matches[:, 0], torch.int32), _dev(matches[:, 1], torch.int32)
    n_mutual = _dev(np.array([len(matches)]), torch.int32)
    kept = torch.full((max_tuples + 2,), -7, dtype=torch.int32, device="cuda")
    n_kept = torch.tensor([-7, 0, -7], dtype=torch.int32, device="cuda")
    for t0, n_t in calls:
        ws = torch.empty(L.ape_fgr_workspace_bytes(1, n_t), dtype=torch.uint8, device="cuda")
        _lib.call.ape_fgr_tuples_batch_f64(1, B._ptrs([s]), B._ints([len(c["src"])]), B._ptrs([t]), B._ints([len(c["tgt"])]), B._ptrs([ms]),
                                           B._ptrs([mt]), _lib.dptr(n_mutual), B._longs([seed]), float(c["opt"]["tuple_scale"]), t0, n_t,
                                           max_tuples, _lib.dptr(kept[1:]), _lib.dptr(n_kept[1:]), _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    nk = n_kept.cpu().tolist()
    out = kept.cpu().numpy()
    assert nk[0] == -7 and nk[2] == -7 and 0 <= nk[1] <= max_tuples
    assert out[0] == -7 and np.all(out[1 + nk[1]:] == -7)
    return out[1:1 + nk[1]].astype(np.int64)


def test_tuple_list_fills_inside_a_chunk_at_a_chunk_border_and_never():
    p = C.base_pair()
    c = dict(p, opt=F.options())
    m = F.mutual_matches(F.feature_nn(p["fs"], p["ft"]), F.feature_nn(p["ft"], p["fs"]))
    want = F.kept_trials(p["src"], p["tgt"], m, 0, 0.95, C.TUPLE_FILL)
    last = int(want[-1]) + 1                                 # trials drawn when the list fills (405: inside a chunk's second block)
    # in the middle of a chunk; the chunk after it is a no-op although it holds passing trials
    assert np.array_equal(_tuples(c, m, [(0, 1024), (1024, 1024)], C.TUPLE_FILL), want)
    # exactly at a chunk border, and the same list from chunks of odd sizes
    assert np.array_equal(_tuples(c, m, [(0, last), (last, 1024)], C.TUPLE_FILL), want)
    assert np.array_equal(_tuples(c, m, [(0, 1), (1, 255), (256, 1), (257, last - 257 - 1), (last - 1, 1), (last, 300)], C.TUPLE_FILL), want)
    assert np.array_equal(_tuples(c, m, [(0, last - 1)], C.TUPLE_FILL), want[:-1])
    # never: the five-match pair stops at its own 100 * ncorr = 500 trials, inside a chunk that goes on
    s = C.small_pair()
    e = C.expected("small_never_full")
    got = _tuples(s, e["matches"], [(0, 300), (300, 724), (1024, 256)], 1000)
    assert np.array_equal(got, e["kept"]) and 0 < len(got) < 1000
    assert not C.repeated_draws(0, got, 5).any()             # no kept trial drew a match twice


@pytest.mark.parametrize("tuple_scale,passes", [(0.5, False), (0.49, True)])
def test_tuple_test_is_strict_at_the_boundary(tuple_scale, passes):
    """edge lengths 1 and 2 with tuple_scale 0.5: 2 * 0.5 < 1 is false, so no trial passes; at 0.49 every trial without a repeated draw does"""
    c = C.triangle_case(tuple_scale)
    got = _run(c)
    want = F.fgr(c["src"], c["tgt"], c["fs"], c["ft"], c["opt"])
    assert got.mutual == 3 and np.array_equal(got.kept, want["kept"]) and (got.tuples > 0) == passes
    if passes:
        assert np.array_equal(got.kept, np.flatnonzero(~C.repeated_draws(0, np.arange(300), 3)))


# ---- the optimisation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.optimisation_cases()))
def test_registration_matches_restatement(name):
    """lists of 9 (identity), 12, 255, 258 and 3000 correspondences; use_absolute_scale and decrease_mu on and off; par below the floor;
    zero iterations and one; a failing pivot (all points on one line); a list that never fills"""
    c, want = C.optimisation_cases()[name], C.expected(name)
    got = _run(c)
    _check(got, want, single_iteration=name in C.SINGLE_ITERATION)
    if name == "n9_identity":
        assert np.array_equal(got.transformation, np.eye(4))
    if name == "line":
        assert got.iterations == 0 < c["opt"]["iteration_number"] and np.array_equal(got.transformation[:3, 3], [3.0, 0.0, 0.0])
    if name == "n255_floor":                                 # par never moves: the decrease_mu run equals the plain one bit for bit
        assert np.array_equal(got.transformation, _run(C.optimisation_cases()["n255"]).transformation)
    assert _same(got, _run(c))                               # the same call twice


def test_options_are_validated():
    _, _, PC = _mods()
    c = C.optimisation_cases()["n12"]
    s, t, fs, ft, _ = _inputs(c)
    with pytest.raises(ValueError):
        PC.registration_fast_based_on_feature_matching(s, t, fs, ft, PC.FastGlobalRegistrationOption(maximum_tuple_count=1001))
    with pytest.raises(ValueError):
        PC.registration_fast_based_on_feature_matching(s, t, fs, PC.Feature(_dev(c["ft"][:-1])))
    r = PC.registration_fast_based_on_feature_matching(s, t, fs, ft, PC.FastGlobalRegistrationOption(maximum_tuple_count=0))
    assert r.tuples == 0 and np.array_equal(r.transformation, np.eye(4)) and r.mutual == 432


# ---- lock step ------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_each_pair_alone():
    """20 pairs -- empty clouds, every matching branch, every list length, both scales, a failing pivot -- passed as one list: each result
    is the one-pair call's bit for bit.  These pairs differ in their options, so registration_fast splits them into many small groups
    (no launch holds more than four of them): this is the grouping's test; the lock step of one group over two launches is the next one"""
    _, B, PC = _mods()
    names = C.batch_list()
    assert len(names) > 16 and names.count(None) == 3
    cases = dict(C.optimisation_cases())
    cases.update({k: v[0] for k, v in C.matching_cases().items()})
    args, k = [], 0
    for nm in names:
        if nm is None:                                       # empty source, empty target, both
            src = PC.PointCloud() if k != 1 else PC.PointCloud(C.small_pair()["src"])
            tgt = PC.PointCloud() if k != 0 else PC.PointCloud(C.small_pair()["tgt"])
            args.append((src, tgt, PC.Feature(_dev(np.zeros((len(src), 33)))), PC.Feature(_dev(np.zeros((len(tgt), 33)))), None))
            k += 1
        else:
            args.append(_inputs(cases[nm]))
    got = B.registration_fast(*[list(x) for x in zip(*args)])
    assert len(got) == len(names)
    for nm, a, g in zip(names, args, got):
        alone = PC.registration_fast_based_on_feature_matching(*a)
        assert _same(g, alone), nm
        if nm is None:
            assert np.array_equal(g.transformation, np.eye(4)) and (g.fitness, g.correspondence_count, g.mutual, g.tuples) == (0.0, 0, 0, 0)
    i = names.index("n3000")
    np.testing.assert_allclose(got[i].transformation, C.expected("n3000")["T"], rtol=0, atol=C.T_ATOL)


def test_one_option_set_across_two_launches_equals_each_pair_alone(monkeypatch):
    """19 live pairs with ONE option set (seeds apart) and three empty clouds between them: one group of batched.registration_fast, so a
    launch of 16 pairs and a launch of 3.  The pairs differ in cloud sizes (1 to 432 points, ns != nt), mutual matches, kept-list length
    (0 to 1000: lists of every length share one LDS size) and in the chunk at which they stop -- the batch runs the tuple test in chunks of
    256, 512, 1024, ... trials, so that full pairs, exhausted pairs and pairs still drawing share launches.  Each result equals the
    one-pair call's (default chunks) bit for bit, and the restatement's lists exactly and transformation at 1e-9."""
    _, B, PC = _mods()
    cases, want = C.shared_option_list(), C.shared_expected()
    args, e = [], 0
    for k, c in enumerate(cases):
        if c is None:                                        # empty source, empty target, both
            src = PC.PointCloud() if e != 1 else PC.PointCloud(C.small_pair()["src"])
            tgt = PC.PointCloud() if e != 0 else PC.PointCloud(C.small_pair()["tgt"])
            e += 1
            args.append((src, tgt, PC.Feature(_dev(np.zeros((len(src), 33)))), PC.Feature(_dev(np.zeros((len(tgt), 33)))),
                         PC.FastGlobalRegistrationOption(maximum_correspondence_distance=0.05)))
        else:
            args.append(_inputs(c))
    alone = [PC.registration_fast_based_on_feature_matching(*a) for a in args]
    monkeypatch.setattr(PC, "_FGR_CHUNK", C.SHARED_CHUNK)
    got = B.registration_fast(*[list(x) for x in zip(*args)])
    assert len(got) == len(cases)
    for k, (c, g, a, w) in enumerate(zip(cases, got, alone, want)):
        assert _same(g, a), k
        if c is None:
            assert np.array_equal(g.transformation, np.eye(4)) and (g.mutual, g.tuples, g.iterations, g.correspondence_count) == (0, 0, 0, 0)
            continue
        assert np.array_equal(g.matches, w["matches"]) and np.array_equal(g.kept, w["kept"]) and g.iterations == w["iterations"], k
        np.testing.assert_allclose(g.transformation, w["T"], rtol=0, atol=C.T_ATOL, err_msg=str(k))


def test_list_lengths_and_iteration_number_are_checked_up_front():
    _, B, PC = _mods()
    s, t, fs, ft, _ = _inputs(C.optimisation_cases()["n12"])
    with pytest.raises(ValueError):
        B.registration_fast([s, s], [t, t], [fs, fs], [ft, ft], [None])
    with pytest.raises(ValueError):
        B.registration_fast([s], [t, t], [fs], [ft], [None])
    with pytest.raises(ValueError):
        PC.registration_fast_based_on_feature_matching(s, t, fs, ft, PC.FastGlobalRegistrationOption(iteration_number=-1))


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------
def _angle_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1) / 2
    return float(np.degrees(np.arccos(max(-1.0, min(1.0, c)))))


def test_icp_regression_with_fgr_recovers_the_large_motion():
    """the 110-degree pair of tests/test_gpu_registration.py through icp_regression(global_regression=True, global_method='fgr'): within the
    bounds that test sets for the RANSAC route (1 degree, 2 mm at the cloud's centre); the batched driver gives the same transformation"""
    import test_gpu_registration as TR
    _, B, PC = _mods()
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    tgt, src, M = TR._pair()
    want = np.linalg.inv(M)
    _, _, T = U.icp_regression(PC.PointCloud(tgt), PC.PointCloud(src), voxel_size=TR.VOXEL, threshold=10, global_regression=True,
                               icp_point2point=True, icp_point2plane=True, global_method="fgr")
    probe = src.mean(0)
    ang = _angle_deg(T[:3, :3], want[:3, :3])
    off = float(np.linalg.norm((T[:3, :3] @ probe + T[:3, 3]) - (want[:3, :3] @ probe + want[:3, 3])))
    print("fgr route: %.4f deg, %.4f mm" % (ang, off))
    assert ang < 1.0 and off < 2.0
    Tb = B.icp_regression_batch([PC.PointCloud(tgt)], [PC.PointCloud(src)], TR.VOXEL, 10, True, True, global_regression=True, global_method="fgr")[0]
    assert np.array_equal(Tb, T)

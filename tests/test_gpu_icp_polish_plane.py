"""The point-to-plane depth ICP polish (ape_icp_polish_plane_batch_f64, csrc/icp_polish.hip kPointToPlane) against the
project's oracle (oracle/pointcloud_oracle.py:registration_icp(point_to_plane=True) through icp_polish_plane_cases.reference, on the
normals read back from the ModelSet), against the existing device ICP (ape_icp_run_batch_f64, kind 1, on the same normals), and wired
into FramePipeline; and the point-to-point export against the bits the parent commit's library gave.

Bars: correspondences, fitness and stop reason exactly; |d rmse| <= 1e-12 + 1e-9 rmse; pose and T within T_ATOL absolute.
T_ATOL = max(10 x measured, 1e-12), where `measured` is the largest |dT| / |d pose| between the two references that existed before the
kernel -- the oracle and batched.registration_icp(kind=1) -- on these seven pairs at N = 1000 and N = 500, taken at the parent commit
on an MI355X: MEASURED_REFERENCE_GAP below (the factor of ten: the kernel adds a summation order of its own to the two compared).
Ten times the measured 9.9e-16 is below the floor, so T_ATOL = 1e-12, a thousandth of the 1e-9 of the point-to-point tests.  The kernel
itself stands at |d pose| <= 6.9e-16 and |dT| <= 1.4e-15 against either reference, the iteration-limit cases included (same date, same
machine)."""
import os

import numpy as np
import pytest
import torch

import icp_polish_cases as C
import icp_polish_plane_cases as P
from conftest import REPO

pytestmark = pytest.mark.gpu
MEASURED_REFERENCE_GAP = 9.853e-16    # 2026-10-21; per pair 2.6e-16 .. 9.9e-16 (`three`: 0, no update), the same at both N
T_ATOL = max(10 * MEASURED_REFERENCE_GAP, 1e-12)
OBJECTS, CLASS_OF_M = P.OBJECTS, P.CLASS_OF_M
PLANE = "point_to_plane"
GOLDEN = os.path.join(REPO, "tests", "golden", "icp_polish_p2p_bits.npz")


class Criteria:
    relative_fitness, relative_rmse, max_iteration = C.CRITERIA


@pytest.fixture(scope="module")
def cases():
    return P.cases()


@pytest.fixture(scope="module")
def clouds():
    """the four classes of the cases and, behind a hole at index 4 (a class of the table with M = 0), a fifth"""
    out = P.clouds()
    out[5] = C.model(63, 1)[0]
    return out


@pytest.fixture(scope="module")
def models(clouds):
    from autoposeestimation_amd.pipeline.polish import ModelSet
    return ModelSet(clouds, "cuda", C.MAX_DIST, normal_radius=P.NORMAL_RADIUS, normal_max_nn=P.NORMAL_MAX_NN)


@pytest.fixture(scope="module")
def normals(models):
    """the normals the kernel reads, read back: the references get exactly these"""
    return {k: n.cpu().numpy() for k, n in models.normals.items()}


def _launch(models, items, N, pad="wrap", min_fitness=0.0, classes=None, criteria=Criteria, estimation=PLANE):
    """items = [(case, n_cand or None, pose or None)] -> (pose_out [n,7], stats [n,4], points4 [n,N,4], n_cand [n]) as numpy"""
    from autoposeestimation_amd import engine as E
    p4 = np.stack([C.points4(c["obs"], N, nc, pad) for c, nc, _ in items])
    n_cand = np.array([len(c["obs"]) if nc is None else nc for c, nc, _ in items], np.int32)
    pose = np.stack([c["pose"] if p is None else p for c, _, p in items])
    cls = [CLASS_OF_M[len(c["model"])] for c, _, _ in items] if classes is None else classes
    out, stats = E.icp_polish(torch.from_numpy(p4).cuda(), torch.from_numpy(n_cand).cuda(), cls, models, torch.from_numpy(pose).cuda(), C.MAX_DIST,
                              criteria, min_fitness, estimation)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy(), p4, n_cand


def _plain(cases):
    return [(c, None, None) for c in cases]


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def launched(models, cases):
    """the 7-object launch at N = 1000 and N = 500, computed once and left unchanged"""
    return {N: _launch(models, _plain(cases), N) for N in P.SIZES}


@pytest.fixture(scope="module")
def references(cases, launched, normals):
    """the oracle on what the kernel is given: the float32 points widened to float64, the ModelSet's normals"""
    out = {}
    for N, (_, _, p4, n_cand) in launched.items():
        out[N] = [P.reference(s, c["model"], normals[CLASS_OF_M[len(c["model"])]], c["pose"]) for s, c in zip(P.sources(p4, n_cand, N), cases)]
    return out


def _check(pose, stats, want_pose, want_stats, want_T, tag):
    fit, rmse, n, reason = want_stats
    got_T = C.rigid_inverse(C.pose_matrix(pose))
    print("%s: corr %d/%d fit %.6f/%.6f reason %d/%d |d rmse| %.3e |d pose| %.3e |d T| %.3e" % (
        tag, stats[2], n, stats[0], fit, stats[3], reason, abs(stats[1] - rmse), np.abs(pose - want_pose).max(), np.abs(got_T - want_T).max()))
    assert stats[2] == n and stats[0] == fit and stats[3] == reason, tag
    assert abs(stats[1] - rmse) <= 1e-12 + 1e-9 * rmse, tag
    assert np.abs(pose - want_pose).max() <= T_ATOL, tag
    assert np.abs(got_T - want_T).max() <= T_ATOL, tag
    assert pose[0] >= 0


def test_the_model_set_keeps_its_normals(models, clouds, normals):
    from autoposeestimation_amd.pipeline.polish import ModelSet
    assert sorted(models.normals) == [0, 1, 2, 3, 5] and models.n_classes == 6
    assert models.flat_normals == {0: 0, 1: 0, 2: 3, 3: 0, 5: models.flat_normals[5]}
    table = models.normals_table.cpu().numpy()
    assert table[4] == 0 and all(table[k] == models.normals[k].data_ptr() for k in models.normals)
    for k, n in normals.items():
        assert n.shape == clouds[k].shape and n.dtype == np.float64 and np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-12
        assert int((n == (0.0, 0.0, 1.0)).all(1).sum()) == models.flat_normals[k]
    plain = ModelSet(clouds, "cuda", C.MAX_DIST)
    assert plain.normals is None and plain.flat_normals is None and plain.normals_table is None
    given = ModelSet(clouds, "cuda", C.MAX_DIST, normals=normals)
    assert all(np.array_equal(given.normals[k].cpu().numpy(), normals[k]) for k in normals) and given.flat_normals == models.flat_normals
    a = ModelSet.cached(clouds, "cuda", C.MAX_DIST, normal_radius=P.NORMAL_RADIUS)
    assert ModelSet.cached(clouds, "cuda", C.MAX_DIST, normal_radius=P.NORMAL_RADIUS) is a
    assert ModelSet.cached(clouds, "cuda", C.MAX_DIST, normal_radius=0.01) is not a
    assert ModelSet.cached(clouds, "cuda", C.MAX_DIST) is not a and ModelSet.cached(clouds, "cuda", C.MAX_DIST).normals is None
    b = ModelSet.cached(clouds, "cuda", C.MAX_DIST, normals=normals)
    assert b is not a and ModelSet.cached(clouds, "cuda", C.MAX_DIST, normals=normals) is b
    assert ModelSet.cached(clouds, "cuda", C.MAX_DIST, normals=dict(normals)) is not b


def test_point_to_plane_needs_normals(clouds, cases):
    from autoposeestimation_amd.pipeline.polish import ModelSet
    with pytest.raises(ValueError, match="needs a ModelSet with normals"):
        _launch(ModelSet(clouds, "cuda", C.MAX_DIST), _plain(cases), 1000)


@pytest.mark.parametrize("N", P.SIZES)
def test_parity_with_the_oracle(launched, references, cases, N):
    pose, stats, _, n_cand = launched[N]
    assert int(n_cand.max()) > 500 and int(n_cand.min()) == 3
    for i, (want_pose, want_stats, want_T) in enumerate(references[N]):
        _check(pose[i], stats[i], want_pose, want_stats, want_T, "%s N=%d" % (OBJECTS[i], N))
    assert (stats[2, 0], stats[2, 2], stats[2, 3]) == (1.0, 3.0, 2.0) and np.array_equal(pose[2], cases[2]["pose"])      # `three`: 3 points, no update
    assert set(np.delete(stats[:, 3], 2).astype(int)) == {1}


@pytest.mark.parametrize("N", P.SIZES)
def test_parity_with_the_existing_device_icp(launched, cases, models, N):
    """batched.icp_states (ape_icp_run_batch_f64, kind 1: three launches per iteration) on the same pairs with the same normals"""
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction.pointcloud import ICPConvergenceCriteria
    pose, stats, p4, n_cand = launched[N]
    states = _device_icp(B, P.sources(p4, n_cand, N), cases, models, ICPConvergenceCriteria(*C.CRITERIA))
    for i, st in enumerate(states):
        T = st[5:21].reshape(4, 4)
        Ti = C.rigid_inverse(T)
        want_pose = cases[i]["pose"] if st[1] == 0 else C.pose7(Ti[:3, :3], Ti[:3, 3])
        _check(pose[i], stats[i], want_pose, (st[2], st[3], st[4], st[37]), T, "%s N=%d vs device ICP" % (OBJECTS[i], N))


def _device_icp(B, srcs, cases, models, crit):
    src = [B._cloud(torch.from_numpy(s).cuda(), "cuda") for s in srcs]
    tgt = []
    for c in cases:
        k = CLASS_OF_M[len(c["model"])]
        t = B._cloud(torch.from_numpy(np.ascontiguousarray(c["model"])).cuda(), "cuda")
        t._n = models.normals[k]
        tgt.append(t)
    inits = [C.rigid_inverse(C.pose_matrix(c["pose"])) for c in cases]
    return B.icp_states(src, tgt, C.MAX_DIST, inits, 1, crit)


def test_a_model_set_too_large_for_lds_gives_the_same_bits(launched, cases, clouds, normals):
    """a 4000-point class beside the others: observed points + the largest grid no longer fit the workgroup's LDS, every object of the
    launch is searched in global memory -- by the same code in the same order (the normals are read from global memory either way)"""
    from autoposeestimation_amd.pipeline.polish import ModelSet
    big = dict(clouds)
    big[6] = C.model(4000, 7)[0]
    given = dict(normals)
    given[6] = np.tile([1.0, 0.0, 0.0], (4000, 1))
    ms = ModelSet(big, "cuda", C.MAX_DIST, normals=given)
    assert 1000 * 24 + ms.max_points * 36 > 144 * 1024
    assert _same(_launch(ms, _plain(cases), 1000), launched[1000])


def test_padding_is_not_read(models, cases, launched):
    """rows ns..N-1 filled with NaN instead of choose's wrap-around, and an object with more candidates than rows (n_cand = 5000 > N)"""
    items = _plain(cases)
    items[0] = (cases[0], 5000, None)                    # "big": 1000 points = N rows, all of them read
    for N in P.SIZES:
        wrap = _launch(models, items, N, "wrap")
        nan = _launch(models, items, N, "nan")
        assert np.isnan(nan[2]).any() and np.isfinite(nan[0]).all() and np.isfinite(nan[1]).all()
        assert _same(wrap, nan) and _same(wrap, launched[N])          # ns = min(n_cand, N) either way


def test_degenerate_objects_pass_through_and_leave_their_neighbours_alone(models, cases, launched, normals):
    mid, odd, mid1 = cases[1], cases[3], cases[6]
    far = mid["pose"].copy()
    far[4:7] += (0.5, 0.0, 0.0)
    items = [(mid, None, None), (mid, 0, None), (mid1, None, None), (mid, 5, None), (mid, None, far), (odd, None, None), (mid, None, None),
             (mid, None, None)]
    classes = [CLASS_OF_M[len(c["model"])] for c, _, _ in items]
    classes[6] = 9                                        # a class outside the table, known to the device alone
    classes[7] = 4                                        # a class of the table without a model (M = 0, no normals)
    dev_classes = torch.tensor(classes, dtype=torch.int32).cuda()
    pose, stats, p4, _ = _launch(models, items, 1000, classes=dev_classes)
    for i in (1, 3, 4, 6, 7):
        assert np.array_equal(pose[i], items[i][0]["pose"] if items[i][2] is None else items[i][2]), i
    assert tuple(stats[1]) == (0.0, 0.0, 0.0, 2.0)
    five = P.reference(p4[3, :5, :3].astype(np.float64), mid["model"], normals[0], mid["pose"])[1]
    assert stats[3, 3] == 2 and 3 <= stats[3, 2] == five[2] <= 5 and stats[3, 0] == five[0]       # at most 5 correspondences: below the 6 of a 6x6 system
    assert abs(stats[3, 1] - five[1]) <= 1e-12 + 1e-9 * five[1]
    assert tuple(stats[4]) == (0.0, 0.0, 0.0, 2.0)
    assert tuple(stats[6]) == (0.0, 0.0, 0.0, 0.0)
    old = _launch(models, items, 1000, classes=dev_classes, estimation="point_to_point")
    assert np.array_equal(stats[7], old[1][7]) and np.array_equal(stats[6], old[1][6]) and tuple(stats[7][:3]) == (0.0, 0.0, 0.0)
    for i, j in ((0, 1), (2, 6), (5, 3)):                 # the neighbours: what the same objects gave in the 7-object launch
        assert np.array_equal(pose[i], launched[1000][0][j]) and np.array_equal(stats[i], launched[1000][1][j])


def test_singular_normal_equations_give_the_identity_update(clouds, cases):
    """every normal (0, 0, 1): columns 2..4 of J = [s x n, n] are exactly zero, solve6 meets an exact zero pivot -- the update is the
    identity and counts as one (icp_step), the second evaluation repeats the first and the loop stops as converged.  The oracle raises
    here (numpy.linalg.solve); the device ICP, kind 1, is the reference."""
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction.pointcloud import ICPConvergenceCriteria
    from autoposeestimation_amd.pipeline.polish import ModelSet
    flat = ModelSet(clouds, "cuda", C.MAX_DIST, normals={k: np.tile([0.0, 0.0, 1.0], (len(p), 1)) for k, p in clouds.items()})
    assert flat.flat_normals == {k: len(p) for k, p in clouds.items()}
    pose, stats, p4, n_cand = _launch(flat, _plain(cases), 1000)
    assert np.isfinite(pose).all() and np.isfinite(stats).all()
    states = _device_icp(B, P.sources(p4, n_cand, 1000), cases, flat, ICPConvergenceCriteria(*C.CRITERIA))
    for i, st in enumerate(states):
        three = OBJECTS[i][0] == "three"
        assert st[1] == (0 if three else 1) and st[37] == (2 if three else 1), OBJECTS[i]      # (one identity update, then "converged")
        assert stats[i, 0] == st[2] and stats[i, 2] == st[4] and stats[i, 3] == st[37], OBJECTS[i]
        assert abs(stats[i, 1] - st[3]) <= 1e-12 + 1e-9 * st[3], OBJECTS[i]
        got_T = C.rigid_inverse(C.pose_matrix(pose[i]))
        assert np.abs(got_T - st[5:21].reshape(4, 4)).max() <= T_ATOL, OBJECTS[i]
        assert np.abs(got_T - C.rigid_inverse(C.pose_matrix(cases[i]["pose"]))).max() <= T_ATOL, OBJECTS[i]      # T never moved
        if three:
            assert np.array_equal(pose[i], cases[i]["pose"])


def test_min_fitness_gates_the_pose_and_keeps_the_stats(models, cases, launched):
    pose, stats, _, _ = _launch(models, _plain(cases), 1000, min_fitness=1.1)
    assert np.array_equal(pose, np.stack([c["pose"] for c in cases]))
    assert np.array_equal(stats, launched[1000][1])
    assert not np.array_equal(launched[1000][0], pose)


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_the_iteration_limit_stops_the_loop(models, cases, normals, limit):
    """stop reason 3 after `limit` updates, the oracle's pose after as many (`three` never gets that far: reason 2 unless the limit is 0);
    a limit of 0 applies no update: the pose passes through"""
    class Limited:
        relative_fitness, relative_rmse, max_iteration = 1e-6, 1e-6, limit
    pose, stats, p4, n_cand = _launch(models, _plain(cases), 1000, criteria=Limited)
    for i, (s, c) in enumerate(zip(P.sources(p4, n_cand, 1000), cases)):
        want_pose, want_stats, want_T = P.reference(s, c["model"], normals[CLASS_OF_M[len(c["model"])]], c["pose"], criteria=(1e-6, 1e-6, limit))
        assert want_stats[3] == (2 if OBJECTS[i][0] == "three" and limit else 3)      # (3 points: the limit is looked at before the count)
        _check(pose[i], stats[i], want_pose, want_stats, want_T, "%s limit %d" % (OBJECTS[i], limit))
        if limit == 0:
            assert np.array_equal(pose[i], c["pose"])


def test_an_object_alone_equals_itself_in_the_batch(models, cases, launched):
    for i, c in enumerate(cases):
        pose, stats, _, _ = _launch(models, [(c, None, None)], 1000)
        assert np.array_equal(pose[0], launched[1000][0][i]) and np.array_equal(stats[0], launched[1000][1][i]), OBJECTS[i]


def test_the_call_is_capturable_and_follows_its_inputs(models, cases, launched):
    """captured on one stream with static buffers, replayed after the inputs were overwritten in place"""
    from autoposeestimation_amd import engine as E
    _, _, p4, n_cand = launched[1000]
    cls = np.array([CLASS_OF_M[len(c["model"])] for c in cases], np.int32)
    pose = np.stack([c["pose"] for c in cases])
    warm = [torch.from_numpy(np.ascontiguousarray(a[::-1])).cuda() for a in (p4, n_cand, cls, pose)]      # first the objects in reverse
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        E.icp_polish(warm[0], warm[1], warm[2], models, warm[3], C.MAX_DIST, Criteria, 0.0, PLANE)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out, stats = E.icp_polish(warm[0], warm[1], warm[2], models, warm[3], C.MAX_DIST, Criteria, 0.0, PLANE)
        graph.replay()
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), launched[1000][0][::-1]) and np.array_equal(stats.cpu().numpy(), launched[1000][1][::-1])
        for t, a in zip(warm, (p4, n_cand, cls, pose)):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        s.synchronize()
    assert np.array_equal(out.cpu().numpy(), launched[1000][0]) and np.array_equal(stats.cpu().numpy(), launched[1000][1])


def test_quality_and_update_count(cases, launched, references, normals):
    """what the estimator is for: the polished poses put the models where the truth has them, in fewer updates than point-to-point needs
    (printed, per object: the restatements' update counts)"""
    for i, c in enumerate(cases):
        if OBJECTS[i][0] == "three":
            continue
        before = C.model_distance(c["model"], c["pose"], c["R"], c["t"])
        after = C.model_distance(c["model"], launched[1000][0][i], c["R"], c["t"])
        s = P.sources(launched[1000][2], launched[1000][3], 1000)[i]
        init = C.rigid_inverse(C.pose_matrix(c["pose"]))
        plane = P.icp_plane_with_reason(s, c["model"], normals[CLASS_OF_M[len(c["model"])]], C.MAX_DIST, init, *C.CRITERIA)[5]
        point = C.icp_with_reason(s, c["model"], C.MAX_DIST, init, *C.CRITERIA)[5]
        print("%s: mean model-point distance to the truth %.3e m -> %.3e m; updates: point-to-plane %d, point-to-point %d" % (OBJECTS[i], before, after, plane, point))
        assert after < before and after < (1e-3 if OBJECTS[i][0] == "noisy" else 1e-6)
        assert plane <= point


def _pose_nets():
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet
    est = PoseNet(1000, 12)
    est.load_state_dict(S.posenet_state_dict(12, 0))
    ref = PoseRefineNet(1000, 12)
    ref.load_state_dict(S.refiner_state_dict(12, 0))
    return est.cuda().eval(), ref.cuda().eval()


def test_wired_into_the_frame_pipeline():
    """FramePipeline(icp_polish=IcpPolish(..., estimation="point_to_plane")) on the frame of the point-to-point wiring test (two painted
    objects of different crop sizes: two buckets; model clouds = the objects' own depth points, turned by 2 degrees and shifted by 2 mm).
    Nothing else moves, and pose / fit are what engine.icp_polish returns for the outputs of the run without the switch -- eagerly and
    through the bucket graphs -- and not what the point-to-point switch gives."""
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.pipeline.polish import IcpPolish
    from autoposeestimation_amd.pipeline.utils import FramePipeline
    classes = ["obj%02d" % i for i in range(12)]
    est, ref = _pose_nets()
    rgb_h, depth_h, label = S.synthetic_frame_multi(31, [(3, (100, 200), (70, 70)), (5, (250, 300), (110, 150))])
    rgb, depth = torch.from_numpy(rgb_h[None]).cuda(), torch.from_numpy(depth_h[None]).cuda()
    logits = torch.from_numpy((np.eye(13, dtype=np.float32)[label] * 10.0)[None]).cuda()
    meta = S.REALSENSE_META
    off = FramePipeline(None, est, ref, classes).run(rgb, depth, meta, inject_logits=logits, seed=5)
    assert [o[1] for o in off["objects"]] == [3, 5] and "fit" not in off and "pose_raw" not in off
    objs = torch.tensor(off["objects"], dtype=torch.int32).cuda()
    pts4 = E.backproject(depth, objs, off["choose"], meta["intr"], meta["depth_scale"])
    pose_off, n_cand_off = off["pose"].cpu().numpy(), off["n_cand"].cpu().numpy()
    clouds = {k: C.model(300, k)[0] for k in range(12)}
    for i, o in enumerate(off["objects"]):
        p = pts4[i, :min(int(n_cand_off[i]), 1000), :3].cpu().numpy().astype(np.float64)
        Ti = C.rigid_inverse(C.pose_matrix(pose_off[i]))
        m = p @ Ti[:3, :3].T + Ti[:3, 3]
        centre = m.mean(0)
        clouds[o[1] - 1] = (m - centre) @ C.rodrigues((1.0, 2.0, 3.0), np.radians(2.0)).T + centre + np.array([0.0015, -0.001, 0.0008])
    switch = IcpPolish(clouds, estimation=PLANE)
    models = switch.model_set(rgb.device)
    assert models.normals is not None and switch.model_set(rgb.device) is models
    cls = [o[1] - 1 for o in off["objects"]]
    want_pose, want_fit = E.icp_polish(pts4, off["n_cand"], cls, models, off["pose"], 0.01, switch.criteria, 0.0, PLANE)
    point_pose, _ = E.icp_polish(pts4, off["n_cand"], cls, models, off["pose"], 0.01, switch.criteria, 0.0)
    print("fit", want_fit.cpu().numpy().tolist())
    assert bool((want_fit[:, 0] > 0.5).all()) and not torch.equal(want_pose, off["pose"])         # (the polish really moved the poses)
    assert not torch.equal(want_pose, point_pose)

    def same(got):
        if got.get("stream") is not None:
            torch.cuda.current_stream().wait_stream(got["stream"])
        torch.cuda.synchronize()
        assert got["objects"] == off["objects"]
        for k in ("objmap", "choose", "n_cand"):
            assert torch.equal(got[k], off[k]), k
        assert torch.equal(got["pose_raw"], off["pose"])
        assert torch.equal(got["pose"], want_pose) and torch.equal(got["fit"], want_fit)

    same(FramePipeline(None, est, ref, classes, icp_polish=switch).run(rgb, depth, meta, inject_logits=logits, seed=5))
    graphs = FramePipeline(None, est, ref, classes, pose_graphs=True, icp_polish=switch)
    for call in range(3):                                 # eager, capture + replay, replay
        same(graphs.run(rgb, depth, meta, inject_logits=logits, seed=5))
    assert len(graphs._graphs) == 2


@pytest.mark.parametrize("N", P.SIZES)
def test_point_to_point_keeps_the_parents_bits(cases, N):
    """ape_icp_polish_batch_f64 shares its loop with the point-to-plane export since the estimator became a compile-time parameter: the
    7-object launch must reproduce, bit for bit, what the library of the commit before gave (tests/golden/icp_polish_p2p_bits.npz,
    recorded by tools/gen_golden_icp_polish_bits.py).  A difference means the point-to-point instantiation was changed."""
    from autoposeestimation_amd.pipeline.polish import ModelSet
    gold = np.load(GOLDEN)
    print("golden recorded with:", str(gold["toolchain"]))
    pose, stats, _, _ = _launch(ModelSet(P.clouds(), "cuda", C.MAX_DIST), _plain(cases), N, estimation="point_to_point")
    assert pose.dtype == gold["pose_%d" % N].dtype == np.float64
    assert np.array_equal(pose.view(np.uint64), gold["pose_%d" % N].view(np.uint64))
    assert np.array_equal(stats.view(np.uint64), gold["stats_%d" % N].view(np.uint64))

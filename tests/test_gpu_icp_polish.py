"""The one-launch depth ICP polish (ape_icp_polish_batch_f64, csrc/icp_polish.hip) against the project's oracle
(oracle/pointcloud_oracle.py:registration_icp through icp_polish_cases.reference), against the existing device ICP, and wired into
FramePipeline.  Bars: correspondences, fitness and stop reason exactly; pose and T within T_ATOL = 1e-9 absolute (the bar of the
registration kernels: at the fixed point the float64 summation-order noise is about 1e-15); |d rmse| <= 1e-12 + 1e-9 rmse."""
import numpy as np
import pytest
import torch

import icp_polish_cases as C

pytestmark = pytest.mark.gpu
T_ATOL = 1e-9
# the launch of the parity tests: every case, mixed order, four objects on the 1000-point model
OBJECTS = (("big", 0), ("mid", 0), ("three", 0), ("odd", 0), ("noisy", 0), ("tiny", 0), ("mid", 1))
CLASS_OF_M = {1000: 0, 257: 1, 63: 2, 2600: 3}


class Criteria:
    relative_fitness, relative_rmse, max_iteration = C.CRITERIA


@pytest.fixture(scope="module")
def cases():
    return [C.named(name, seed) for name, seed in OBJECTS]


@pytest.fixture(scope="module")
def clouds():
    return {k: C.model(m, 0)[0] for m, k in CLASS_OF_M.items()}


@pytest.fixture(scope="module")
def models(clouds):
    from autoposeestimation_amd.pipeline.polish import ModelSet
    return ModelSet(clouds, "cuda", C.MAX_DIST)


def _launch(models, items, N, pad="wrap", min_fitness=0.0, classes=None, criteria=Criteria):
    """items = [(case, n_cand or None, pose or None)] -> (pose_out [n,7], stats [n,4], points4 [n,N,4], n_cand [n]) as numpy"""
    from autoposeestimation_amd import engine as E
    p4 = np.stack([C.points4(c["obs"], N, nc, pad) for c, nc, _ in items])
    n_cand = np.array([len(c["obs"]) if nc is None else nc for c, nc, _ in items], np.int32)
    pose = np.stack([c["pose"] if p is None else p for c, _, p in items])
    cls = [CLASS_OF_M[len(c["model"])] for c, _, _ in items] if classes is None else classes
    out, stats = E.icp_polish(torch.from_numpy(p4).cuda(), torch.from_numpy(n_cand).cuda(), cls, models, torch.from_numpy(pose).cuda(), C.MAX_DIST,
                              criteria, min_fitness)
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy(), p4, n_cand


def _plain(cases):
    return [(c, None, None) for c in cases]


@pytest.fixture(scope="module")
def launched(models, cases):
    """the 7-object launch at N = 1000 and N = 500, computed once and left unchanged"""
    return {N: _launch(models, _plain(cases), N) for N in (1000, 500)}


def _sources(p4, n_cand, N):
    return [p4[i, :min(int(n_cand[i]), N), :3].astype(np.float64) for i in range(len(p4))]


@pytest.fixture(scope="module")
def references(cases, launched):
    """the oracle on what the kernel is given: the float32 points widened to float64"""
    out = {}
    for N, (_, _, p4, n_cand) in launched.items():
        out[N] = [C.reference(s, c["model"], c["pose"]) for s, c in zip(_sources(p4, n_cand, N), cases)]
    return out


def _check(pose, stats, want_pose, want_stats, want_T, tag):
    fit, rmse, n, reason = want_stats
    print("%s: corr %d/%d fit %.6f/%.6f reason %d/%d |d rmse| %.3e |d pose| %.3e" % (tag, stats[2], n, stats[0], fit, stats[3], reason,
                                                                                  abs(stats[1] - rmse), np.abs(pose - want_pose).max()))
    assert stats[2] == n and stats[0] == fit and stats[3] == reason, tag
    assert abs(stats[1] - rmse) <= 1e-12 + 1e-9 * rmse, tag
    assert np.abs(pose - want_pose).max() <= T_ATOL, tag
    assert np.abs(C.rigid_inverse(C.pose_matrix(pose)) - want_T).max() <= T_ATOL, tag
    assert pose[0] >= 0


@pytest.mark.parametrize("N", [1000, 500])
def test_parity_with_the_oracle(launched, references, N):
    pose, stats, _, n_cand = launched[N]
    assert int(n_cand.max()) > 500 and int(n_cand.min()) == 3
    for i, (want_pose, want_stats, want_T) in enumerate(references[N]):
        _check(pose[i], stats[i], want_pose, want_stats, want_T, "%s N=%d" % (OBJECTS[i], N))
    assert set(stats[:, 3].astype(int)) <= {1, 2, 3}


@pytest.mark.parametrize("N", [1000, 500])
def test_parity_with_the_existing_device_icp(launched, cases, clouds, N):
    """batched.registration_icp (ape_icp_run_batch_f64, kind 0: three launches per iteration, grids per call) on the same pairs"""
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction.pointcloud import ICPConvergenceCriteria
    pose, stats, p4, n_cand = launched[N]
    crit = ICPConvergenceCriteria(*C.CRITERIA)
    src = [B._cloud(torch.from_numpy(s).cuda(), "cuda") for s in _sources(p4, n_cand, N)]
    tgt = [B._cloud(torch.from_numpy(np.ascontiguousarray(clouds[CLASS_OF_M[len(c["model"])]])).cuda(), "cuda") for c in cases]
    inits = [C.rigid_inverse(C.pose_matrix(c["pose"])) for c in cases]
    Ts = B.registration_icp(src, tgt, C.MAX_DIST, inits, 0, crit)
    states = B.icp_states(src, tgt, C.MAX_DIST, inits, 0, crit)
    for i, (T, st) in enumerate(zip(Ts, states)):
        assert np.array_equal(T, st[5:21].reshape(4, 4))
        Ti = C.rigid_inverse(T)
        _check(pose[i], stats[i], C.pose7(Ti[:3, :3], Ti[:3, 3]), (st[2], st[3], st[4], st[37]), T, "%s N=%d vs device ICP" % (OBJECTS[i], N))


def test_a_model_set_too_large_for_lds_gives_the_same_bits(launched, cases, clouds):
    """a 4000-point class beside the others: observed points + the largest grid no longer fit the workgroup's LDS, every object of the
    launch is searched in global memory -- by the same code in the same order"""
    from autoposeestimation_amd.pipeline.polish import ModelSet
    big = dict(clouds)
    big[4] = C.model(4000, 7)[0]
    ms = ModelSet(big, "cuda", C.MAX_DIST)
    assert 1000 * 24 + ms.max_points * 36 > 144 * 1024
    pose, stats, _, _ = _launch(ms, _plain(cases), 1000)
    assert np.array_equal(pose, launched[1000][0]) and np.array_equal(stats, launched[1000][1])


def test_padding_is_not_read(models, cases, launched):
    """rows ns..N-1 filled with NaN instead of choose's wrap-around, and an object with more candidates than rows (n_cand = 5000 > N)"""
    items = _plain(cases)
    items[0] = (cases[0], 5000, None)                    # "big": 1000 points = N rows, all of them read
    for N in (1000, 500):
        wrap = _launch(models, items, N, "wrap")
        nan = _launch(models, items, N, "nan")
        assert np.isnan(nan[2]).any() and np.isfinite(nan[0]).all() and np.isfinite(nan[1]).all()
        assert np.array_equal(wrap[0], nan[0]) and np.array_equal(wrap[1], nan[1])
        assert np.array_equal(wrap[0], launched[N][0]) and np.array_equal(wrap[1], launched[N][1])       # ns = min(n_cand, N) either way


def test_degenerate_objects_pass_through_and_leave_their_neighbours_alone(models, cases, launched):
    mid, odd, mid1 = cases[1], cases[3], cases[6]
    far = mid["pose"].copy()
    far[4:7] += (0.5, 0.0, 0.0)
    items = [(mid, None, None), (mid, 0, None), (mid1, None, None), (mid, 2, None), (mid, None, far), (odd, None, None), (mid, None, None)]
    classes = [CLASS_OF_M[len(c["model"])] for c, _, _ in items]
    classes[6] = 9                                        # a class outside the table, known to the device alone: passed through, all-zero stats
    pose, stats, p4, _ = _launch(models, items, 1000, classes=torch.tensor(classes, dtype=torch.int32).cuda())
    for i in (1, 3, 4, 6):
        assert np.array_equal(pose[i], items[i][0]["pose"] if items[i][2] is None else items[i][2]), i
    assert tuple(stats[1]) == (0.0, 0.0, 0.0, 2.0)
    two = C.reference(p4[3, :2, :3].astype(np.float64), mid["model"], mid["pose"])[1]
    assert stats[3, 3] == 2 and stats[3, 2] == two[2] <= 2 and stats[3, 0] == two[0]
    assert tuple(stats[4]) == (0.0, 0.0, 0.0, 2.0)
    assert tuple(stats[6]) == (0.0, 0.0, 0.0, 0.0)
    for i, j in ((0, 1), (2, 6), (5, 3)):                 # the neighbours: what the same objects gave in the 7-object launch
        assert np.array_equal(pose[i], launched[1000][0][j]) and np.array_equal(stats[i], launched[1000][1][j])


def test_min_fitness_gates_the_pose_and_keeps_the_stats(models, cases, launched):
    pose, stats, _, _ = _launch(models, _plain(cases), 1000, min_fitness=1.1)
    assert np.array_equal(pose, np.stack([c["pose"] for c in cases]))
    assert np.array_equal(stats, launched[1000][1])
    assert not np.array_equal(launched[1000][0], pose)


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_the_iteration_limit_stops_the_loop(models, cases, limit):
    """stop reason 3 after `limit` updates, the oracle's pose after as many; a limit of 0 applies no update: the pose passes through"""
    class Limited:
        relative_fitness, relative_rmse, max_iteration = 1e-6, 1e-6, limit
    pose, stats, p4, n_cand = _launch(models, _plain(cases), 1000, criteria=Limited)
    for i, (s, c) in enumerate(zip(_sources(p4, n_cand, 1000), cases)):
        want_pose, want_stats, want_T = C.reference(s, c["model"], c["pose"], criteria=(1e-6, 1e-6, limit))
        assert want_stats[3] == 3
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
        E.icp_polish(warm[0], warm[1], warm[2], models, warm[3], C.MAX_DIST, Criteria, 0.0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out, stats = E.icp_polish(warm[0], warm[1], warm[2], models, warm[3], C.MAX_DIST, Criteria, 0.0)
        graph.replay()
        s.synchronize()
        assert np.array_equal(out.cpu().numpy(), launched[1000][0][::-1]) and np.array_equal(stats.cpu().numpy(), launched[1000][1][::-1])
        for t, a in zip(warm, (p4, n_cand, cls, pose)):
            t.copy_(torch.from_numpy(a))
        graph.replay()
        s.synchronize()
    assert np.array_equal(out.cpu().numpy(), launched[1000][0]) and np.array_equal(stats.cpu().numpy(), launched[1000][1])


def test_quality_on_the_noisy_case(cases, launched):
    """0.5 mm of noise on the observed points: the polished pose puts the model closer to the truth than the predicted one
    (the oracle: millimetres -> below 0.1 mm)"""
    c = cases[4]
    before = C.model_distance(c["model"], c["pose"], c["R"], c["t"])
    after = C.model_distance(c["model"], launched[1000][0][4], c["R"], c["t"])
    print("noisy case: mean model-point distance to the truth %.3e m -> %.3e m" % (before, after))
    assert after < before


def _pose_nets():
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet
    est = PoseNet(1000, 12)
    est.load_state_dict(S.posenet_state_dict(12, 0))
    ref = PoseRefineNet(1000, 12)
    ref.load_state_dict(S.refiner_state_dict(12, 0))
    return est.cuda().eval(), ref.cuda().eval()


def test_wired_into_the_frame_pipeline():
    """FramePipeline(icp_polish=...) on one synthetic frame with two painted objects of different crop sizes (two buckets), injected
    logits, untrained fixture weights.  The model clouds of the two classes are the objects' own depth points moved into the model frame
    of the unpolished pose and then turned by 2 degrees and shifted by 2 mm, so the polish has something to do.  Nothing else moves, and
    pose / fit are what engine.icp_polish returns for the outputs of the run without the switch -- eagerly and through the bucket graphs."""
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd import synthetic as S
    from autoposeestimation_amd.pipeline.polish import IcpPolish, ModelSet
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
    switch = IcpPolish(clouds)
    want_pose, want_fit = E.icp_polish(pts4, off["n_cand"], [o[1] - 1 for o in off["objects"]], ModelSet.cached(clouds, rgb.device, 0.01),
                                       off["pose"], 0.01, switch.criteria, 0.0)
    assert bool((want_fit[:, 0] > 0.5).all()) and not torch.equal(want_pose, off["pose"])         # (the polish really moved the poses)

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

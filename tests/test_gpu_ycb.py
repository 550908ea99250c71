"""The YCB-Video sample builder on the GPU (DenseFusion/datasets/ycb/augment.py, csrc/ycb.hip): `batch` against `sample_host` and the
reference's golden bit for bit, the three entry points against numpy at edge inputs, determinism and the refusals; and the driver
DenseFusion/tools/eval_ycb.py against a restated loop over the oracle's networks."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import ycb_reference as R
from autoposeestimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = R.H, R.W
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
CAM = (312.9869, 241.3109, 1066.778, 1067.487)
EINVAL = -1


def _same(got, want, what):
    """a device sample (as DataLoader(batch_size=1) delivers it) against a host sample"""
    assert len(got) == len(want) == 6
    for g, w, name in zip(got, want, R.NAMES):
        w = w.view(1, 1) if w.dim() == 1 and w.numel() == 1 and g.dim() == 2 else w.unsqueeze(0)
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), "%s: %s differs" % (what, name)


# ---- batch() against the host path and the reference's golden ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_batch_equals_sample_host_and_the_reference(name):
    """under reference_rng the batch (built sample after sample) makes the reference's draws: it equals the golden; and it equals
    `sample_host` with the parameters it returns"""
    order = R.GOLD[name + "_order"].tolist()
    random.seed(int(R.GOLD["seed"]))
    np.random.seed(int(R.GOLD["seed"]))
    ds = R.dataset(name, reference_rng=True, device=DEV)
    out, ps = ds.batch(order, return_params=True)
    state = random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2]
    assert len(out) == len(order) == len(ps)
    for k, (i, got, p) in enumerate(zip(order, out, ps)):
        _same(got, R.golden_sample(name, k), "%s sample %d against the reference" % (name, k))
        _same(got, ds.sample_host(i, p), "%s sample %d against sample_host" % (name, k))
    fronts = [p.get("front") for p in ps]
    if name == "noise":
        assert any(f is not None for f in fronts)                # an accepted front
    if name == "reject":
        assert all(f is None for f in fronts) and all("front" in p for p in ps)         # all five candidates skipped or rejected
        assert all("subset" in p for p in ps)                    # more valid pixels than num_pt = 60
    if name == "threshold":                                      # exactly 1000 labelled pixels left: rejected; 1001: accepted
        assert fronts[0] is None and fronts[1] is not None and fronts[1][0] == S.YCB_SYN_HOLE and sorted(fronts[1][2]) == [13, 14]
    if name == "plain":
        lines = [ds.list[i] for i in order]
        assert S.YCB_CAM2 in lines and S.YCB_SYN_MULTI in lines and S.YCB_SMALL in lines
        k = lines.index(S.YCB_SYN_MULTI)
        assert ps[k]["noise"].dtype == np.float64 and ps[k]["back"][0] in ds.real
        assert "subset" not in ps[lines.index(S.YCB_SMALL)]      # 51 valid pixels: the wrap pad
    if name == "refine":
        assert out[0][4].shape == (1, 2600, 3)
    # the generators are left as the reference's loop leaves them
    random.seed(int(R.GOLD["seed"]))
    np.random.seed(int(R.GOLD["seed"]))
    for i in order:
        ds[i]
    assert (random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2]) == state
    again = ds.batch(order, params=ps)                           # one batch, the draws injected
    for k, i in enumerate(order):
        _same(again[k], R.golden_sample(name, k), "%s sample %d of the injected batch" % (name, k))


@pytest.mark.parametrize("size", [1, 16, 17])
def test_seeded_batches_across_the_chunk_boundary(size):
    """per-sample seeded draws, all front candidates counted in one launch: real, camera-2 and synthetic entries mixed"""
    ds = R.dataset("noise", seed=4, device=DEV)
    idx = [k % len(ds) for k in range(size)] if size > 1 else [3]
    out, ps = ds.batch(idx, return_params=True)
    lines = [ds.list[i] for i in idx]
    if size > 1:
        assert S.YCB_CAM2 in lines and S.YCB_SYN_MULTI in lines and S.YCB_REAL_A in lines
        assert any(p["front"] is not None for p in ps) and any(p["front"] is None for p in ps)
    for k, i in enumerate(idx):
        _same(out[k], ds.sample_host(i, ps[k]), "sample %d of %d against sample_host" % (k, size))
        _same(out[k], ds[i], "sample %d of %d against ds[i]" % (k, size))         # the generator was rewound to the accepted candidate


def test_objects_with_pixels_on_the_frame_borders():
    """the object the sample is about has members in row 0 and column 0 (class 1 of YCB_REAL_A), in row 479 and column 639 (class 4 of
    YCB_REAL_B), in column 0 only (class 7 of YCB_CAM2): extents, the shifted crop, `choose` and the cloud against the host path"""
    seen = set()
    for seed in (3, 4):                                          # the seeds whose object draws fall on these objects
        ds = R.dataset("plain", seed=seed, device=DEV)
        idx = [ds.list.index(x) for x in (S.YCB_REAL_A, S.YCB_REAL_B, S.YCB_CAM2)]
        out, ps = ds.batch(idx, return_params=True)
        for k, i in enumerate(idx):
            _same(out[k], ds.sample_host(i, ps[k]), "seed %d sample %d against sample_host" % (seed, k))
            _same(out[k], ds[i], "seed %d sample %d against ds[i]" % (seed, k))
            lab = ds._resident(ds.list[i])[2].cpu().numpy() == int(out[k][5]) + 1
            seen.add((ds.list[i], int(out[k][5]) + 1, bool(lab[0].any()), bool(lab[:, 0].any()), bool(lab[H - 1].any()), bool(lab[:, W - 1].any())))
    assert {(S.YCB_REAL_A, 1, True, True, False, False), (S.YCB_REAL_B, 4, False, False, True, True),
            (S.YCB_CAM2, 7, False, True, False, False)} <= seen


def test_the_over_1000_decision_at_its_threshold_with_seeded_draws():
    """all candidates counted in one launch: the table's sum is exactly 1000 for YCB_REAL_B (rejected five times), 1001 for YCB_EDGE"""
    ds = R.dataset("threshold", seed=2, device=DEV)
    out, ps = ds.batch([0, 1], return_params=True)
    assert ps[0]["front"] is None and ps[1]["front"] is not None and ps[1]["front"][0] == S.YCB_SYN_HOLE
    for k in (0, 1):
        _same(out[k], ds[k], "sample %d" % k)
    assert tuple(out[1][2].shape) == (1, 3, 40, 40) and int(out[1][5]) == 18


def test_rejecting_candidates_with_seeded_draws():
    ds = R.dataset("reject", seed=9, device=DEV)
    out, ps = ds.batch([0, 1, 2], return_params=True)
    assert all(p["front"] is None for p in ps)
    for k, i in enumerate([0, 1, 2]):
        _same(out[k], ds[i], "sample %d" % k)
    with pytest.raises(ValueError, match=S.YCB_NONE):
        ds.batch([4])


# ---- the entry points against numpy --------------------------------------------------------------------------------------------------------
def _overlap_numpy(label, front, depth):
    t = np.zeros((22, 22, 2), np.uint32)
    f = np.zeros_like(label) if front is None else front
    np.add.at(t, (label.reshape(-1), f.reshape(-1), (depth.reshape(-1) != 0).astype(np.int64)), 1)
    return t


def _overlap_inputs():
    rng = np.random.default_rng(3)
    depth = rng.integers(0, 3, (H, W)).astype(np.uint16) * 4000
    one = np.full((H, W), 7, np.uint8)                           # a one-class frame
    mixed = rng.integers(0, 22, (H, W)).astype(np.uint8)         # every class, 21 among them
    mixed[:40] = 21
    front = np.zeros((H, W), np.uint8)
    front[100:300, 200:500] = 21
    front[50:120, 0:640] = 4
    return [(one, front, depth), (mixed, front, depth), (mixed, mixed, np.zeros((H, W), np.uint16)), (mixed, None, depth), (one, None, depth)]


def test_overlap_equals_numpy_and_is_deterministic():
    from autoposeestimation_amd.DenseFusion.datasets.ycb import augment as G
    host = _overlap_inputs() * 4                                 # 20 triples: two launches
    up = lambda a: None if a is None else torch.from_numpy(a).to(DEV)  # noqa: E731
    pairs = [tuple(up(a) for a in t) for t in host]
    got = G.overlap(pairs, H, W)
    assert got.shape == (20, 22, 22, 2) and got.dtype == np.uint32
    for k, t in enumerate(host):
        assert np.array_equal(got[k], _overlap_numpy(*t)), k
        assert int(got[k].sum()) == H * W
    assert got[0][7].sum() == H * W and got[2][:, :, 1].sum() == 0 and got[3][:, 1:].sum() == 0 and got[1][21].sum() >= 40 * W
    assert np.array_equal(G.overlap(pairs, H, W), got)           # integers only: bit for bit


def _frame(rng, label):
    rgb = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    depth = rng.integers(5000, 12000, (H, W)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.1] = 0
    return rgb, depth, label


def test_rows_with_a_window_narrower_than_the_mask():
    """the eval case: the window is the crop of a roi, the mask reaches beyond it on every side and is partly covered by a front"""
    from autoposeestimation_amd.DenseFusion.datasets.ycb import augment as G
    rng = np.random.default_rng(5)
    label = np.zeros((H, W), np.uint8)
    label[50:430, 30:610] = 3
    label[200:220, 300:330] = 8
    flabel = np.zeros((H, W), np.uint8)
    flabel[100:140, :] = 5
    flabel[:, 400:420] = 9
    flabel[300:310, 100:200] = 2                                 # not one of the two front classes
    host, fhost = _frame(rng, label), _frame(rng, flabel)
    frame = tuple(torch.from_numpy(x).to(DEV) for x in host)
    front = tuple(torch.from_numpy(x).to(DEV) for x in fhost)
    ops = [("contrast", 0.87), ("brightness", 1.1)]
    jobs = (G.YcbJob * 2)()
    jobs[0] = G.make_job(frame, H, W, 3, CAM, 10000, ops=ops, front=(front[0], front[2], [5, 9], ops[::-1]), window=(120, 360, 77, 397))
    jobs[1] = G.make_job(frame, H, W, 3, CAM, 10000, window=(0, 40, 0, 40))
    ws, got = G.rows(jobs, H, W, 60, torch.device(DEV))
    member = (label == 3) & (flabel != 5) & (flabel != 9)
    for k, (mem, (r0, r1, c0, c1)) in enumerate([(member, (120, 360, 77, 397)), (label == 3, (0, 40, 0, 40))]):
        valid = mem & (host[1] != 0)
        win = np.zeros((H, W), bool)
        win[r0:r1, c0:c1] = True
        assert np.array_equal(got[k, :, 0], (valid & win).sum(axis=1)), k
        first = np.where(mem.any(axis=1), mem.argmax(axis=1), W)
        last = np.where(mem.any(axis=1), W - 1 - mem[:, ::-1].argmax(axis=1), -1)
        assert np.array_equal(got[k, :, 1], first) and np.array_equal(got[k, :, 2], last), k
    assert got[0, :, 0].sum() > 0 and got[1, :, 0].sum() == 0 and (got[0, 100:140, 2] == -1).all()
    # the L sums of the two jittered sources with a contrast op, as Pillow's ImageStat sees them
    from PIL import Image, ImageEnhance
    L = np.array(ImageEnhance.Brightness(Image.fromarray(fhost[0])).enhance(1.1).convert("L")).astype(np.int64).sum()
    lum = ws[:2 * 3 * 64 * 8].cpu().numpy().view(np.uint64).reshape(2, 3, 64)
    assert int(lum[0, 0].sum()) == int(np.array(Image.fromarray(host[0]).convert("L")).astype(np.int64).sum())
    assert int(lum[0, 2].sum()) == int(L) and int(lum[0, 1].sum()) == 0 and int(lum[1].sum()) == 0


def test_two_launches_agree_bit_for_bit():
    ds = R.dataset("noise", seed=2, device=DEV)
    idx = [0, 3, 2, 3]
    out, ps = ds.batch(idx, return_params=True)
    again = ds.batch(idx, params=ps)
    for a, b in zip(out, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_jobs_are_refused_without_a_launch():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import sample_jobs as J
    from autoposeestimation_amd.DenseFusion.datasets.ycb import augment as G
    L = _lib.lib()
    rng = np.random.default_rng(47)
    label = np.zeros((H, W), np.uint8)
    label[100:200, 100:200] = 6
    host = _frame(rng, label)
    frame = tuple(torch.from_numpy(x).to(DEV) for x in host)
    N = 60
    noise_bytes = 24 * 120 * 120
    ws_bytes = L.ape_ycb_noise_offset(1, H, N) + noise_bytes
    ws = torch.full((ws_bytes + 64,), 0x5a, dtype=torch.uint8, device=DEV)
    out_bytes = L.ape_pose_train_sample_bytes(N, 120, 120)
    out = torch.full((out_bytes + 64,), 0x5a, dtype=torch.uint8, device=DEV)
    table = torch.full((22 * 22 * 2 + 4,), -7, dtype=torch.int32, device=DEV)
    m, sd = J.norm(MEAN, STD, 3)

    def job(rmin=90, rmax=210, cmin=90, cmax=210, **kw):
        jobs = (G.YcbJob * 1)()
        jobs[0] = G.make_job(frame, H, W, 6, CAM, 10000)
        j = jobs[0]
        j.rmin, j.rmax, j.cmin, j.cmax = rmin, rmax, cmin, cmax
        for key, v in kw.items():
            setattr(j, key, v)
        return jobs

    def rows(jobs, ws_ptr=None, nbytes=None):
        return L.ape_ycb_rows(ctypes.cast(jobs, ctypes.c_void_p), 1, H, W, ctypes.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr),
                              ws_bytes if nbytes is None else nbytes, _lib.stream_ptr())

    def samples(jobs, out_ptr=None, nbytes=None, obytes=None, ws_ptr=None):
        return L.ape_ycb_samples(ctypes.cast(jobs, ctypes.c_void_p), 1, H, W, N, m, sd,
                                 ctypes.c_void_p(out.data_ptr() if out_ptr is None else out_ptr), out_bytes if obytes is None else obytes,
                                 ctypes.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr), ws_bytes if nbytes is None else nbytes,
                                 _lib.stream_ptr())

    def overlap(label_ptr, depth_ptr, table_ptr):
        pair = (G.YcbPair * 1)()
        pair[0].label, pair[0].front_label, pair[0].depth = label_ptr, None, depth_ptr
        return L.ape_ycb_overlap(ctypes.cast(pair, ctypes.c_void_p), 1, H, W, ctypes.c_void_p(table_ptr), _lib.stream_ptr())

    for bad in (job(rmin=400, rmax=520), job(cmin=-40, cmax=80), job(cmin=600, cmax=680),       # a crop outside the frame
                job(rmax=200), job(cmax=215), job(rmin=100, rmax=100)):                         # a side that is no multiple of 40
        assert samples(bad) == EINVAL
    for bad in (job(rgb=None), job(depth=None), job(label=None), job(depth=frame[1].data_ptr() + 1),      # a null or misaligned pointer
                job(front_label=frame[2].data_ptr()), job(obj=0), job(obj=22), job(front_a=22), job(win_r1=H + 1), job(win_c0=-1)):
        assert rows(bad) == EINVAL and samples(bad) == EINVAL
    assert rows(job(), nbytes=L.ape_ycb_tables_offset(1, H) - 1) == EINVAL                      # a short workspace
    assert samples(job(), nbytes=L.ape_ycb_noise_offset(1, H, N) - 1) == EINVAL
    assert samples(job(noise_off=L.ape_ycb_noise_offset(1, H, N)), nbytes=ws_bytes - 1) == EINVAL          # the noise does not fit
    assert samples(job(noise_off=L.ape_ycb_noise_offset(1, H, N) + 4)) == EINVAL
    assert samples(job(noise_off=0)) == EINVAL                                                  # noise over the tables
    assert rows(job(), ws_ptr=ws.data_ptr() + 8) == EINVAL and samples(job(), ws_ptr=ws.data_ptr() + 8) == EINVAL      # misaligned
    assert samples(job(), out_ptr=out.data_ptr() + 8) == EINVAL
    assert samples(job(), obytes=out_bytes - 16) == EINVAL                                      # a sample that does not fit
    assert samples(job(out_off=8)) == EINVAL
    assert overlap(None, frame[1].data_ptr(), table.data_ptr()) == EINVAL
    assert overlap(frame[2].data_ptr(), None, table.data_ptr()) == EINVAL
    assert overlap(frame[2].data_ptr(), frame[1].data_ptr(), None) == EINVAL
    assert overlap(frame[2].data_ptr(), frame[1].data_ptr(), table.data_ptr() + 2) == EINVAL
    torch.cuda.synchronize()
    assert bool((ws == 0x5a).all()) and bool((out == 0x5a).all()) and bool((table == -7).all())          # nothing was launched
    assert overlap(frame[2].data_ptr(), frame[1].data_ptr(), table.data_ptr()) == 0              # and the good calls go through
    assert rows(job()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(table[:968].cpu().numpy().view(np.uint32).reshape(22, 22, 2), _overlap_numpy(host[2], None, host[1]))
    assert table[968:].tolist() == [-7] * 4
    r0 = L.ape_ycb_rows_offset(1)
    got = ws[r0:r0 + 12 * H].cpu().numpy().view(np.int32).reshape(H, 3)
    assert np.array_equal(got[:, 0], ((label == 6) & (host[1] != 0)).sum(axis=1)) and got[150].tolist()[1:] == [100, 199]


# ---- the evaluation driver ---------------------------------------------------------------------------------------------------------------------
_memo = {}


def _restated():
    if "restated" not in _memo:
        _memo["restated"] = R.restated_eval(S.posenet_state_dict(21, 0), S.refiner_state_dict(21, 0))
    return _memo["restated"]


def _run(mode, out_dir):
    if mode not in _memo:
        from autoposeestimation_amd.DenseFusion.tools import eval_ycb as D
        root, dirs = R.tree()
        _memo[mode] = D.main(root, S.posenet_state_dict(21, 0), S.refiner_state_dict(21, 0), ycb_toolbox_dir=dirs["toolbox"],
                             dataset_config_dir=dirs["config"], result_wo_refine_dir=os.path.join(out_dir, mode, "wo"),
                             result_refine_dir=os.path.join(out_dir, mode, "it"), mode=mode, batch_size=2, device=DEV)
        _memo[mode + "_dir"] = os.path.join(out_dir, mode)
    return _memo[mode]


def _pose_diff(a, b):
    """quaternion (sign-aligned: q and -q are one rotation) and translation of two poses [7] -> the largest absolute difference"""
    q = b[:4] if np.dot(a[:4], b[:4]) >= 0 else -b[:4]
    return max(float(np.abs(a[:4] - q).max()), float(np.abs(a[4:] - b[4:]).max()))


def test_eval_ycb_f32_against_the_restated_loop(tmp_path):
    import scipy.io as scio
    want = _restated()
    res = _run("f32", str(tmp_path))
    assert sorted(res["refine"]) == sorted(res["wo_refine"]) == [0, 1, 2]
    worst = 0.0
    for now, fr in enumerate(want):
        first, last = res["wo_refine"][now], res["refine"][now]
        assert first.shape == last.shape == (len(fr), 7)
        for k, w in enumerate(fr):
            if w is None:
                assert (now, k) in res["lost"] and not first[k].any() and not last[k].any()
                continue
            assert (now, k) not in res["lost"]
            worst = max(worst, _pose_diff(w["first"], first[k]), _pose_diff(w["last"], last[k]))
        for sub, got in (("wo", first), ("it", last)):           # the files the YCB toolbox reads
            back = scio.loadmat(os.path.join(_memo["f32_dir"], sub, "%04d.mat" % now))["poses"]
            assert back.shape == (len(fr), 7) and np.array_equal(back, got)
    print("eval_ycb f32: largest |pose - restated| = %.3e over %d objects" % (worst, sum(r is not None for fr in want for r in fr)))
    assert res["lost"] == [(now, k) for now, fr in enumerate(want) for k, r in enumerate(fr) if r is None] == [(0, 4), (1, 3)]
    assert worst <= 1e-4                                         # the project's pose bar, SURVEY.md 8d


def test_eval_ycb_bf16x3_stays_near_f32(tmp_path):
    """the largest difference of a pose (sign-aligned quaternion, translation in m) to the f32 run under bf16x3 is held to four times the
    value measured over the fixture's ten objects, before and after the refinement (1.764e-5 measured on an MI355X; the
    clouds stay within 1.5 m), never above the 1e-3 cap of tests/test_gpu_linemod.py"""
    f32, b3 = _run("f32", str(tmp_path)), _run("bf16x3", str(tmp_path))
    assert b3["lost"] == f32["lost"]
    worst = 0.0
    for now in f32["refine"]:
        for key in ("wo_refine", "refine"):
            for a, b in zip(f32[key][now], b3[key][now]):
                if a.any():
                    worst = max(worst, _pose_diff(a, b))
    print("eval_ycb bf16x3: largest |pose - pose_f32| = %.3e" % worst)
    assert worst <= BF16X3_BAR <= 1e-3


BF16X3_BAR = 4 * 1.764e-5    # min(4 x the measured 1.764e-5, 1e-3); see the docstring above

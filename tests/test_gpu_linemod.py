"""The LineMOD sample builder (csrc/linemod.hip), PoseDataset.batch and DenseFusion.tools.eval_linemod.main on the GPU, against the
package's host path (PoseDataset.sample_host / ds[i]: Pillow and numpy, pinned to the reference by tests/test_linemod_host.py), against
tests/golden/linemod_dataset.npz (made by running the reference's class) and against a restatement of the reference's evaluation loop
over the oracle's networks.  Every comparison of samples is exact -- torch.equal on all six tensors -- no element excused."""
import ctypes
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

import linemod_reference as R
from test_linemod_host import CASES, GOLD, golden_sample
from autoposeestimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W, NUM = R.H, R.W, 500
CAM = (325.26110, 242.04899, 572.41140, 573.57043)
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
OPS = [("brightness", 1.13), ("contrast", 0.87), ("saturation", 1.08), ("hue", -0.031)]


def _dataset(*a, **kw):
    from autoposeestimation_amd.DenseFusion.datasets.linemod.dataset import PoseDataset
    return PoseDataset(*a, **kw)


def _same(got, want, what):
    """a device sample (as DataLoader(batch_size=1) delivers it) against a host sample"""
    assert len(got) == len(want) == 6
    for g, w, name in zip(got, want, ("cloud", "choose", "img", "target", "model_points", "idx")):
        w = w.view(1, 1) if w.dim() == 1 and w.numel() == 1 and g.dim() == 2 else w.unsqueeze(0)
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w), "%s: %s differs" % (what, name)


# ---- batch() against the host path and the reference's golden ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_batch_equals_sample_host_and_the_reference(name):
    c = CASES[name]
    order = GOLD[name + "_order"].tolist()
    random.seed(int(GOLD["seed"]))
    np.random.seed(int(GOLD["seed"]))
    ds = _dataset(c["mode"], NUM, c["add_noise"], R.tree(), c["noise_trans"], c["refine"], reference_rng=True, trancolor=R.FixedJitter())
    out, ps = ds.batch(order, return_params=True)                # one batch of mixed crop sizes; 'eval' holds a lost sample in its middle
    state = random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2]
    assert len(out) == len(order) == len(ps)
    sizes = set()
    for k, (i, got, p) in enumerate(zip(order, out, ps)):
        want = golden_sample(name, k)
        host = ds.sample_host(i, p)
        if want is None:
            assert all(t.shape == (1, 1) and t.dtype == torch.int64 and t.is_cuda and int(t) == 0 for t in got) and host[0].tolist() == [0]
            continue
        _same(got, want, "%s sample %d against the reference" % (name, k))
        _same(got, host, "%s sample %d against sample_host" % (name, k))
        sizes.add(tuple(got[2].shape[2:]))
    assert len(sizes) > 1 or name == "eval"                    # (the tree's 'eval' crops are all 40 x 40; mixed ones: the edge tests below)
    # the generators are left as the reference's loop leaves them
    random.seed(int(GOLD["seed"]))
    np.random.seed(int(GOLD["seed"]))
    for i in order:
        ds[i]
    assert (random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2]) == state
    one = ds.batch([order[1]], params=[ps[1]])                   # a batch of one
    _same(one[0], ds.sample_host(order[1], ps[1]), name + " batch of one")


def test_batches_of_five_with_seeded_draws_in_every_mode():
    for mode, noise in (("train", True), ("test", False), ("eval", False)):
        ds = _dataset(mode, NUM, noise, R.tree(), 0.03 if noise else 0.0, mode != "train", seed=3)
        idx = [0, 1, 2, 3, len(ds) - 1] if mode != "eval" else [0, 11, 12, 13, 30]
        out, ps = ds.batch(idx, return_params=True)
        for i, got, p in zip(idx, out, ps):
            host = ds[i]
            if host[0].dim() == 1:
                assert got[0].shape == (1, 1)
                continue
            _same(got, host, "%s %d against ds[i]" % (mode, i))
            _same(got, ds.sample_host(i, p), "%s %d against sample_host" % (mode, i))


# ---- edge samples, built in memory ----------------------------------------------------------------------------------------------------------
def _frame(rng, label, depth=None):
    yy, xx = np.mgrid[0:H, 0:W]
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if depth is None:
        depth = (700 + 25 * np.sin(xx / 17.0) + 15 * np.cos(yy / 13.0) + rng.integers(0, 9, (H, W))).astype(np.uint16)
    return rgb, np.ascontiguousarray(depth, np.uint16), np.ascontiguousarray(label, np.uint8)


def _rect3(r0, r1, c0, c1, bands=3):
    lab = np.zeros((H, W, bands), np.uint8)
    lab[r0:r1, c0:c1] = 255
    return lab


def _edge_cases():
    """name -> (frame, obj_bb, expected count or None)"""
    rng = np.random.default_rng(41)
    full = np.full((H, W, 3), 255, np.uint8)
    cases = {}
    for name, bb in (("over_top", [300, -20, 50, 60]), ("over_left", [-30, 200, 70, 50]), ("over_bottom", [100, 440, 60, 90]),
                     ("over_right", [600, 100, 90, 60]), ("corner", [-5, -5, 30, 30])):
        cases[name] = (_frame(rng, full), bb, None)             # the crop is shifted inside; mask pixels all around it
    cases["crop_40x40"] = (_frame(rng, full), [200, 100, 40, 40], None)
    cases["crop_480x640"] = (_frame(rng, _rect3(3, 470, 7, 633)), [0, 0, 640, 480], None)
    cases["mask_outside_on_all_sides"] = (_frame(rng, _rect3(50, 400, 60, 600)), [250, 180, 100, 70], None)
    dense = lambda: (700 + rng.integers(0, 50, (H, W))).astype(np.uint16)  # noqa: E731
    lab = _rect3(100, 120, 200, 225)                             # 20 x 25 = 500 pixels inside the crop of [190, 90, 50, 40]
    cases["count_num"] = (_frame(rng, lab, dense()), [190, 90, 50, 40], 500)
    lab = _rect3(100, 120, 200, 225); lab[119, 224] = 0
    cases["count_num_minus_1"] = (_frame(rng, lab, dense()), [190, 90, 50, 40], 499)
    lab = _rect3(100, 120, 200, 225); lab[120, 200] = 255
    cases["count_num_plus_1"] = (_frame(rng, lab, dense()), [190, 90, 50, 40], 501)
    lab = _rect3(100, 101, 200, 201)
    cases["count_1"] = (_frame(rng, lab, dense()), [190, 90, 50, 40], 1)
    lab = _rect3(300, 320, 20, 45)                               # labelled, but outside the crop
    cases["count_0"] = (_frame(rng, lab, dense()), [190, 90, 50, 40], 0)
    one = np.zeros((H, W), np.uint16); one[210, 333] = 812
    cases["depth_one_pixel"] = (_frame(rng, _rect3(150, 280, 250, 420), one), [250, 150, 170, 130], 1)
    lab = np.zeros((H, W, 3), np.uint8); lab[100:160, 100:180, 0] = 255; lab[90:200, 60:140, 1] = 255; lab[100:160, 100:180, 2] = 254
    lab[120:130, 110:150, 0] = 254
    cases["bands_differ"] = (_frame(rng, lab, dense()), [95, 95, 90, 70], 60 * 80 - 10 * 40)
    return cases


def _build(frames, boxes, eval_mode, add_noise, params, subsets):
    """-> per sample the device views or None, and the counts"""
    from autoposeestimation_amd.DenseFusion.datasets import packed
    from autoposeestimation_amd.DenseFusion.datasets.linemod import augment as G
    dev = [tuple(torch.from_numpy(x).to(DEV) for x in f) for f in frames]
    st = G.count(dev, params, boxes, eval_mode, add_noise, CAM, NUM)
    sels = [None if c == 0 else packed.selection(int(c), NUM, subsets[k]) for k, c in enumerate(st.counts)]
    return G.samples(st, sels, MEAN, STD), st.counts


def _host(frame, box, eval_mode, add_noise, p, subset):
    from autoposeestimation_amd.DenseFusion.datasets.linemod.dataset import host_arrays
    from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import ColorJitterPIL
    rgb, depth, label = frame
    if add_noise:
        rgb = np.array(ColorJitterPIL.apply(Image.fromarray(rgb), p["ops"]))
    return host_arrays(rgb, depth, label, eval_mode, box, NUM, CAM, np.array(p["add_t"], np.float64) if add_noise else None, subset)


def _compare_views(views, hosts, names):
    for v, h, name in zip(views, hosts, names):
        if h is None:
            assert v is None, name
            continue
        for g, w, what in zip(v, h, ("cloud", "choose", "img")):
            assert g.dtype == w.dtype and torch.equal(g.cpu()[0], w), "%s: %s differs" % (name, what)


def _subsets(frames, boxes, rng):
    """for every sample with more than NUM valid in-crop pixels: NUM sorted ranks, drawn here"""
    from autoposeestimation_amd.DenseFusion.datasets.linemod.dataset import get_bbox
    out = []
    for (rgb, depth, label), bb in zip(frames, boxes):
        rmin, rmax, cmin, cmax = get_bbox(list(bb))
        band0 = label if label.ndim == 2 else label[:, :, 0]
        count = int(((band0 == 255) & (depth != 0))[rmin:rmax, cmin:cmax].sum())
        out.append(np.sort(rng.choice(count, NUM, replace=False)) if count > NUM else None)
    return out


def test_edge_samples_equal_the_host_arithmetic():
    cases = _edge_cases()
    names = list(cases)
    frames, boxes = [cases[n][0] for n in names], [cases[n][1] for n in names]
    subsets = _subsets(frames, boxes, np.random.default_rng(2))
    views, counts = _build(frames, boxes, False, False, [{} for _ in names], subsets)
    for n, c in zip(names, counts):
        if cases[n][2] is not None:
            assert int(c) == cases[n][2], n
    assert views[names.index("count_0")] is None and views[names.index("count_1")] is not None
    assert tuple(views[names.index("crop_40x40")][2].shape) == (1, 3, 40, 40) and tuple(views[names.index("crop_480x640")][2].shape) == (1, 3, 480, 640)
    for n in ("over_top", "over_left", "over_bottom", "over_right", "corner", "mask_outside_on_all_sides"):
        v = views[names.index(n)]
        hc, wc = v[2].shape[2:]
        assert int(counts[names.index(n)]) <= hc * wc and int(v[1].max()) < hc * wc, n       # nothing outside the crop is counted or chosen
    _compare_views(views, [_host(f, b, False, False, {}, s) for f, b, s in zip(frames, boxes, subsets)], names)


def test_edge_samples_with_jitter_and_translation_noise():
    """add_noise: the jitter of the whole frame (a contrast among the ops: its mean is over the frame, not the crop) and an add_t whose
    float32 and float64 sums differ in the last bit for some points"""
    cases = _edge_cases()
    names = ["over_left", "mask_outside_on_all_sides", "count_num_minus_1", "bands_differ"]
    frames, boxes = [cases[n][0] for n in names], [cases[n][1] for n in names]
    add_t = [0.012345678901, -0.0298765432101, 0.0100000123]
    params = [{"ops": OPS[k % 4:] + OPS[:k % 4], "add_t": add_t} for k in range(len(names))]
    subsets = _subsets(frames, boxes, np.random.default_rng(3))
    views, _ = _build(frames, boxes, False, True, params, subsets)
    hosts = [_host(f, b, False, True, p, s) for f, b, p, s in zip(frames, boxes, params, subsets)]
    _compare_views(views, hosts, names)
    plain = _host(frames[1], boxes[1], False, False, {}, subsets[1])[0].numpy()
    in32 = plain + np.array(add_t, np.float32)
    assert (in32 != hosts[1][0].numpy()).any()                   # adding in float32 would differ: the case tells the two apart


def test_eval_mode_crops_around_the_largest_contour():
    rng = np.random.default_rng(43)
    labs = []
    a = np.zeros((H, W), np.uint8); a[100:180, 200:330] = 255; a[130:140, 250:260] = 0; a[300:306, 500:509] = 255; a[5:60, 5:300] = 128
    labs.append(a)                                               # a hole, an extra blob, a larger region of another value
    a = np.zeros((H, W), np.uint8); a[440:478, 600:638] = 255
    labs.append(a)                                               # at the far corner: the crop is shifted inside
    labs.append(np.zeros((H, W), np.uint8))                      # no detection: the crop of get_bbox([0, 0, 0, 0]) holds nothing
    a = np.zeros((H, W), np.uint8); i = np.arange(100); a[50 + i, 80 + i] = 255; a[300:340, 300:340] = 255
    labs.append(a)                                               # the diagonal's box wins; most of its crop is empty
    frames = [_frame(rng, lab) for lab in labs]
    boxes = [None] * len(frames)
    subsets = []
    from autoposeestimation_amd.DenseFusion.datasets.linemod.dataset import get_bbox, mask_to_bbox
    for rgb, depth, lab in frames:
        rmin, rmax, cmin, cmax = get_bbox(mask_to_bbox(lab == 255))
        count = int(((lab == 255) & (depth != 0))[rmin:rmax, cmin:cmax].sum())
        subsets.append(np.sort(np.random.default_rng(count).choice(count, NUM, replace=False)) if count > NUM else None)
    views, counts = _build(frames, boxes, True, False, [{} for _ in frames], subsets)
    assert views[2] is None and int(counts[2]) == 0
    _compare_views(views, [_host(f, None, True, False, {}, s) for f, s in zip(frames, subsets)], ["hole_blob", "corner", "empty", "diagonal"])


# ---- the largest-contour box ----------------------------------------------------------------------------------------------------------------
def test_largest_contour_boxes_equal_mask_to_bbox():
    from autoposeestimation_amd.DenseFusion.datasets.linemod import augment as G
    from autoposeestimation_amd.DenseFusion.datasets.linemod.dataset import mask_to_bbox
    masks = R.masks()
    a = np.zeros((H, W), bool); a[10:20, 600:640] = True; a[400:440, 0:10] = True; a[200:205, 300:305] = True
    masks["equal_areas"] = a                                     # 40 x 10 and 10 x 40: the tie goes to the first in raster order
    names = list(masks)
    labs = []
    for k, n in enumerate(names):
        lab = masks[n].astype(np.uint8) * 255
        if k % 3 == 0:
            lab[(~masks[n]) & (np.add.outer(np.arange(H), np.arange(W)) % 7 == 0)] = 254      # other values are not the object
        labs.append(torch.from_numpy(lab).to(DEV))
    assert names.index("empty") not in (0, len(names) - 1) or len(names) > 2                  # an empty frame inside the batch
    want = [mask_to_bbox(masks[n]) for n in names]
    got = G.largest_boxes(labs).cpu().numpy()
    again = G.largest_boxes(labs).cpu().numpy()
    assert np.array_equal(got, again)                            # integer min / max only: two launches agree
    for n, g, w in zip(names, got.tolist(), want):
        assert g == w, n
    assert want[names.index("equal_areas")] == [600, 10, 40, 10] and want[names.index("empty")] == [0, 0, 0, 0]
    assert G.largest_boxes(labs[:1]).cpu().numpy().tolist() == want[:1]
    rev = G.largest_boxes(labs[::-1]).cpu().numpy().tolist()    # a frame's box does not depend on its place in the batch
    assert rev == want[::-1]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_jobs_are_refused_without_a_launch():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import sample_jobs as J
    from autoposeestimation_amd.DenseFusion.datasets.linemod.augment import LinemodJob
    L = _lib.lib()
    rng = np.random.default_rng(47)
    host = _frame(rng, _rect3(100, 200, 100, 200))
    host[1][rng.random((H, W)) < 0.05] = 0
    rgb, depth, label = (torch.from_numpy(x).to(DEV) for x in host)
    ws_bytes = L.ape_linemod_workspace_bytes(1, H, NUM)
    ws = torch.full((ws_bytes + 64,), 0x5a, dtype=torch.uint8, device=DEV)
    out_bytes = L.ape_pose_train_sample_bytes(NUM, 120, 120)
    out = torch.full((out_bytes + 64,), 0x5a, dtype=torch.uint8, device=DEV)
    m, sd = J.norm(MEAN, STD, 3)

    def job(rmin=90, rmax=210, cmin=90, cmax=210):
        jobs = (LinemodJob * 1)()
        j = jobs[0]
        j.rgb, j.depth, j.label, j.label_bands = rgb.data_ptr(), depth.data_ptr(), label.data_ptr(), 3
        j.cam_cx, j.cam_cy, j.cam_fx, j.cam_fy, j.cam_scale = CAM + (1.0,)
        j.rmin, j.rmax, j.cmin, j.cmax = rmin, rmax, cmin, cmax
        return jobs

    def rows(jobs, ws_ptr=None, nbytes=None):
        return L.ape_linemod_rows(ctypes.cast(jobs, ctypes.c_void_p), 1, H, W, ctypes.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr),
                                  ws_bytes if nbytes is None else nbytes, _lib.stream_ptr())

    def samples(jobs, out_ptr=None, nbytes=None, obytes=None):
        return L.ape_linemod_samples(ctypes.cast(jobs, ctypes.c_void_p), 1, H, W, NUM, m, sd,
                                     ctypes.c_void_p(out.data_ptr() if out_ptr is None else out_ptr), out_bytes if obytes is None else obytes,
                                     ctypes.c_void_p(ws.data_ptr()), ws_bytes if nbytes is None else nbytes, _lib.stream_ptr())

    EINVAL = -1
    for bad in (job(rmin=400, rmax=520), job(cmin=-40, cmax=80), job(cmin=600, cmax=680),       # a crop outside the frame
                job(rmax=200), job(cmax=215), job(rmin=100, rmax=100)):                         # a side that is no multiple of 40
        assert rows(bad) == EINVAL and samples(bad) == EINVAL
    assert rows(job(), nbytes=L.ape_linemod_tables_offset(1, H) - 1) == EINVAL                  # a short workspace
    assert samples(job(), nbytes=ws_bytes - 1) == EINVAL
    assert rows(job(), ws_ptr=ws.data_ptr() + 8) == EINVAL                                      # a misaligned workspace
    assert samples(job(), out_ptr=out.data_ptr() + 8) == EINVAL                                 # a misaligned output
    assert samples(job(), obytes=out_bytes - 16) == EINVAL                                      # a sample that does not fit
    off = job(); off[0].out_off = 8
    assert samples(off) == EINVAL
    box = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    ptrs = (ctypes.c_void_p * 1)(label[:, :, 0].contiguous().data_ptr())
    bws = torch.empty(L.ape_linemod_box_workspace_bytes(1, H, W), dtype=torch.uint8, device=DEV)
    assert L.ape_linemod_boxes(ctypes.cast(ptrs, ctypes.c_void_p), 1, H, W, ctypes.c_void_p(box.data_ptr()), ctypes.c_void_p(bws.data_ptr()),
                               bws.numel() - 1, _lib.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((ws == 0x5a).all()) and bool((out == 0x5a).all()) and box.tolist() == [-7] * 4  # nothing was launched
    assert rows(job()) == 0                                      # and the good job goes through
    torch.cuda.synchronize()
    r0 = L.ape_linemod_rows_offset(1)
    got = ws[r0:r0 + 4 * H].cpu().numpy().view(np.int32)
    want = (host[2][:, :, 0] == 255) & (host[1] != 0)
    want[:, :90] = False; want[:, 210:] = False; want[:90] = False; want[210:] = False
    assert np.array_equal(got, want.sum(axis=1))


# ---- through the training loop --------------------------------------------------------------------------------------------------------------
class _First:
    """the first n samples of a data set, as `Batches` reads one"""

    def __init__(self, ds, n):
        self.ds, self.n = ds, n

    def __len__(self):
        return self.n

    def batch(self, indices):
        return self.ds.batch(indices)


def test_linemod_dataset_feeds_batches_and_train_epoch():
    from autoposeestimation_amd.autograd import Adam
    from autoposeestimation_amd.DenseFusion.lib.loss import Loss
    from autoposeestimation_amd.DenseFusion.lib.loss_refiner import Loss_refine
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet
    from autoposeestimation_amd.DenseFusion.tools.train import Batches, train_epoch
    ds = _dataset("train", NUM, True, R.tree(), 0.03, False, seed=5)
    est, ref = PoseNet(NUM, 13), PoseRefineNet(NUM, 13)
    est.load_state_dict(S.posenet_state_dict(13, seed=7))
    ref.load_state_dict(S.refiner_state_dict(13, seed=8))
    est.to(DEV)
    ref.to(DEV)
    crit, crit_r = Loss(ds.get_num_points_mesh(), ds.get_sym_list()), Loss_refine(ds.get_num_points_mesh(), ds.get_sym_list())
    opt = SimpleNamespace(w=0.015, refine_start=False, iteration=2, batch_size=4, repeat_epoch=1)
    loader = Batches(_First(ds, 6), opt, shuffle=False)
    st = train_epoch(est, ref, Adam(est.parameters(), lr=1e-4), crit, crit_r, loader, opt)
    assert st["samples"] == 6 and st["optimizer_steps"] == 2 and np.isfinite(st["loss"]) and np.isfinite(st["train_dis"])
    opt.refine_start = True
    st = train_epoch(est, ref, Adam(ref.parameters(), lr=1e-4), crit, crit_r, loader, opt)
    assert st["samples"] == 6 and st["optimizer_steps"] == 2 and np.isfinite(st["loss"]) and np.isfinite(st["refiner_loss"])


# ---- the benchmark driver -------------------------------------------------------------------------------------------------------------------
_memo = {}


def _restated():
    if "restated" not in _memo:
        from autoposeestimation_amd.DenseFusion.tools import eval_linemod as D
        ds = _dataset("eval", NUM, False, R.tree(), 0.0, True)
        _memo["diameter"] = D.read_diameters(R.tree())
        _memo["restated"] = R.restated_eval(ds, S.posenet_state_dict(13, 0), S.refiner_state_dict(13, 0), _memo["diameter"])
    return _memo["restated"], _memo["diameter"]


def _run(precision, out_dir=None):
    if precision not in _memo:
        from autoposeestimation_amd.DenseFusion.tools import eval_linemod as D
        _memo[precision] = D.main(R.tree(), S.posenet_state_dict(13, 0), S.refiner_state_dict(13, 0), output_result_dir=out_dir,
                                  precision=precision, device=DEV)
    return _memo[precision]


def _strip(line):
    return line.split("Distance:")[0]


def test_eval_linemod_f32_against_the_restated_loop(tmp_path):
    want, diameter = _restated()
    res = _run("f32", str(tmp_path))
    assert len(res["dis"]) == len(want)
    worst = 0.0
    lines = []
    success, count = [0] * 13, [0] * 13
    for i, (d, w) in enumerate(zip(res["dis"], want)):
        if w is None:
            assert d is None and i in res["lost"]
            lines.append("No.{0} NOT Pass! Lost detection!".format(i))
            continue
        worst = max(worst, abs(d - w["dis"]))
        lines.append("No.{0} {1}Pass! ".format(i, "" if w["ok"] else "NOT "))
        success[w["idx"]] += int(w["ok"])
        count[w["idx"]] += 1
    print("eval_linemod f32: largest |dis - restated| = %.3e m over %d samples" % (worst, sum(count)))
    assert worst <= 1e-4                                         # the project's ADD-S bar, SURVEY.md 8d
    assert res["success_count"] == success and res["num_count"] == count and res["lost"] == [i for i, w in enumerate(want) if w is None]
    log = open(os.path.join(str(tmp_path), "eval_result_logs.txt")).read().split("\n")
    assert [_strip(x) for x in log[:len(lines)]] == lines
    rates = ["Object {0} success rate: {1}".format(R.OBJLIST[k], float(success[k]) / count[k] if count[k] else float("nan")) for k in range(13)]
    assert log[len(lines):] == rates + ["ALL success rate: {0}".format(float(sum(success)) / sum(count)), ""]
    for i, d in enumerate(res["dis"]):
        if d is not None:
            assert log[i].endswith("Distance: {0}".format(d))


def test_eval_linemod_bf16x3_keeps_the_flags():
    """|dis - dis_f32| under bf16x3 is held to four times the largest difference measured over the fixture's samples (DESIGN.md 6m:
    4.824e-4 m measured over the 24 counted samples of the synthetic tree, whose far points stretch the clouds to 63 m; four times
    that is above the cap, so the bar is the cap), never above 1e-3 m"""
    want, diameter = _restated()
    f32, b3 = _run("f32"), _run("bf16x3")
    worst = 0.0
    for d0, d1, w in zip(f32["dis"], b3["dis"], want):
        assert (d0 is None) == (d1 is None)
        if d0 is not None:
            worst = max(worst, abs(d1 - d0))
            assert (d1 < diameter[w["idx"]]) == w["ok"]
    print("eval_linemod bf16x3: largest |dis - dis_f32| = %.3e m" % worst)
    assert b3["success_count"] == f32["success_count"] and b3["num_count"] == f32["num_count"] and b3["lost"] == f32["lost"]
    assert worst <= BF16X3_BAR <= 1e-3


BF16X3_BAR = 1e-3            # min(4 x the measured 4.824e-4 m, 1e-3 m); see the docstring above

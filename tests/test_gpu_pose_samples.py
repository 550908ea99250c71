"""DenseFusion's training-sample builder (csrc/pose_train.hip), PoseDataset.batch and DenseFusion.tools.train.main on the GPU, against the
package's host path (PoseDataset.sample_host / ds[i]: Pillow and numpy, pinned to the reference by tests/test_pose_dataset_golden.py)
and against tests/golden/pose_dataset.npz (made by running the reference's class).  Every comparison of samples is exact -- torch.equal
/ np.array_equal on the fp32 image, the fp32 points, the i64 choose, target, model points and idx -- no element excused."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import pose_samples_reference as R
from autoposeestimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "pose_dataset.npz"))
CASES = {"train_noise": dict(mode="train", add_noise=True, noise_trans=0.03, p_extra_data=0.5, p_viewpoints=0.75),
         "train_plain": dict(mode="train", add_noise=False, noise_trans=0.0, p_extra_data=0.0, p_viewpoints=1.0),
         "test": dict(mode="test", add_noise=False, noise_trans=0.0, p_extra_data=0.0, p_viewpoints=1.0)}
MEAN = torch.tensor([0.485, 0.456, 0.406])[:, None, None]
STD = torch.tensor([0.229, 0.224, 0.225])[:, None, None]


def _dataset(*a, **kw):
    from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import PoseDataset
    return PoseDataset(*a, **kw)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("posedata"))
    S.pose_dataset_tree(root)
    return root


def _made_frames():
    """the hand-made frames, by name"""
    rng = np.random.default_rng(17)
    holes = np.zeros((R.H, R.W), bool)
    holes[100:110, 200:210] = True
    f = {
        "top_left": R.frame(rng, R.ellipse(26, 33, 24.4, 29.3)),                   # get_bbox shifts down and right (rmin < 0, cmin < 0)
        "far_corner": R.frame(rng, R.ellipse(440, 600, 36.2, 37.7)),               # rotations carry part of it out of the frame
        "multiple_of_40": R.frame(rng, R.rect(160, 240, 300, 420)),                # tight extents 80 x 120
        "big": R.frame(rng, R.ellipse(250, 300, 90.5, 140.2)),
        "rect_500": R.frame(rng, R.rect(100, 120, 200, 225), zero_depth=0),        # 20 x 25 pixels, all with depth
        "rect_501": R.frame(rng, R.rect(100, 120, 200, 225) | R.rect(120, 121, 200, 201), zero_depth=0),
        "seven": R.frame(rng, R.rect(300, 301, 400, 407), zero_depth=0),
        "holes": R.frame(rng, R.rect(90, 130, 190, 230), zero_depth=0, depth_holes=holes),      # 1600 labelled, 100 without depth
        "no_depth": R.frame(rng, R.rect(50, 70, 60, 90), zero_depth=0, depth_holes=R.rect(40, 80, 50, 100) > 0),
        "label_254": R.frame(rng, R.rect(50, 70, 60, 90, value=254)),
    }
    return f


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("posemade"))
    frames = _made_frames()
    R.write_tree(root, "made", list(frames.values()))
    return root, {name: k for k, name in enumerate(frames)}, frames


def _dellist(ds, rng):
    return sorted(rng.choice(1200, 1200 - ds.num_pt_mesh, replace=False).tolist())


def _subsets(ds, params, rng):
    """fills in `subset` where the host path finds more valid pixels than points: params as a caller would inject them"""
    for i, p in params:
        rel, lmode = ds.list[i], ds.label_mode
        _, depth, label = ds._open(rel, lmode)
        angle = p.get("angle") if ds.add_noise else None
        if angle is not None:
            depth, label = depth.rotate(angle), label.rotate(angle)
        count = int(((np.array(label) == 255) & (np.array(depth) != 0)).sum())
        if count > ds.num_pt:
            p["subset"] = np.sort(rng.choice(count, ds.num_pt, replace=False))
        p["count"] = count
    return params


def _against_host(ds, pairs, what):
    """ds.batch with injected parameters against sample_host with the same, sample by sample"""
    got = ds.batch([i for i, _ in pairs], params=[p for _, p in pairs])
    assert len(got) == len(pairs)
    for k, (i, p) in enumerate(pairs):
        want = R.as_loader(ds.sample_host(i, dict(p, entry=(ds.list[i], ds.label_mode))))
        diff = [int((a.cpu() != b).sum()) if tuple(a.shape) == tuple(b.shape) else -1 for a, b in zip(got[k][:6], want)]
        print("%s sample %d (index %d, angle %r, %d ops, count %d): crop %s, differing elements %r"
              % (what, k, i, p.get("angle"), len(p.get("ops") or []), p["count"], tuple(got[k][2].shape[2:]), diff))
        assert all(t.is_cuda for t in got[k][:6])
        assert R.same(got[k], want), (what, k, diff)
    return got


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_golden_through_the_device_path(tree, name):
    """the reference's own samples, extra-data mixing and its wrap included, from one ds.batch(order)"""
    c = CASES[name]
    seed = int(GOLD["seed"])
    random.seed(seed)
    np.random.seed(seed)
    ds = _dataset(c["mode"], 500, c["add_noise"], c["noise_trans"], False, "synth", tree, p_extra_data=c["p_extra_data"],
                  p_viewpoints=c["p_viewpoints"], label_mode="new_pred", reference_rng=True, trancolor=R.FixedJitter())
    order = GOLD[name + "_order"].tolist()
    out = ds.batch(order)
    assert len(out) == len(order)
    for k, s in enumerate(out):
        assert len(s) == (8 if c["mode"] == "test" else 6)
        pre = "%s_%d_" % (name, k)
        crop = torch.from_numpy(GOLD[pre + "crop"])
        assert np.array_equal(s[1].cpu().numpy(), GOLD[pre + "choose"][None]), (name, k, "choose")
        assert np.array_equal(s[0].cpu().numpy(), GOLD[pre + "cloud"][None]), (name, k, "cloud")
        assert torch.equal(s[2].cpu(), ((crop.float() - MEAN) / STD)[None]), (name, k, "image")
        assert np.array_equal(s[4].cpu().numpy(), GOLD[pre + "model"][None]), (name, k, "model points")
        assert np.array_equal(s[3].cpu().numpy(), GOLD[pre + "target"][None]), (name, k, "target")
        assert np.array_equal(s[5].cpu().numpy(), GOLD[pre + "idx"][None])
        assert s[0].dtype == torch.float32 and s[1].dtype == torch.int64 and s[5].dtype == torch.int64
    if c["mode"] == "test":
        assert set(out[0][6]) == {"fx", "fy", "ppx", "ppy"} and out[0][7].dtype == torch.uint8 and tuple(out[0][7].shape) == (1, 480, 640, 3)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_builder_equals_sample_host_mixed_batch(made):
    root, at, frames = made
    rng = np.random.default_rng(2)
    t = lambda: list(rng.uniform(-0.03, 0.03, 3))  # noqa: E731
    ds = R.dataset(root, "made", 500, True, device=DEV)
    pairs = [(at["top_left"], {"ops": R.OPS, "angle": None, "add_t": t()}),                         # shifts: rmin < 0, cmin < 0
             (at["top_left"], {"ops": R.OPS[::-1], "angle": 180.0, "add_t": t()}),                  # now bottom right: rmax > 480, cmax > 640
             (at["far_corner"], {"ops": [], "angle": 33.3, "add_t": t()}),
             (at["far_corner"], {"ops": [R.OPS[1]], "angle": -120.5, "add_t": t()}),
             (at["multiple_of_40"], {"ops": R.OPS, "angle": None, "add_t": t()}),
             (at["big"], {"ops": R.OPS[::-1], "angle": -120.5, "add_t": t()}),
             (at["seven"], {"ops": [R.OPS[3], R.OPS[0]], "angle": 33.3, "add_t": t()})]
    for _, p in pairs:
        p["dellist"] = _dellist(ds, rng)
    _subsets(ds, pairs, rng)
    got = _against_host(ds, pairs, "noise, N = 500")
    # the cases are the ones meant
    from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import bbox_from_extents
    lab = frames["top_left"][2]
    rows, cols = np.where(lab.any(1))[0], np.where(lab.any(0))[0]
    assert rows[0] < 20 and cols[0] < 20 and bbox_from_extents(rows[0], rows[-1], cols[0], cols[-1])[::2] == (0, 0)
    assert tuple(got[0][2].shape) == (1, 3, 80, 80) and tuple(got[1][2].shape) == (1, 3, 80, 80)
    turned = np.array(Image.fromarray(lab).rotate(180.0))
    rows, cols = np.where(turned.any(1))[0], np.where(turned.any(0))[0]
    assert bbox_from_extents(rows[0], rows[-1], cols[0], cols[-1])[1::2] == (480, 640) and rows[-1] + 41 > 480 and cols[-1] + 41 > 640
    for k in (2, 3):                                                # part of the object left the frame: zero fill
        assert 0 < pairs[k][1]["count"] and (np.array(Image.fromarray(frames["far_corner"][2]).rotate(pairs[k][1]["angle"])) == 255).sum() \
            < (frames["far_corner"][2] == 255).sum() - 200
    assert tuple(got[4][2].shape) == (1, 3, 80, 120)                # exact multiples of 40 stay as they are
    assert pairs[5][1]["count"] > 500 and pairs[6][1]["count"] < 20             # 7 pixels, resampled
    # without noise: no jitter, no rotation, no add_t; N = 1000; and millimetres
    plain = R.dataset(root, "made", 1000, False, device=DEV)
    pairs = _subsets(plain, [(at[n], {"dellist": _dellist(plain, rng)}) for n in ("big", "holes", "far_corner")], rng)
    _against_host(plain, pairs, "plain, N = 1000")
    mm = R.dataset(root, "made", 1000, True, to_meter=False, device=DEV)
    pairs = _subsets(mm, [(at["big"], {"ops": R.OPS, "angle": 33.3, "add_t": t(), "dellist": _dellist(mm, rng)}),
                          (at["multiple_of_40"], {"ops": [], "angle": 180.0, "add_t": t(), "dellist": _dellist(mm, rng)})], rng)
    got = _against_host(mm, pairs, "millimetres, N = 1000")
    assert float(got[0][0][0, :, 2].min()) > 400.0                  # depth in millimetres


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_count_boundaries(made):
    """no noise, so no rotation: the counts hold by construction.  The batch against ds[i] from the same seeds, and the `c_mask` shuffle
    is drawn only above N."""
    root, at, _ = made
    names = ["rect_500", "rect_501", "seven", "holes"]
    states = {}
    for n_idx, name in enumerate(names):
        for path in ("host", "device"):
            ds = R.dataset(root, "made", 500, False, reference_rng=True, device=DEV)
            random.seed(40 + n_idx)
            np.random.seed(40 + n_idx)
            s = R.as_loader(ds[at[name]]) if path == "host" else ds.batch([at[name]])[0]
            states[(name, path)] = (s, random.getstate(), np.random.get_state())
        (a, ra, na), (b, rb, nb) = states[(name, "host")], states[(name, "device")]
        assert R.same(b, a), name
        assert ra == rb and all(np.array_equal(x, y) for x, y in zip(na, nb)), name
    np.random.seed(40)
    untouched = np.random.get_state()
    assert all(np.array_equal(x, y) for x, y in zip(states[("rect_500", "device")][2], untouched))          # count = N: no draw
    np.random.seed(41)
    assert not all(np.array_equal(x, y) for x, y in zip(states[("rect_501", "device")][2], np.random.get_state()))    # N + 1: the subset
    ch = states[("rect_500", "device")][0][1].cpu().numpy().reshape(-1)
    assert len(set(ch.tolist())) == 500 and np.array_equal(ch, np.sort(ch))
    ch = states[("rect_501", "device")][0][1].cpu().numpy().reshape(-1)
    assert len(set(ch.tolist())) == 500 and np.array_equal(ch, np.sort(ch))
    ch = states[("seven", "device")][0][1].cpu().numpy().reshape(-1)
    assert np.array_equal(ch, np.tile(ch[:7], 72)[:500]) and len(set(ch[:7].tolist())) == 7                  # wraps 71 times
    ch = states[("holes", "device")][0][1].cpu().numpy().reshape(-1)
    assert len(set(ch.tolist())) == 500                              # 1500 valid pixels of 1600 labelled
    ds = R.dataset(root, "made", 500, False, device=DEV)
    for name in ("no_depth", "label_254"):
        with pytest.raises(ValueError, match="%06d" % at[name]):
            ds.batch([at["seven"], at[name]])
        with pytest.raises(ValueError, match="%06d" % at[name]):
            ds[at[name]]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_17_samples_cross_the_job_chunk(tree):
    ds = _dataset("train", 500, True, 0.03, False, "synth", tree, p_extra_data=0.0, seed=6, device=DEV)
    indices = [i % len(ds) for i in range(17)]
    a, params = ds.batch(indices, return_params=True)
    b = ds.batch(indices)
    assert len(a) == 17 and all(R.same(x, y) for x, y in zip(a, b))
    one = ds.batch([indices[16]], params=[params[16]])
    assert R.same(one[0], a[16])
    one = ds.batch([indices[5], indices[16], indices[0]])
    assert R.same(one[0], a[5]) and R.same(one[1], a[16]) and R.same(one[2], a[0])
    for k in (0, 7, 15, 16):                                        # both sides of the chunk boundary against the host path
        assert R.same(a[k], R.as_loader(ds[indices[k]])), k
        assert R.same(a[k], R.as_loader(ds.sample_host(indices[k], params[k]))), k


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_seeded_mode_equals_getitem_and_leaves_the_global_generators(tree):
    ds = _dataset("train", 500, True, 0.03, False, "synth", tree, p_extra_data=0.25, seed=9, device=DEV)
    random.seed(123)
    np.random.seed(123)
    r0, n0 = random.getstate(), np.random.get_state()
    got = ds.batch([5, 3, 0])
    assert random.getstate() == r0 and all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), n0))
    want = [ds[5], ds[3], ds[0]]
    assert random.getstate() == r0 and all(np.array_equal(x, y) for x, y in zip(np.random.get_state(), n0))
    for g, w in zip(got, want):
        assert R.same(g, R.as_loader(w))


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_reference_stream_mode_leaves_both_generators_as_getitem_does(made):
    """`big` has more valid pixels than points under every rotation (a shuffle from numpy.random), `seven` and `rect_500` never"""
    root, at, _ = made
    indices = [at["big"], at["seven"], at["multiple_of_40"], at["rect_500"]]
    out = {}
    for path in ("host", "device"):
        ds = R.dataset(root, "made", 1000, True, reference_rng=True, device=DEV)
        random.seed(77)
        np.random.seed(77)
        s = [R.as_loader(ds[i]) for i in indices] if path == "host" else ds.batch(indices)
        out[path] = (s, random.getstate(), np.random.get_state())
    for a, b in zip(out["host"][0], out["device"][0]):
        assert R.same(b, a)
    assert out["host"][1] == out["device"][1]
    assert all(np.array_equal(x, y) for x, y in zip(out["host"][2], out["device"][2]))
    np.random.seed(77)
    assert not all(np.array_equal(x, y) for x, y in zip(out["device"][2], np.random.get_state()))          # a shuffle was drawn


def test_batch_refuses_a_bare_callable_jitter_and_other_frame_sizes(tree, tmp_path):
    ds = _dataset("train", 500, True, 0.03, False, "synth", tree, p_extra_data=0.0, trancolor=lambda img: img, device=DEV)
    assert len(ds[0]) == 6
    with pytest.raises(TypeError, match="callable"):
        ds.batch([0])
    root = str(tmp_path)
    rng = np.random.default_rng(1)
    rels = R.write_tree(root, "small", [R.frame(rng, R.rect(100, 150, 100, 150)) for _ in range(2)])
    path = os.path.join(root, "data_generation/data", rels[1] + ".color.png")
    Image.open(path).crop((0, 0, 320, 240)).save(path)
    ds = R.dataset(root, "small", 500, False, device=DEV)
    assert len(ds.batch([0])) == 1
    with pytest.raises(ValueError, match=rels[1]):
        ds.batch([0, 1])


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_return_errors_without_launching():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented import augment as A
    L = _lib.lib()
    h, w, n = 480, 640, 64
    rgb = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    depth = torch.ones(h, w, dtype=torch.uint16, device=DEV)
    label = torch.zeros(h, w, dtype=torch.uint8, device=DEV)
    need = L.ape_pose_train_workspace_bytes(1, h, n)
    assert L.ape_pose_train_extents_offset(1) == 64 * 8 and L.ape_pose_train_rows_offset(1) == 64 * 8 + 64 * 16
    assert L.ape_pose_train_tables_offset(1, h) == 64 * 24 + h * 4 and L.ape_pose_train_sel_offset(1, h) == 64 * 24 + 2 * h * 4
    assert need == 64 * 24 + 2 * h * 4 + n * 4
    assert L.ape_pose_train_image_offset(n) == 20 * n and L.ape_pose_train_sample_bytes(n, 40, 80) == 20 * n + 12 * 40 * 80
    assert L.ape_pose_train_image_offset(5) == 112 and L.ape_pose_train_sample_bytes(5, 40, 40) == 112 + 12 * 1600
    nbytes = L.ape_pose_train_sample_bytes(n, 40, 80)
    ws = torch.full((need,), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((nbytes + 16,), 7, dtype=torch.uint8, device=DEV)
    m, sd = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)

    def job(box=(0, 40, 0, 80), rgb_ptr=rgb.data_ptr(), off=0):
        j = A.make_job({}, h, w, rgb_ptr, depth.data_ptr(), label.data_ptr(), R.INTR, R.DEPTH_SCALE, True, False)
        A.set_crop(j, box)
        j.out_off = off
        return j

    def run(j, out_ptr=None, out_bytes=nbytes, ws_bytes=need, ws_ptr=None):
        jobs = (_lib.PoseTrainJob * 1)(j)
        return L.ape_pose_train_samples(ctypes.cast(jobs, ctypes.c_void_p), 1, h, w, n, ctypes.cast(m, ctypes.c_void_p),
                                        ctypes.cast(sd, ctypes.c_void_p), out_ptr or _lib.dptr(out), out_bytes, ws_ptr or _lib.dptr(ws), ws_bytes,
                                        _lib.stream_ptr())

    def stats(j, ws_bytes):
        jobs = (_lib.PoseTrainJob * 1)(j)
        return L.ape_pose_train_stats(ctypes.cast(jobs, ctypes.c_void_p), 1, h, w, _lib.dptr(ws), ws_bytes, _lib.stream_ptr())

    EINVAL, EWORKSPACE = -1, -3                                              # include/ape_hip.h
    assert run(job(rgb_ptr=0)) == EINVAL                                     # null frame
    assert run(job(), out_ptr=ctypes.c_void_p(out.data_ptr() + 8)) == EINVAL  # misaligned output
    assert run(job(off=8), out_bytes=nbytes + 16) == EINVAL                  # misaligned sample offset
    assert run(job(), ws_ptr=ctypes.c_void_p(ws.data_ptr() + 4)) == EINVAL   # misaligned workspace
    assert run(job(), ws_bytes=need - 1) == EWORKSPACE                       # workspace too small
    assert run(job(), out_bytes=nbytes - 1) == EINVAL                        # the sample does not fit the block
    assert run(job(off=16), out_bytes=nbytes + 15) == EINVAL
    for box in ((0, 0, 0, 80), (0, 40, 0, 0), (0, 20, 0, 80), (0, 40, 0, 60), (0, 41, 0, 80), (-40, 40, 0, 80), (0, 40, 600, 680),
                (440, 520, 0, 80), (40, 0, 0, 80)):
        assert run(job(box=box)) == EINVAL, box                              # outside 40..480 x 40..640, no multiple of 40, outside the frame
    assert stats(job(rgb_ptr=0), need) == EINVAL
    assert stats(job(), L.ape_pose_train_tables_offset(1, h) - 1) == EWORKSPACE
    bad = job()
    bad.jit.n_ops, bad.jit.code[0] = 1, 9
    assert stats(bad, need) == EINVAL and run(bad) == EINVAL
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7 and int(ws.min()) == 9 and int(ws.max()) == 9            # nothing ran
    with pytest.raises(_lib.ApeError):
        A.build_samples([(rgb.cpu(), depth.cpu(), label.cpu())], [{}], [(R.INTR, R.DEPTH_SCALE)], n, True, False, [0.5] * 3, [0.2] * 3, None)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_train_driver(tmp_path):
    """3 = nepoch: epochs 1 and 2; refine_margin = 1e9 starts the refiner phase after epoch 1"""
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet
    from autoposeestimation_amd.DenseFusion.tools.train import main
    root = str(tmp_path)
    S.pose_dataset_tree(root)
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    logs = main("synth", root, load_pretrained=False, nepoch=3, batch_size=2, refine_margin=1e9, num_points=500)
    on_disk = json.load(open(os.path.join(root, "DenseFusion/experiments/logs/synth/losses.json")))
    assert set(on_disk) == {"losses", "refiner_losses", "train_dists", "test_dists"}
    for key, values in on_disk.items():
        assert values == logs[key] and len(values) == 2 and all(np.isfinite(v) for v in values), key
    assert on_disk["refiner_losses"][0] == 0 and on_disk["refiner_losses"][1] > 0                   # the refiner phase ran in epoch 2
    assert logs["batch_size"] == 1                                                                  # int(2 / 2)
    out = os.path.join(root, "DenseFusion/trained_models/synth")
    est, ref = PoseNet(500, 2), PoseRefineNet(500, 2)
    sd = torch.load(os.path.join(out, "pose_model.pth"), map_location="cpu")
    assert set(sd) == set(est.state_dict())
    est.load_state_dict(sd)
    sd = torch.load(os.path.join(out, "pose_refine_model.pth"), map_location="cpu")
    assert set(sd) == set(ref.state_dict())
    ref.load_state_dict(sd)

"""The segmentor's training-sample builder (csrc/seg_train.hip), SegmentationDataset.batch and segmentation_training on the GPU, against
the package's host Pillow path (segmentation/utils.py's transforms, pinned to the reference by tests/test_seg_train_samples_host.py) and
against tests/golden/seg_train.npz (made by running the reference).  Every comparison of samples is exact: np.array_equal on the fp32
image and on the labels, no pixel excused."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

import seg_train_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = R.golden()
NAMES = [str(n) for n in G["names"]]
OPS = [("brightness", 1.13), ("contrast", 0.87), ("saturation", 1.08), ("hue", -0.031)]


def _build(samples, params, class_ids, crop):
    from autoposeestimation_amd.segmentation import augment as A
    dev = [(torch.from_numpy(np.ascontiguousarray(r)).to(DEV), torch.from_numpy(np.ascontiguousarray(l)).to(DEV)) for r, l in samples]
    img, lab, boxes = A.build_samples(dev, params, class_ids, R.MEAN, R.STD, crop)
    assert img.dtype == torch.float32 and lab.dtype == torch.int64
    return img.cpu().numpy(), lab.cpu().numpy(), boxes


def _compare(samples, params, class_ids, crop, what):
    """builder against the host Pillow path with the same parameters, the boxes the builder drew included"""
    img, lab, boxes = _build(samples, params, class_ids, crop)
    s = crop.output_size
    assert img.shape == (len(samples), 3, s, s) and lab.shape == (len(samples), s, s)
    for i, ((rgb, label), p, cid) in enumerate(zip(samples, params, class_ids)):
        wi, wl = R.pillow_sample(rgb, label, dict(p, box=boxes[i]), crop, cid)
        print("%s sample %d: box %r side %d, %d fp32 values and %d labels differ" % (what, i, boxes[i], boxes[i][2] - boxes[i][0],
                                                                                   int((img[i] != wi).sum()), int((lab[i] != wl).sum())))
        assert np.array_equal(img[i], wi) and np.array_equal(lab[i], wl)
    return img, lab, boxes


def _mixed(h, w, s, seed):
    """5 samples: no rotation / 180 / arbitrary angles, jitter with and without contrast and none, every crop branch (square object,
    tall, wide: the slide draws np.random.randint), a box past the frame (Image.crop's zero fill) and a crop of the output's own size"""
    from autoposeestimation_amd.segmentation.utils import CropAndZoom
    rng = np.random.default_rng(seed)
    crop = CropAndZoom(output_size=s)
    shapes = ["ellipse", "tall", "wide", "ellipse", "ellipse"]
    samples = [R.synthetic_sample(rng, h, w, sh) for sh in shapes]
    random.seed(seed)
    np.random.seed(seed)
    params = [{"ops": OPS, "angle": None, "zoom": crop.draw_zoom()},
              {"ops": [o for o in OPS if o[0] != "contrast"], "angle": 180.0, "zoom": crop.draw_zoom()},
              {"ops": OPS[::-1], "angle": 33.3, "zoom": crop.draw_zoom()},
              {"ops": [], "angle": -120.5, "box": (-5, -3, s - 9, s - 7)},
              {"ops": [OPS[1]], "angle": 7.25, "box": (w - s, 0, w, s)}]
    return samples, params, [1, 2, 3, 4, 5], crop


@pytest.mark.parametrize("h,w,s", [(48, 64, 48), (40, 56, 40)])
def test_builder_equals_pillow_mixed_batch(h, w, s):
    samples, params, cids, crop = _mixed(h, w, s, 21)
    img, lab, boxes = _compare(samples, params, cids, crop, "%dx%d" % (h, w))
    assert {int(v) for v in np.unique(lab)} <= set([0] + cids) and all(int((lab[i] == cids[i]).sum()) > 0 for i in range(3))
    # the same batch again is bit-identical, and a sample does not depend on its batch
    img2, lab2, _ = _build(samples, [dict(p, box=b) for p, b in zip(params, boxes)], cids, crop)
    assert np.array_equal(img, img2) and np.array_equal(lab, lab2)
    img3, lab3, _ = _build(samples[2:3], [dict(params[2], box=boxes[2])], cids[2:3], crop)
    assert np.array_equal(img3[0], img[2]) and np.array_equal(lab3[0], lab[2])


def test_more_samples_than_one_launch_takes():
    """the job table travels 16 samples per launch: 17 samples cross the chunk boundary"""
    from autoposeestimation_amd.segmentation.utils import CropAndZoom, colorJitter, rotate
    rng = np.random.default_rng(4)
    crop = CropAndZoom(output_size=40)
    samples = [R.synthetic_sample(rng, 40, 56, ["ellipse", "tall", "wide"][i % 3]) for i in range(17)]
    random.seed(4)
    np.random.seed(4)
    params = [{"ops": colorJitter().params(), "angle": rotate().params(), "zoom": crop.draw_zoom()} for _ in range(17)]
    _compare(samples, params, [1 + i % 3 for i in range(17)], crop, "17 samples")


def test_one_real_size_sample():
    """480 x 640 -> 480 x 480: the fixed-point ranges of the affine walk and of the filter sums at the size the reference trains at"""
    from autoposeestimation_amd.segmentation.utils import CropAndZoom
    rng = np.random.default_rng(9)
    crop = CropAndZoom()
    sample = R.synthetic_sample(rng, 480, 640)
    random.seed(9)
    np.random.seed(9)
    _, _, boxes = _compare([sample], [{"ops": OPS, "angle": 33.3, "zoom": crop.draw_zoom()}], [7], crop, "480x640")
    assert 240 <= boxes[0][2] - boxes[0][0] < 480


@pytest.mark.parametrize("name", NAMES)
def test_golden_case_through_the_device_path(name):
    """the reference's own CropAndZoom outputs: box drawn from the extents the first launch finds, crop and both resizes on the device"""
    label, seed = G["%s_label" % name], int(G["%s_seed" % name])
    cz = R.crop_and_zoom(G, name)
    random.seed(seed)
    np.random.seed(seed)
    img, lab, boxes = _build([(G["rgb"], label)], [{"ops": [], "angle": None, "zoom": cz.draw_zoom()}], [3], cz)
    assert list(boxes[0]) == [int(v) for v in G["%s_box" % name]]
    assert np.array_equal(img[0], R.normalise(G["%s_img_out" % name]))
    assert np.array_equal(lab[0], np.where(G["%s_label_out" % name] != 0, 3, 0))


def test_golden_rotation_through_the_device_path():
    """the reference's rotate result, looked at through a crop of the whole height at scale 1 (48 -> 48 is the identity in Pillow)"""
    from autoposeestimation_amd.segmentation.utils import CropAndZoom
    cz = CropAndZoom(output_size=48)
    for left in (0, 16):
        img, lab, _ = _build([(G["rgb"], G["rotate_label"])], [{"ops": [], "angle": float(G["rotate_angle"]), "box": (left, 0, left + 48, 48)}],
                             [1], cz)
        assert np.array_equal(img[0], R.normalise(G["rotate_img_out"][:, left:left + 48]))
        assert np.array_equal(lab[0], (G["rotate_label_out"][:, left:left + 48] != 0).astype(np.int64))


def test_argument_checks_return_errors_without_launching():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd.segmentation import augment as A
    L = _lib.lib()
    h, w, s = 40, 56, 40
    rgb = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    label = torch.zeros(h, w, dtype=torch.uint8, device=DEV)
    need = L.ape_seg_train_workspace_bytes(1, s)
    assert need == L.ape_seg_train_tables_offset(1) + 14 * s * 4 and L.ape_seg_train_extents_offset(1) == 64 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    img = torch.full((3 * s * s + 4,), 7.0, dtype=torch.float32, device=DEV)
    lab = torch.full((s * s,), 7, dtype=torch.int64, device=DEV)
    m, sd = (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)

    def run(job, img_ptr=None, ws_bytes=need, out=s):
        jobs = (_lib.SegTrainJob * 1)(job)
        return L.ape_seg_train_samples(ctypes.cast(jobs, ctypes.c_void_p), 1, h, w, out, ctypes.cast(m, ctypes.c_void_p),
                                       ctypes.cast(sd, ctypes.c_void_p), img_ptr or _lib.dptr(img), _lib.dptr(lab), _lib.dptr(ws), ws_bytes,
                                       _lib.stream_ptr())

    def job(side=20, rgb_ptr=rgb.data_ptr()):
        j = A.make_job({}, h, w, rgb_ptr, label.data_ptr(), 1)
        j.crop_x, j.crop_y, j.crop_side = 0, 0, side
        return j

    EINVAL, EWORKSPACE = -1, -3                                              # include/ape_hip.h
    assert run(job(side=s + 1)) == EINVAL                                    # crop larger than the output: enlargement only
    assert run(job(), img_ptr=ctypes.c_void_p(img.data_ptr() + 4)) == EINVAL  # misaligned output
    assert run(job(rgb_ptr=0)) == EINVAL                                     # null frame
    assert run(job(), ws_bytes=need - 1) == EWORKSPACE                       # workspace too small
    jobs = (_lib.SegTrainJob * 1)(job())
    assert L.ape_seg_train_stats(ctypes.cast(jobs, ctypes.c_void_p), 1, h, w, _lib.dptr(ws), L.ape_seg_train_tables_offset(1) - 1,
                                 _lib.stream_ptr()) == EWORKSPACE
    torch.cuda.synchronize()
    assert float(img.min()) == 7.0 and float(img.max()) == 7.0 and int(lab.min()) == 7 and int(lab.max()) == 7      # nothing ran
    with pytest.raises(ValueError, match="enlargement"):
        A.set_crop(job(), (0, 0, s + 2, s + 2), s)
    with pytest.raises(_lib.ApeError):
        A.build_samples([(rgb.cpu(), label.cpu())], [{}], [1], R.MEAN, R.STD, None)


def test_empty_label_raises_with_the_sample_name(tmp_path):
    from autoposeestimation_amd.segmentation.dataset import SegmentationDataset
    from autoposeestimation_amd.segmentation.utils import CropAndZoom
    rng = np.random.default_rng(3)
    rgb, label = R.synthetic_sample(rng, 40, 56)
    R.write_tree(str(tmp_path), "one", [("bluedude/000007", rgb, np.where(label == 255, 254, 0).astype(np.uint8))], [], ["bluedude"])
    ds = SegmentationDataset("one", "train", mean=R.MEAN, std=R.STD, root=str(tmp_path), crop=CropAndZoom(output_size=40))
    with pytest.raises(ValueError, match="bluedude/000007"):
        ds.batch([0])


def test_dataset_batch_equals_its_host_path(tmp_path):
    """SegmentationDataset.batch (device) and sample_host (Pillow) from the same seeds, in both modes"""
    from autoposeestimation_amd.segmentation.dataset import SegmentationDataset
    from autoposeestimation_amd.segmentation.utils import CropAndZoom
    rng = np.random.default_rng(6)
    items = [("%s/%06d" % (c, i), ) + R.synthetic_sample(rng, 40, 56, sh) for i, (c, sh) in
             enumerate([("bluedude", "ellipse"), ("greendude", "tall"), ("bluedude", "wide")])]
    R.write_tree(str(tmp_path), "two", items, items[:2], ["bluedude", "greendude"])
    ds = SegmentationDataset("two", "train", mean=R.MEAN, std=R.STD, root=str(tmp_path), crop=CropAndZoom(output_size=40))
    random.seed(8)
    np.random.seed(8)
    img, lab, params = ds.batch([2, 0, 1], return_params=True)
    for k, i in enumerate([2, 0, 1]):
        wi, wl = ds.sample_host(i, params[k])
        assert torch.equal(img[k].cpu(), wi) and torch.equal(lab[k].cpu(), wl)
    assert sorted(int(v) for v in torch.unique(lab[2])) == [0, 2]
    test = SegmentationDataset("two", "test", mean=R.MEAN, std=R.STD, root=str(tmp_path))
    img, lab = test.batch([0, 1])
    assert tuple(img.shape) == (2, 3, 40, 56) and tuple(lab.shape) == (2, 40, 56) and lab.dtype == torch.int64
    for i in range(2):
        wi, wl = test[i]
        assert torch.equal(img[i].cpu(), wi) and torch.equal(lab[i].cpu(), wl)


def test_segmentation_training_driver(tmp_path):
    """2 epochs over a tree of 6 frames of 64 x 96 with 2 classes: the log, the checkpoint's keys, and get_default_model loads it"""
    from autoposeestimation_amd.label_generator.create_labels import get_default_model
    from autoposeestimation_amd.segmentation import segmentation_training
    from autoposeestimation_amd.segmentation.utils import CropAndZoom
    rng = np.random.default_rng(12)
    items = [("%s/%06d" % (["bluedude", "greendude"][i % 2], i),) + R.synthetic_sample(rng, 64, 96) for i in range(6)]
    root = str(tmp_path)
    R.write_tree(root, "tiny", items[:4], items[4:], ["bluedude", "greendude"])
    training_config = {"epochs": 2, "batch_size": 2, "lr": 1e-3, "weight_decay": 0.1, "shuffle": True, "num_workers": 0, "momentum": 0.9,
                       "dataset_name": "tiny"}
    segmentation_config = {"name": "Unet", "encoder_name": "resnet18", "encoder_weights": None, "activation": "softmax"}
    random.seed(1)
    np.random.seed(1)
    torch.manual_seed(1)
    logs = segmentation_training(training_config, segmentation_config, root=root, crop=CropAndZoom(output_size=64))
    assert segmentation_config["name"] == "Unet"                      # the caller's dict is left alone
    on_disk = json.load(open(os.path.join(root, "segmentation", "logs", "tiny", "Unet_resnet18.json")))
    assert on_disk == logs
    for key in ("train_iou_scores", "train_losses", "valid_iou_scores", "valid_losses"):
        assert len(logs[key]) == 2 and all(np.isfinite(v) for v in logs[key]), key
    assert logs["best_iou_score"] == max(logs["valid_iou_scores"]) and logs["best_iou_score_epoch"] in (0, 1)
    cp = torch.load(os.path.join(root, "segmentation", "trained_models", "tiny", "Unet_resnet18.ckpt"), map_location="cpu")
    assert set(cp) == {"state_dict", "epoch", "iou", "train_iou_scores", "train_losses", "train_loss", "valid_iou_scores", "valid_losses",
                       "training_config", "name", "segmentation_config"}
    assert cp["name"] == "Unet" and cp["segmentation_config"]["classes"] == 3 and cp["training_config"]["dataset_name"] == "tiny"
    model = get_default_model(root, "tiny", 3, name="Unet", encoder_name="resnet18")
    assert set(model.state_dict()) == set(cp["state_dict"])

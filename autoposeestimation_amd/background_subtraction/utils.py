"""Drop-in for the labelling half of background_subtraction/utils.py: `get_default_model` (:648-663),
`do_cca` (:199-222) and `get_mask_prediction` (:666-873) -- the step that writes the `.pred.label.png` files the pose-label
generator consumes (label_generator/create_labels.py:167-168).

Per frame the reference decodes six PNGs, builds a 7-channel difference image in numpy, runs its segmentor on ONE frame,
copies the probabilities to the host and loops over components in Python.  Here a batch of frame pairs is uploaded once;
`ape_bgsub_features_f32` builds the normalised 7-channel NHWC tensor on the device, the segmentor runs on the batch, the
fused head emits arg-max + max-probability and `ape_seg_components_scored(APE_SEG_SCORE_SUM)` keeps the component with the
largest summed probability.  Only the final uint8 labels come back for PNG encoding.

Network: the reference hard-codes smp's Unet-resnet34 with in_channels = 7 (third-party, unavailable: segmentation/utils.py)
-> the default here is the in-repo PSPNet ('PsPNet', resnet34 encoder, 7 input channels, 2 classes), checkpoint
`<root>/background_subtraction/trained_models/<name>_<encoder>.ckpt` holding {'state_dict': ...} like the reference's.

Training side (reference :63-384, :414-646): `load_subtraction` and `augment` build ONE sample through the device batch builder
(background_subtraction/augment.py, csrc/bgsub_train.hip); `IoU_cca` is the metric behind `do_cca`, entirely on the device;
`jaccard_loss`, `Metric`, `ConfusionMatrix`, `IoU` and `get_model` are the segmentation package's (segmentation/metrics.py,
segmentation/utils.py).  The reference keeps a second copy of them in this module; checked against :63-384: `Metric`,
`ConfusionMatrix`, `IoU` and `get_model` are the same functions, and both modules' `IoU.value()` and `IoU_cca.value()` average `iou[1:]`.
`jaccard_loss` is NOT the same: this module's (:63-99) ends in `jacc_loss[1:].mean()` -- every class but the first, so with two classes
only the object's IoU term -- where segmentation/utils.py:110-111 averages `jacc_loss[unique(true)]`, the classes present in the batch,
background included.  The name exported here is the segmentation package's device kernel (`ape_jaccard_fwd_f32`), so the driver of this
build minimises `1 - mean(J_background, J_object)` where the reference minimises `1 - J_object`; a `[1:]` variant of the kernel is not
built yet and the logged losses are therefore not comparable with the reference's.  The torchvision
wrapper classes (HFlipDefault, colorJitter, normalize, toTensor, :16-58) are unused by the reference's own driver and not provided;
`animate` is a matplotlib view and not provided."""
import json
import os
import random

import numpy as np
import torch
from PIL import Image

from autoposeestimation_amd import engine as E
from autoposeestimation_amd.background_subtraction import augment as G
from autoposeestimation_amd.background_subtraction.augment import ColorJitterPIL  # noqa: F401
from autoposeestimation_amd.data_generation import sample_io
from autoposeestimation_amd.segmentation.metrics import ConfusionMatrix, IoU, Metric, jaccard_loss  # noqa: F401
from autoposeestimation_amd.segmentation.utils import get_model

DEFAULT_MEAN = [0.040278014, 0.04060352, 0.038310923, 0.0381776, 0.03656849, 0.03636289, 0.03556486]      # :670-673
DEFAULT_STD = [0.059689723, 0.05965291, 0.056203008, 0.05619316, 0.054657422, 0.054514673, 0.05377024]


def get_default_model(root, name="PsPNet", encoder_name="resnet34", load=True):
    """reference :648-663"""
    segmentation_config = {"encoder_name": encoder_name,
                           "encoder_weights": None,
                           "activation": "softmax",
                           "in_channels": 7,
                           "classes": 2}
    model = get_model(name, segmentation_config)
    if load:
        cp = torch.load(os.path.join(root, "background_subtraction", "trained_models",
                                     "{}_{}.ckpt".format(name, segmentation_config["encoder_name"])),
                        map_location=torch.device("cpu"))
        model.load_state_dict(cp["state_dict"])
    return model


def _biggest_component(label, score):
    """label[B,H,W] u8 (arg-max), score[B,H,W] f32 (max probability) -> u8 {0,1}: do_cca's component choice (:208-219);
    cv2.connectedComponents treats every non-zero label as foreground."""
    fg = (label != 0).to(torch.uint8)
    objmap, _ = E.seg_components(fg, score, 2, min_pixels=0, score_mode=E.SEG_SCORE_SUM)
    return objmap


def do_cca(predicted, cuda=True):
    """reference :199-222.  predicted[B,C,H,W] device tensor (the model's `predict` output) -> ndarray [B,H,W] f64 in {0,1}"""
    if not predicted.is_cuda:
        raise RuntimeError("do_cca runs on the GPU only (no CPU fallback in this build)")
    b, c, h, w = predicted.shape
    nhwc = predicted.permute(0, 2, 3, 1).contiguous().float()
    label, score = E.seg_argmax(nhwc, c, double_softmax=False)          # F.softmax(predicted, dim=1) (:200) + argmax / max
    return _biggest_component(label.view(b, h, w), score.view(b, h, w)).cpu().numpy().astype(np.float64)


def depth_gate(meta, reference_point):
    """(min, max) of the accepted depth range in sensor units (:733-752)"""
    rp = np.asarray(reference_point, dtype=np.float64).reshape(-1)
    measure_dist = None
    if rp.size:
        measure_dist = np.linalg.norm(rp - sample_io.robot2cam(meta)[:3, 3])
    if not measure_dist:
        return 0.0, float(int(1500))
    return measure_dist - 150, measure_dist + 150


def subtract_frames(model, f_rgb, b_rgb, f_depth, b_depth, gate, mean=None, std=None):
    """Device form of the per-frame block (:721-833) for a batch of (object frame, empty-scene frame) pairs.
    f_rgb/b_rgb[B,H,W,3] u8, f_depth/b_depth[B,H,W] u16, gate[B,2] f64 (cuda) -> labels[B,H,W] u8 {0,255} (cuda)"""
    x8 = E.bgsub_features(f_rgb, b_rgb, f_depth, b_depth, gate, DEFAULT_MEAN if mean is None else mean,
                          DEFAULT_STD if std is None else std)
    if hasattr(model, "label_score_nhwc"):
        label, score = model.label_score_nhwc(x8, double_softmax=True)      # predict's softmax, then do_cca's (:200)
    else:
        label, score = E.seg_argmax(model.logits_nhwc(x8), model.classes, double_softmax=True)
    b, h, w = f_depth.shape
    return _biggest_component(label.view(b, h, w), score.view(b, h, w)) * 255


def get_mask_prediction(object_name, root, mean=None, std=None, reference_point=np.array([]), plot=False, use_cuda=True,
                        model=None, batch=16):
    """reference :666-873: for every non-background directory of `data_generation/data/<object_name>` pair frame idx with
    background frame idx and write `label_generator/data/<object_name>/<dir>/<idx>.pred.label.png`.
    `model` (optional) replaces get_default_model(root); `batch` frame pairs are processed per device pass."""
    if plot:
        raise NotImplementedError("plot=True is a matplotlib debugging view of the reference; not provided")
    # `use_cuda` is accepted for signature compatibility (main.py:194 passes use_cuda=False to keep the reference's
    # single-frame Unet off a busy GPU); this build has no CPU path, so it always runs on the GPU and fails loudly without one
    if not torch.cuda.is_available():
        raise RuntimeError("get_mask_prediction runs on the GPU only (no CPU fallback in this build)")
    device = torch.device("cuda:0")
    object_path = os.path.join(root, "data_generation/data", object_name)
    dirs = os.listdir(object_path)
    background_path = os.path.join(object_path, "background")
    if "background" not in dirs:
        raise ValueError("background does not exist in object_path: {}".format(object_path))
    dirs.remove("background")
    if "extra" in dirs:
        dirs.remove("extra")
    if len(dirs) < 1:
        raise ValueError("no foreground")
    n = int(len(os.listdir(background_path)) / 3)
    if model is None:
        model = get_default_model(root)
    model.to(device)
    model.eval()
    ns, counter = n * len(dirs), 0
    for d in dirs:
        foreground_path = os.path.join(object_path, d)
        save_dir = os.path.join(root, "label_generator/data", object_name, d)
        os.makedirs(save_dir, exist_ok=True)
        for i0 in range(0, n, batch):
            ids = ["{:06d}".format(i) for i in range(i0, min(n, i0 + batch))]
            f_rgb = np.stack([sample_io.read_color(foreground_path, s) for s in ids])
            b_rgb = np.stack([sample_io.read_color(background_path, s) for s in ids])
            f_depth = np.stack([sample_io.read_depth(foreground_path, s) for s in ids])
            b_depth = np.stack([sample_io.read_depth(background_path, s) for s in ids])
            if np.asarray(reference_point).size:
                gates = [depth_gate(sample_io.read_meta(foreground_path, s), reference_point) for s in ids]
            else:
                gates = [depth_gate(None, reference_point)] * len(ids)
            up = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
            labels = subtract_frames(model, up(f_rgb), up(b_rgb), up(f_depth), up(b_depth),
                                     up(np.asarray(gates, dtype=np.float64)), mean, std).cpu().numpy()
            for s, lab in zip(ids, labels):
                sample_io.write_label(save_dir, s, "pred", lab)
            counter += len(ids)
            print("number = {}/{}".format(counter, ns))


class IoU_cca(IoU):
    """reference :225-301: IoU of the prediction AFTER `do_cca` -- softmax again, arg-max, 8-connected components of the non-zero labels,
    keep the one with the largest summed probability (component 1 when there is none) -- against the target.  `add` runs on the device
    (`ape_seg_argmax_f32`, `ape_seg_components_scored(APE_SEG_SCORE_SUM)`, `ape_confusion_add`) and does not synchronise; `value()` reads
    the confusion matrix once.  predicted[N,K,H,W] f32 scores, target[N,H,W] integer labels, both on the device (the reference's `do_cca`
    cannot take [N,H,W] predictions either, and its `target.view(-1)` rules out [N,K,H,W] targets)."""

    def add(self, predicted, target):
        if predicted.shape[0] != target.shape[0]:
            raise ValueError("number of targets and predicted outputs do not match")
        if predicted.dim() != 4:
            raise ValueError("IoU_cca takes (N, K, H, W) scores: do_cca needs the class probabilities")
        if target.dim() != 3:
            raise ValueError("IoU_cca takes (N, H, W) integer targets")
        if not (predicted.is_cuda and target.is_cuda):
            raise RuntimeError("IoU_cca runs on the GPU only (no CPU fallback in this build)")
        b, k, h, w = predicted.shape
        nhwc = predicted.permute(0, 2, 3, 1).contiguous().float()
        label, score = E.seg_argmax(nhwc, k, double_softmax=False)          # F.softmax(predicted, dim=1) (:200) + argmax / max
        self.conf_metric._add_device(_biggest_component(label.view(b, h, w), score.view(b, h, w)), target)


def _open(root, key, sub, name, idx):
    return Image.open(os.path.join(root, key, sub, name.format(idx)))


def read_sample(root, key, idx):
    """the five files of one training sample (:443-447, :457-461, :499-503, :513-517, :597-601) -> (f_rgb[H,W,3] u8, b_rgb, f_depth[H,W]
    u16, b_depth, label[H,W] u8); refuses what the device builder cannot take"""
    b_rgb = np.array(_open(root, key, "background", "img{:06d}.png", idx).convert("RGB"))
    f_rgb = np.array(_open(root, key, "foreground", "img{:06d}.png", idx).convert("RGB"))
    depths = []
    for sub in ("foreground", "background"):
        d = _open(root, key, sub, "depth{:06d}.png", idx)
        if d.mode != "I;16":
            raise TypeError("%s depth of %s/%d is a %r image; the builder takes 16-bit depth (Pillow mode I;16)" % (sub, key, idx, d.mode))
        depths.append(np.array(d))
    y = _open(root, key, "groundtruth", "img{:06d}.mask.0.png", idx)
    if len(y.getbands()) != 1:
        raise ValueError("label of %s/%d has %d bands %r; one band expected" % (key, idx, len(y.getbands()), y.getbands()))
    if y.mode not in ("L", "P", "1"):
        raise TypeError("label of %s/%d is a %r image; an 8-bit label expected" % (key, idx, y.mode))
    label = np.array(y).astype(np.uint8)
    if not (f_rgb.shape == b_rgb.shape and f_rgb.shape[:2] == depths[0].shape == depths[1].shape == label.shape):
        raise ValueError("the five frames of %s/%d differ in size" % (key, idx))
    return f_rgb, b_rgb, depths[0], depths[1], label


def _flag_params(angle, resize, rotate, colorJitter, hflip, vflip, size):
    if resize is not None and resize is not False:
        want = tuple(getattr(resize, "size", ()))
        if want != tuple(size):
            raise ValueError("resize to %r of %r frames: only the identity is provided (the reference's Resize([480, 640]) of its 480 x 640 "
                             "frames; bilinear resizing of other sizes is not restated)" % (want, tuple(size)))
    if colorJitter is not None and colorJitter is not False and not isinstance(colorJitter, ColorJitterPIL):
        raise TypeError("colorJitter must be a ColorJitterPIL (the draws are made on the host, the jitter runs on the device)")
    return {"angle": angle if rotate else None, "hflip": bool(hflip), "vflip": bool(vflip)}


def load_subtraction(root, key, idx, resize=None, rotate=None, colorJitter=None, hflip=None, vflip=None, plot=False, abs=True):
    """reference :414-626 for one sample, through the batch builder with a batch of one: -> x[H,W,7] uint8 difference channels,
    y[H,W] float64.  Draws as the reference: `random.uniform(-180, 180)` when `rotate`, `np.random.rand()` per requested flip (dropped
    when <= 0.5), then the jitter of the background, then of the foreground.  `rotate` / `hflip` / `vflip` are used as flags, `resize`
    must carry `.size` equal to the frames', `colorJitter` is a ColorJitterPIL.  One difference: y is the BINARISED label (0. / 1.), not
    the rotated raw values -- dataset.py:76, the reference's only consumer, binarises at once."""
    if plot:
        raise NotImplementedError("plot=True is a matplotlib debugging view of the reference; not provided")
    if not abs:
        raise NotImplementedError("abs=False (signed differences cast to uint8) is not provided; the reference's dataset never asks for it")
    if not torch.cuda.is_available():
        raise RuntimeError("load_subtraction runs on the GPU only (no CPU fallback in this build)")
    p = G.draw_params(rotate=rotate, hflip=hflip, vflip=vflip, jitter=None)
    frames = read_sample(root, key, idx)
    _flag_params(p["angle"], resize, rotate, colorJitter, hflip, vflip, frames[4].shape)
    if colorJitter:
        p["ops_b"] = colorJitter.params()
        p["ops_f"] = colorJitter.params()
    dev = torch.device("cuda:0")
    _, lab, u8 = G.build_samples([tuple(torch.from_numpy(a).to(dev) for a in frames)], [p], DEFAULT_MEAN, DEFAULT_STD, want_u8=True)
    return u8[0].cpu().numpy(), lab[0].cpu().numpy().astype(np.float64)


def augment(x, angle=0, resize=None, rotate=None, colorJitter=None, hflip=None, vflip=None):
    """reference :629-646 on ONE image given as a device tensor: [H,W,3] u8 (RGB: rotate -> jitter -> flips) or
    [H,W] u8 (label): geometry only, returned binarised (0 / 1).  Same flag conventions as load_subtraction; the jitter draws its parameters when called.  The image
    goes through the sample builder beside blank companions and is read back from its difference against them."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError("augment takes a device tensor (no CPU fallback in this build)")
    h, w = x.shape[:2]
    p = _flag_params(angle, resize, rotate, colorJitter, hflip, vflip, (h, w))
    p["ops_f"] = colorJitter.params() if colorJitter else []
    z = lambda dt, *sh: torch.zeros(*sh, dtype=dt, device=x.device)  # noqa: E731
    if x.dtype == torch.uint8 and x.dim() == 3 and x.shape[2] == 3:
        frames = (x.contiguous(), z(torch.uint8, h, w, 3), z(torch.uint16, h, w), z(torch.uint16, h, w), z(torch.uint8, h, w))
        _, _, u8 = G.build_samples([frames], [p], [0.0] * 7, [1.0] * 7, want_u8=True)
        return u8[0, :, :, :3].contiguous()                 # |f - 0|
    if x.dtype == torch.uint8 and x.dim() == 2:
        frames = (z(torch.uint8, h, w, 3), z(torch.uint8, h, w, 3), z(torch.uint16, h, w), z(torch.uint16, h, w), x.contiguous())
        p["ops_f"] = []
        _, lab = G.build_samples([frames], [p], [0.0] * 7, [1.0] * 7)
        return lab[0].to(torch.uint8)                       # binarised, as the builder emits labels
    raise TypeError("augment takes [H,W,3] uint8 or [H,W] uint8 images, got %s %s (depth frames are augmented inside load_subtraction: their "
                    "difference, not the frame, leaves the builder)" % (x.dtype, tuple(x.shape)))

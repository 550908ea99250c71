"""Drop-in for the inference surface of segmentation/utils.py (reference :352-359): `nets`, `get_model`.

The reference builds its segmentor from the third-party `segmentation_models_pytorch==0.1.3` (smp.Unet / PSPNet /
Linknet), which is neither vendored in the reference tree nor installed here, so its arithmetic cannot be restated or
pinned.  DECISION: `get_model('PsPNet', cfg)` returns the reference's OWN in-repo PSPNet
(DenseFusion/lib/pspnet.py, BasicBlock encoder `cfg['encoder_name']` in {resnet18, resnet34}) executed by the gfx950
kernels; `predict()` returns the first `classes` channels of its `final` 1x1 conv with the configured activation.
`get_model('Unet', cfg)` returns segmentation/unet.py's UnetSegmentor, a restatement of smp 0.1.3's Unet (resnet18 / resnet34
encoder) with smp's state-dict keys, so the reference's `Unet_resnet34.ckpt` files load; LinkNet raises NotImplementedError.

The training loss and metric (jaccard_loss, Metric, ConfusionMatrix, IoU) live in segmentation/metrics.py and are re-exported here under
the reference's names; in train mode both segmentors' forward() builds a training graph on the tape (segmentation/train.py drives them).

The reference's transforms (:12-66, CropAndZoom :361-487) are at the end of this file under their names: callable on `[PIL image, PIL
label]` through Pillow -- the host path -- and each with a `params(...)` that draws from the reference's generators in the reference's
order and returns plain numbers, which the device builder (segmentation/augment.py, csrc/seg_train.hip) takes instead.  animate* stay
outside the package.
"""
import random

import numpy as np
import torch
from PIL import Image

from autoposeestimation_amd import engine as E
from autoposeestimation_amd.DenseFusion.lib.network import PSPNet, _need_cuda, _pspnet_train
from autoposeestimation_amd.segmentation.metrics import ConfusionMatrix, IoU, Metric, jaccard_loss  # noqa: F401


class PsPNetSegmentor(PSPNet):
    """`model.predict(x[B,in_channels,H,W]) -> [B,classes,H,W]` like smp's SegmentationModel.predict (eval + no_grad + activation)."""

    def __init__(self, encoder_name="resnet18", encoder_weights=None, activation="softmax", in_channels=3, classes=2):
        if not 1 <= in_channels <= 8:
            raise NotImplementedError("in_channels must be in 1..8")
        if encoder_weights is not None:
            raise NotImplementedError("no pretrained encoder weights are available offline")
        if not 1 <= classes <= 32:
            raise ValueError("classes must be in 1..32 (the in-repo PSPNet's final conv has 32 channels, pspnet.py:54)")
        if activation not in (None, "softmax", "softmax2d", "identity"):
            raise NotImplementedError("activation %r" % (activation,))
        super().__init__(backend=encoder_name, in_channels=in_channels)
        self.classes, self.activation = classes, activation
        self._final_cls = None

    def _build_plan(self, sd, dev):
        pl = super()._build_plan(sd, dev)
        # only the first `classes` rows of the final 1x1 conv are ever needed
        self._final_cls = E.Conv(sd["final.0.weight"][:self.classes], sd["final.0.bias"][:self.classes], device=dev,
                                 precision=self.precision)
        self._head_w = sd["final.0.weight"][:self.classes].detach().to(dev, torch.float32).reshape(self.classes, 64).contiguous()
        self._head_b = sd["final.0.bias"][:self.classes].detach().to(dev, torch.float32).contiguous()
        return pl

    def logits_nhwc(self, x4):
        """x4[B,H,W,4] (ToTensor+Normalize'd RGB, zero 4th channel; [B,H,W,8] for in_channels > 4) -> logits[B,H,W,classes]"""
        pl = self.plan()
        return self._final_cls(pl.features(x4))

    def label_score_nhwc(self, x4, double_softmax=True):
        """x4[B,H,W,4] -> (label u8[B,H,W], score f32[B,H,W]): features -> fused head (final conv rows 0..classes-1 in exact
        fp32 + softmax(+softmax) + argmax); the logits tensor of `logits_nhwc` is never materialised."""
        pl = self.plan()
        b, h, w, _ = x4.shape
        # the kernels index a tensor with 32 bits: the largest of the pass is the full-resolution 64-channel map up_3 reads / the head
        # consumes (B x H x W x 64 elements; 109 frames of 480x640).  Larger batches go through in slices.
        max_b = max(1, ((1 << 31) - 1) // (h * w * 64))
        if b > max_b:
            parts = [self.label_score_nhwc(x4[i:i + max_b], double_softmax) for i in range(0, b, max_b)]
            return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        if self.classes > 16:
            return E.seg_argmax(self.logits_nhwc(x4), self.classes, double_softmax)
        return pl.label_score(x4, self._head_w, self._head_b, double_softmax)

    def predict(self, x):
        _need_cuda(x, "input")
        if x.shape[1] != self.in_channels:
            raise ValueError("expected %d input channels, got %d" % (self.in_channels, x.shape[1]))
        x4 = torch.zeros(x.shape[0], x.shape[2], x.shape[3], (self.in_channels + 3) // 4 * 4, dtype=torch.float32, device=x.device)
        x4[..., :self.in_channels] = x.permute(0, 2, 3, 1)
        logits = self.logits_nhwc(x4).permute(0, 3, 1, 2).contiguous()
        if self.activation in ("softmax", "softmax2d"):
            return torch.softmax(logits, dim=1)
        return logits

    def forward(self, x):
        """train mode: x[B,in_channels,H,W] -> [B,classes,H,W] (a view of the NHWC result) through the PSPNet training graph (dropout
        masks included, set_dropout_masks) up to the `final` conv, its first `classes` channels, then the activation -- the head predict()
        uses.  eval mode: PSPNet.forward (unchanged)."""
        if not self.training:
            return super().forward(x)
        from autoposeestimation_amd import autograd as A
        _need_cuda(x, "input")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError("expected [B,%d,H,W], got %s" % (self.in_channels, tuple(x.shape)))
        b, _, h, w = x.shape
        if b * h * w * 64 >= 1 << 31:
            raise ValueError("batch %s is too large for one training step: B*H*W*64 must stay below 2^31" % (tuple(x.shape),))
        self.sync_banks()
        x4 = torch.zeros(b, h, w, (self.in_channels + 3) // 4 * 4, dtype=torch.float32, device=x.device)
        x4[..., :self.in_channels] = x.detach().permute(0, 2, 3, 1)
        y = _pspnet_train(self, "", self.backend, x4, self._drop, self.precision, logits_only=True)[..., :self.classes]
        if self.activation in ("softmax", "softmax2d"):
            y = A.SoftmaxChannelsFn.apply(y)
        return y.permute(0, 3, 1, 2)


def _unavailable(name):
    def ctor(**cfg):
        raise NotImplementedError(
            "%s comes from segmentation_models_pytorch, which is not vendored in the reference and not installed; "
            "use get_model('PsPNet', cfg) (in-repo PSPNet on gfx950)" % name)
    return ctor


def _unet(**cfg):
    from autoposeestimation_amd.segmentation.unet import UnetSegmentor
    return UnetSegmentor(**cfg)


nets = {"Unet": _unet, "PsPNet": PsPNetSegmentor, "LinkNet": _unavailable("smp.Linknet")}


def get_model(name, segmentation_config):
    """reference segmentation/utils.py:356-359"""
    model = nets[name]
    model = model(**segmentation_config)
    return model


# ---- the transforms of the training samples (reference :12-66, :361-487) -------------------------------------------------------------
from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import ColorJitterPIL  # noqa: E402


class HFlipDefault:
    def __init__(self):
        self.p = 0.5

    def params(self):
        return bool(np.random.rand() <= self.p)

    def __call__(self, data, flip=None):
        img, label = data
        if self.params() if flip is None else flip:
            img = img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
            label = label.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
        return [img, label]


class rotate:
    def __init__(self):
        self.range = [-180, 180]

    def params(self):
        return random.uniform(self.range[0], self.range[1])

    def __call__(self, data, angle=None):
        image, label = data
        if angle is None:
            angle = self.params()
        return image.rotate(angle), label.rotate(angle)          # transforms.functional.rotate's defaults: nearest, no expand, zero fill


class colorJitter:
    def __init__(self):
        self.ColorJitter = ColorJitterPIL(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.05)

    def params(self):
        return self.ColorJitter.params()

    def __call__(self, data, ops=None):
        img, label = data
        img = ColorJitterPIL.apply(img, self.params() if ops is None else ops)
        return [img, label]


class normalize:
    def __init__(self, mean, std):
        self.mean = torch.as_tensor([float(m) for m in mean], dtype=torch.float32).view(-1, 1, 1)
        self.std = torch.as_tensor([float(s) for s in std], dtype=torch.float32).view(-1, 1, 1)
        if (self.std == 0).any():
            raise ValueError("std evaluated to zero")

    def params(self):
        return [float(m) for m in self.mean.view(-1)], [float(s) for s in self.std.view(-1)]

    def __call__(self, data):
        img, label = data
        return [(img - self.mean) / self.std, label]


class toTensor:
    """ToTensor of the frame (HWC u8 -> CHW f32 / 255); the label becomes an i64 tensor of its values"""

    def params(self):
        return 255.0

    def __call__(self, data):
        img, label = data
        a = np.asarray(img, dtype=np.uint8)
        if a.ndim == 2:
            a = a[:, :, None]
        img = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1))).to(torch.float32).div(255)
        return [img, torch.from_numpy(np.asarray(label).astype(np.int64))]


def _square(centre, side):
    """rows and columns of the square of `side` around `centre`: the half side is truncated, so an odd side loses a pixel"""
    half = int(side / 2)
    return [centre[0] - half, centre[0] + half, centre[1] - half, centre[1] + half]


def _shift_inside(box, height, width):
    """slide the box back when it sticks out at the top / left, else at the bottom / right; a box larger than the frame still sticks out"""
    top, bottom, left, right = box
    dr = top if top < 0 else max(bottom - height, 0)
    dc = left if left < 0 else max(right - width, 0)
    return [top - dr, bottom - dr, left - dc, right - dc]


class CropAndZoom:
    """The label-driven random crop of reference :361-487, restated.  A square of a random side in [min_l, max_l) is centred on the
    object (the label's pixels == 255).  When the object's extent is not about square (height / width outside [0.8, 1.2]) the centre is
    first moved to a random place along the longer axis.  A square taller than the frame is replaced by one of height - 2; the square is
    then slid inside the frame, cropped and resized to output_size (Pillow's default BICUBIC for the image, NEAREST for the label).

    Three properties of the reference's arithmetic are kept because the boxes depend on them: the "taller than the frame" test and the
    height - 2 replacement use the frame's HEIGHT for the columns too; every half (of a side, of an extent) is truncated with int(); an
    about-square object is slid, along the columns, only on the too-tall route.  The reference also builds a box of 1.1 times the
    object first, but only its centre survives the zoom, and that is the object's, so it is not built here."""

    def __init__(self, output_size=480, max_zoom=2):
        self.output_size, self.max_zoom = output_size, max_zoom
        self.max_l = output_size
        self.min_l = int(float(output_size) / max_zoom)
        self.to_small, self.to_big = 0.8, 1.2

    def draw_zoom(self):
        """the side, before truncation: the one draw from `random`; it does not depend on the label"""
        return random.uniform(self.min_l, self.max_l)

    def box(self, extreme_points, size, zoom=None):
        """extreme_points = (first row, last row, first column, last column) of the object, size = (height, width) of the frame ->
        [top, bottom, left, right] as Python ints.  Draws the zoom unless it is given, then at most one `np.random.randint(0, n)` with
        n the object's extent along the axis it slides on."""
        height, width = int(size[0]), int(size[1])
        r0, r1, c0, c1 = [int(v) for v in extreme_points]
        extent = [r1 - r0, c1 - c0]
        centre = [r0 + int(extent[0] / 2), c0 + int(extent[1] / 2)]
        ratio = (float(extent[0]) / float(self.output_size)) / (float(extent[1]) / float(self.output_size))
        side = 2 * int(int(self.draw_zoom() if zoom is None else zoom) / 2)
        if self.to_small <= ratio <= self.to_big:
            axis = 1 if side > height else None
        else:
            axis = 1 if extent[1] > extent[0] else 0
        if axis is not None:
            centre[axis] = int(centre[axis] - extent[axis] / 2) + int(np.random.randint(0, extent[axis]))
        return _shift_inside(_square(centre, side if side <= height else height - 2), height, width)

    def params(self, extreme_points, size, zoom=None):
        """-> the box in Image.crop's order: (left, upper, right, lower)"""
        top, bottom, left, right = self.box(extreme_points, size, zoom)
        return (left, top, right, bottom)

    def get_extreme_points(self, label, name=None):
        rows, cols = np.where(np.asarray(label) == 255)
        if rows.size == 0:
            raise ValueError("the label of sample %s has no pixel equal to 255: CropAndZoom has no object to crop around" %
                             ("<unnamed>" if name is None else name))
        return [int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())]

    def __call__(self, data, box=None, name=None):
        image, label = data
        if box is None:
            lab = np.array(label)
            box = self.params(self.get_extreme_points(lab, name), lab.shape[:2])
        out = (self.output_size, self.output_size)
        return [image.crop(box=list(box)).resize(size=out), label.crop(box=list(box)).resize(size=out, resample=Image.NEAREST)]

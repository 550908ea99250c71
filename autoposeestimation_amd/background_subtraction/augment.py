"""Augmentation parameters of the background-subtraction training samples and their device builder.

The reference augments in Pillow on the host (background_subtraction/utils.py:414-646).  Here the host only DRAWS the parameters -- from the
reference's generators in the reference's order, `draw_params` -- and turns them into one `ape_bgsub_train_job` per sample (`make_job`);
`build_samples` hands a batch of jobs over raw frames that already live on the device to `ape_bgsub_train_samples` (csrc/bgsub_train.hip).

A parameter set is a dict: angle (None = no rotation step, else the float given to `Image.rotate`), hflip, vflip (bools: applied or not),
ops_f / ops_b (the ordered `(name, factor)` lists of `ColorJitterPIL.params` for the foreground / background image; [] = no jitter)."""
import ctypes
import math
import random

import numpy as np
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import ColorJitterPIL

ROT_NONE, ROT_180, ROT_AFFINE, ROT_90, ROT_270 = 0, 1, 2, 3, 4
_OP_CODES = {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4}
MAX_OPS = 4


def draw_params(rotate=None, hflip=None, vflip=None, jitter=None):
    """the draws of load_subtraction (:430-440) and of the two ColorJitter calls inside augment (:448, :474): `random.uniform` for the
    angle, `np.random.rand` per requested flip -- a requested flip is DROPPED when the draw is <= 0.5 --, then the jitter parameters of
    the background image, then those of the foreground image.  Arguments are truthy / falsy like the reference's callables; `jitter` is a
    ColorJitterPIL (its `params` draws from `random`)."""
    angle = random.uniform(-180, 180) if rotate else None
    if hflip and np.random.rand() <= 0.5:
        hflip = None
    if vflip and np.random.rand() <= 0.5:
        vflip = None
    ops_b = jitter.params() if jitter else []
    ops_f = jitter.params() if jitter else []
    return {"angle": angle, "hflip": bool(hflip), "vflip": bool(vflip), "ops_f": ops_f, "ops_b": ops_b}


def rotation(angle, h, w):
    """-> (rot_mode, a[6], fa[6]): what Pillow's `Image.rotate(angle)` (nearest, no expand, centre of the image, zero fill) does with an
    h x w image.  Multiples of 180 degrees (and of 90 for square images) are copies / transposes; everything else is the AFFINE transform
    with the matrix Image.rotate builds (rounded to 15 decimals there), walked in 16.16 fixed point for 8-bit images."""
    if angle is None:
        return ROT_NONE, [0.0] * 6, [0] * 6
    angle = angle % 360.0
    if angle == 0:
        return ROT_NONE, [0.0] * 6, [0] * 6
    if angle == 180:
        return ROT_180, [0.0] * 6, [0] * 6
    if angle in (90, 270) and w == h:
        return (ROT_90 if angle == 90 else ROT_270), [0.0] * 6, [0] * 6
    cx, cy = w / 2, h / 2
    rad = -math.radians(angle)
    a = [round(math.cos(rad), 15), round(math.sin(rad), 15), 0.0, round(-math.sin(rad), 15), round(math.cos(rad), 15), 0.0]
    a[2] = a[0] * -cx + a[1] * -cy + a[2]
    a[5] = a[3] * -cx + a[4] * -cy + a[5]
    a[2] += cx
    a[5] += cy
    if a[1] == 0 and a[3] == 0:
        raise ValueError("rotation by %r degrees rounds to a pure scaling in Pillow (its ImagingScaleAffine route), which the builder does "
                         "not restate" % angle)
    for x, y in ((0, 0), (w, h), (0, h), (w, 0)):       # Geometry.c check_fixed: else Pillow leaves the fixed-point walk
        if not (abs(x * a[0] + y * a[1] + a[2]) < 32768.0 and abs(x * a[3] + y * a[4] + a[5]) < 32768.0):
            raise ValueError("image too large for Pillow's fixed-point affine walk")
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))  # noqa: E731
    fa = [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]
    return ROT_AFFINE, a, fa


def make_job(params, h, w, f_rgb, b_rgb, f_depth, b_depth, label):
    """one `ape_bgsub_train_job`; the five frames are addresses (device pointers for the kernel)"""
    job = _lib.BgsubTrainJob()
    job.f_rgb, job.b_rgb, job.f_depth, job.b_depth, job.label = f_rgb, b_rgb, f_depth, b_depth, label
    mode, a, fa = rotation(params.get("angle"), h, w)
    job.rot_mode = mode
    for i in range(6):
        job.a[i], job.fa[i] = a[i], fa[i]
    job.hflip, job.vflip = int(bool(params.get("hflip"))), int(bool(params.get("vflip")))
    for im, key in ((0, "ops_f"), (1, "ops_b")):
        ops = list(params.get(key) or [])
        if len(ops) > MAX_OPS:
            raise ValueError("at most %d colour ops per image, got %d" % (MAX_OPS, len(ops)))
        if sum(1 for name, _ in ops if name == "contrast") > 1:
            raise ValueError("at most one contrast op per image (its mean is taken over the whole image in a pass of its own)")
        job.n_ops[im] = len(ops)
        for k, (name, f) in enumerate(ops):
            if name not in _OP_CODES:
                raise ValueError("unknown colour op %r" % (name,))
            job.op_code[im][k] = _OP_CODES[name]
            if name == "hue":
                job.op_shift[im][k] = int(f * 255) & 0xFF          # adjust_hue's uint8 shift
            else:
                job.op_factor[im][k] = float(f)                    # Image.blend takes a C float
    return job


def _frame(t, dtype, shape, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.ApeError("%s must be a device tensor (the sample builder has no CPU path)" % what)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (what, dtype, t.dtype))
    if tuple(t.shape) != shape:
        raise ValueError("%s must be %s, got %s" % (what, shape, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return t.data_ptr()


_ws = {}


def build_samples(samples, params, mean, std, want_u8=False):
    """samples: per sample a tuple (f_rgb[H,W,3] u8, b_rgb, f_depth[H,W] u16, b_depth, label[H,W] u8) of device tensors (views into a
    resident set; nothing is copied), params: one parameter dict per sample -> x8[B,H,W,8] f32 (7 normalised channels + a zero),
    label[B,H,W] i64 in {0,1}[, u8[B,H,W,7] the un-normalised channels]"""
    if len(samples) != len(params):
        raise ValueError("%d samples but %d parameter sets" % (len(samples), len(params)))
    if not samples:
        raise ValueError("empty batch")
    if len(mean) != 7 or len(std) != 7:
        raise ValueError("mean and std must have 7 entries")
    lab0 = samples[0][4]
    if not torch.is_tensor(lab0) or lab0.dim() != 2:
        raise ValueError("label must be [H,W] (one band)")
    h, w = lab0.shape
    dev = lab0.device
    jobs = (_lib.BgsubTrainJob * len(samples))()
    for i, (s, p) in enumerate(zip(samples, params)):
        f_rgb, b_rgb, f_depth, b_depth, label = s
        jobs[i] = make_job(p, h, w, _frame(f_rgb, torch.uint8, (h, w, 3), "foreground RGB"), _frame(b_rgb, torch.uint8, (h, w, 3), "background RGB"),
                           _frame(f_depth, torch.uint16, (h, w), "foreground depth"), _frame(b_depth, torch.uint16, (h, w), "background depth"),
                           _frame(label, torch.uint8, (h, w), "label"))
    b = len(samples)
    x8 = torch.empty(b, h, w, 8, dtype=torch.float32, device=dev)
    lab = torch.empty(b, h, w, dtype=torch.int64, device=dev)
    u8 = torch.empty(b, h, w, 7, dtype=torch.uint8, device=dev) if want_u8 else None
    nbytes = _lib.lib().ape_bgsub_train_workspace_bytes(b)
    key = (str(dev), _lib.stream_ptr().value)
    ws = _ws.get(key)
    if ws is None or ws.numel() < nbytes:                   # one per stream: the sums of a batch live there between its two launches
        ws = torch.empty(max(nbytes, 16 * 1024), dtype=torch.uint8, device=dev)
        _ws[key] = ws
    m = (ctypes.c_float * 7)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 7)(*[float(v) for v in std])
    _lib.call.ape_bgsub_train_samples(ctypes.cast(jobs, ctypes.c_void_p), b, h, w, ctypes.cast(m, ctypes.c_void_p),
                                      ctypes.cast(sd, ctypes.c_void_p), _lib.dptr(x8), _lib.dptr(lab), _lib.dptr(u8) if want_u8 else None,
                                      _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    return (x8, lab, u8) if want_u8 else (x8, lab)

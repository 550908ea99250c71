"""Augmentation parameters of the background-subtraction training samples and their device builder.

The reference augments in Pillow on the host (background_subtraction/utils.py:414-646).  Here the host only DRAWS the parameters -- from the
reference's generators in the reference's order, `draw_params` -- and turns them into one `ape_bgsub_train_job` per sample (`make_job`);
`build_samples` hands a batch of jobs over raw frames that already live on the device to `ape_bgsub_train_samples` (csrc/bgsub_train.hip).

A parameter set is a dict: angle (None = no rotation step, else the float given to `Image.rotate`), hflip, vflip (bools: applied or not),
ops_f / ops_b (the ordered `(name, factor)` lists of `ColorJitterPIL.params` for the foreground / background image; [] = no jitter)."""
import ctypes
import random

import numpy as np
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd import sample_jobs as J
from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import ColorJitterPIL        # noqa: F401  (the jitter `draw_params` takes)
from autoposeestimation_amd.sample_jobs import ROT_180, ROT_270, ROT_90, ROT_AFFINE, ROT_NONE, rotation     # noqa: F401


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


def make_job(params, h, w, f_rgb, b_rgb, f_depth, b_depth, label):
    """one `ape_bgsub_train_job`; the five frames are addresses (device pointers for the kernel)"""
    job = _lib.BgsubTrainJob()
    job.f_rgb, job.b_rgb, job.f_depth, job.b_depth, job.label = f_rgb, b_rgb, f_depth, b_depth, label
    J.fill_rotation(job.rot, params.get("angle"), h, w)
    job.hflip, job.vflip = int(bool(params.get("hflip"))), int(bool(params.get("vflip")))
    J.fill_jitter(job.jit[0], params.get("ops_f"), " per image")
    J.fill_jitter(job.jit[1], params.get("ops_b"), " per image")
    return job


def build_samples(samples, params, mean, std, want_u8=False):
    """samples: per sample a tuple (f_rgb[H,W,3] u8, b_rgb, f_depth[H,W] u16, b_depth, label[H,W] u8) of device tensors (views into a
    resident set; nothing is copied), params: one parameter dict per sample -> x8[B,H,W,8] f32 (7 normalised channels + a zero),
    label[B,H,W] i64 in {0,1}[, u8[B,H,W,7] the un-normalised channels]"""
    if len(samples) != len(params):
        raise ValueError("%d samples but %d parameter sets" % (len(samples), len(params)))
    if not samples:
        raise ValueError("empty batch")
    m, sd = J.norm(mean, std, 7)
    lab0 = samples[0][4]
    if not torch.is_tensor(lab0) or lab0.dim() != 2:
        raise ValueError("label must be [H,W] (one band)")
    h, w = lab0.shape
    dev = lab0.device
    jobs = (_lib.BgsubTrainJob * len(samples))()
    for i, (s, p) in enumerate(zip(samples, params)):
        f_rgb, b_rgb, f_depth, b_depth, label = s
        jobs[i] = make_job(p, h, w, J.frame(f_rgb, torch.uint8, (h, w, 3), "foreground RGB"), J.frame(b_rgb, torch.uint8, (h, w, 3), "background RGB"),
                           J.frame(f_depth, torch.uint16, (h, w), "foreground depth"), J.frame(b_depth, torch.uint16, (h, w), "background depth"),
                           J.frame(label, torch.uint8, (h, w), "label"))
    b = len(samples)
    x8 = torch.empty(b, h, w, 8, dtype=torch.float32, device=dev)
    lab = torch.empty(b, h, w, dtype=torch.int64, device=dev)
    u8 = torch.empty(b, h, w, 7, dtype=torch.uint8, device=dev) if want_u8 else None
    ws = J.workspace("bgsub", dev, _lib.lib().ape_bgsub_train_workspace_bytes(b))         # the sums of a batch between its two launches
    _lib.call.ape_bgsub_train_samples(ctypes.cast(jobs, ctypes.c_void_p), b, h, w, m, sd, _lib.dptr(x8), _lib.dptr(lab),
                                      _lib.dptr(u8) if want_u8 else None, _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    return (x8, lab, u8) if want_u8 else (x8, lab)

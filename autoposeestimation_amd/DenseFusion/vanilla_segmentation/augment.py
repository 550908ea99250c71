"""Device builder of SegNet's training samples (csrc/segnet_samples.hip): the job structure, the job filling and the two launches.

The reference builds a sample in Pillow and numpy on the host (data_controller.py:43-93).  Here the host only DRAWS; a batch over frames
that already live on the device is `ape_segnet_samples_prepare` (the blurred `data_syn` frames and the L sums of the contrast ops) ->
`ape_segnet_samples` (jitter, composite, flip, Normalize).  No draw depends on a pixel, so nothing is read back; the one upload is the
float64 noise of the `data_syn` samples (24 bytes per pixel), staged once per batch.

A parameter set is a dict: ops (the ordered `(name, factor)` list of `ColorJitterPIL.params()` that is APPLIED to the frame; None or []
= none), flip (0 left-right, 1 up-down, 2 both, 3 or None neither), and for a `data_syn` sample noise (f64 [3,H,W]) and ops_back (the
background's list).  Every index the kernels take from here is range-checked before the launch."""
import ctypes

import numpy as np
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd import sample_jobs as J

_c = ctypes
NORM_MEAN, NORM_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BRIGHTNESS, BLUR_RADIUS = 1.5, 0.8          # data_controller.py:58-59


class SegnetJob(_c.Structure):
    """Mirror of `ape_segnet_job` (include/ape_hip.h); tests/test_segnet_samples_host.py compares the layout with the C compiler's."""
    _fields_ = [("rgb", _c.c_void_p), ("label", _c.c_void_p), ("back_rgb", _c.c_void_p), ("back_label", _c.c_void_p),
                ("noise_off", _c.c_longlong), ("blur_off", _c.c_longlong), ("jit", _lib.AugJitter * 2), ("bright", _c.c_float),
                ("blur_ww", _c.c_uint32), ("blur_fw", _c.c_uint32), ("flip", _c.c_int32)]


def blur_weights(radius, passes=3):
    """-> (ww, fw): the 8.24 fixed-point weights of the centre and of each neighbour in one pass of the box blur that Pillow's
    `ImageFilter.GaussianBlur(radius)` runs (BoxBlur.c: _gaussian_blur_radius in C floats with double intermediates, then
    ImagingLineBoxBlur8's `ww = (UINT32)(1 << 24) / (2 r + 1)`, `fw = ((1 << 24) - ww) / 2`).  Only a box of integer radius 0 -- three
    taps -- is restated; a larger Gaussian radius is refused."""
    f32 = np.float32
    r = f32(radius)
    if not (r > 0):
        raise ValueError("blur radius %r: Pillow skips the blur, and so must the caller" % (radius,))
    sigma2 = f32(r * r / f32(passes))
    length = f32(np.sqrt(12.0 * float(sigma2) + 1.0))
    whole = f32(np.floor((float(length) - 1.0) / 2.0))
    if whole != 0:
        raise ValueError("blur radius %r gives a box of integer radius %d; only the three-tap box (integer radius 0) is provided"
                         % (radius, int(whole)))
    a = f32(f32(2 * whole + 1) * f32(whole * f32(whole + 1) - 3 * sigma2))
    a = f32(a / f32(6 * f32(sigma2 - f32(whole + 1) * f32(whole + 1))))
    box = f32(whole + a)
    ww = int(f32(f32(1 << 24) / f32(box * 2 + 1)))
    fw = ((1 << 24) - ww) // 2
    return ww, fw


def _addr(t, dtype, shape, what):
    """the address of a resident frame after `sample_jobs.frame`'s checks; an int is an address already (tools/check_segnet_px.py: host
    arrays)"""
    return t if isinstance(t, int) else J.frame(t, dtype, shape, what)


def make_job(frame, h, w, params, back=None):
    """frame: (rgb u8 [H,W,3], label u8 [H,W]) device tensors; back: None or the same pair of the real frame a `data_syn` sample is
    composited with -> SegnetJob (blur_off and noise_off are set by `build_samples`)"""
    job = SegnetJob()
    job.rgb = _addr(frame[0], torch.uint8, (h, w, 3), "frame")
    job.label = _addr(frame[1], torch.uint8, (h, w), "label")
    J.fill_jitter(job.jit[0], params.get("ops"))
    flip = params.get("flip")
    flip = 3 if flip is None else int(flip)
    if not 0 <= flip <= 3:
        raise ValueError("flip %r outside 0..3" % (params.get("flip"),))
    job.flip = flip
    job.noise_off = job.blur_off = -1
    if back is not None:
        job.back_rgb = _addr(back[0], torch.uint8, (h, w, 3), "background")
        job.back_label = _addr(back[1], torch.uint8, (h, w), "background label")
        J.fill_jitter(job.jit[1], params.get("ops_back"), " of the background")
        job.bright = float(params.get("brightness", BRIGHTNESS))
        job.blur_ww, job.blur_fw = blur_weights(params.get("blur_radius", BLUR_RADIUS))
    return job


def _noise(p, h, w, k):
    noise = p.get("noise")
    if noise is None:
        raise ValueError("sample %d: a `data_syn` sample needs its noise" % k)
    noise = np.asarray(noise)
    if noise.shape != (3, h, w) or noise.dtype != np.float64:
        raise ValueError("sample %d: the noise must be float64 %s, got %s %s" % (k, (3, h, w), noise.dtype, noise.shape))
    return noise


def build_samples(frames, params, backs=None, mean=NORM_MEAN, std=NORM_STD, timings=None):
    """frames: per sample (rgb u8 [H,W,3], label u8 [H,W]) device tensors of one size (views into a resident set; nothing is copied);
    params: one parameter dict per sample; backs: per sample None or the (rgb, label) pair of its background, which makes the sample a
    `data_syn` one -> rgb f32 [B,3,H,W], target i64 [B,H,W].  timings: None, or a dict that receives 'upload' and 'kernels' in ms (HIP events;
    the call then waits for the device)."""
    if not frames:
        raise ValueError("empty batch")
    backs = list(backs) if backs is not None else [None] * len(frames)
    if len(frames) != len(params) or len(frames) != len(backs):
        raise ValueError("%d frames, %d parameter sets, %d backgrounds" % (len(frames), len(params), len(backs)))
    lab0 = frames[0][1]
    if not torch.is_tensor(lab0) or lab0.dim() != 2:
        raise ValueError("label must be [H,W] (one band)")
    h, w = (int(v) for v in lab0.shape)
    dev, b = lab0.device, len(frames)
    L = _lib.lib()
    jobs = (SegnetJob * b)()
    for k in range(b):
        jobs[k] = make_job(frames[k], h, w, params[k], backs[k])
    # the workspace behind the sums: the blurred frames (16-byte aligned), then the noise planes in one run, so that one copy fills them
    syn = [k for k in range(b) if backs[k] is not None]
    end = L.ape_segnet_samples_frames_offset(b)
    for k in syn:
        jobs[k].blur_off = end
        end += (h * w * 3 + 15) & ~15
    n0 = end
    noises = [_noise(params[k], h, w, k) for k in syn]
    for k in syn:
        jobs[k].noise_off = end
        end += 24 * h * w
    ws = J.workspace("segnet", dev, end)
    for k in syn:                                                # what the kernels index with lies inside the workspace
        if not (0 < jobs[k].blur_off <= n0 - 3 * h * w and n0 <= jobs[k].noise_off <= ws.numel() - 24 * h * w):
            raise _lib.ApeError("sample %d: workspace offsets outside the workspace" % k)
    jp = _c.cast(jobs, _c.c_void_p)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
    if ev:
        ev[0].record()
    if noises:                                                   # one staging buffer, one copy
        stage = np.empty((len(noises), 3, h, w), np.float64)
        for i, noise in enumerate(noises):
            stage[i] = noise
        ws[n0:end].copy_(torch.from_numpy(stage.reshape(-1).view(np.uint8)))
    if ev:
        ev[1].record()
    if noises or any(j.jit[0].n_ops for j in jobs):
        _lib.call.ape_segnet_samples_prepare(jp, b, h, w, _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    rgb = torch.empty(b, 3, h, w, dtype=torch.float32, device=dev)
    target = torch.empty(b, h, w, dtype=torch.int64, device=dev)
    m, sd = J.norm(mean, std, 3)
    _lib.call.ape_segnet_samples(jp, b, h, w, m, sd, _lib.dptr(rgb), _lib.dptr(target), _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    if ev:
        ev[2].record()
        ev[2].synchronize()
        timings["upload"], timings["kernels"] = ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])
    return rgb, target

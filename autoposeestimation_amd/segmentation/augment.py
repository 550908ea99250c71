"""Device builder of the segmentor's training samples (csrc/seg_train.hip) and the tables it needs.

The reference augments in Pillow on the host, per sample (segmentation/dataset.py:88-112): colorJitter -> rotate -> CropAndZoom ->
toTensor -> normalize.  Here the host only DRAWS (segmentation/utils.py's `params` methods, the reference's generators in the reference's
order) and builds the resize tables; `build_samples` runs a batch over frames that already live on the device in two launches:
`ape_seg_train_stats` (the L sums of the contrast ops and the extents of the rotated labels), one read-back of the extent partials -- the
crop box needs them: the upper bound of CropAndZoom's `np.random.randint(0, n)` is the object's size --, `ape_seg_train_samples`.

A parameter set is a dict: ops (the ordered `(name, factor)` list of `colorJitter.params()`; [] = none), angle (the float given to
`Image.rotate`; None = no rotation), and either box (`CropAndZoom.params(...)`: left, upper, right, lower) or zoom
(`CropAndZoom.draw_zoom()`), from which the box is drawn once the extents are known.

Draw order.  The reference draws per sample: jitter and angle and zoom from `random`, then at most one `np.random.randint`.  Only the last
depends on the label, and it is the only draw from `numpy.random`, so drawing jitter, angle and zoom of every sample of the batch before
the first launch and the randints after the read-back, both in sample order, leaves either generator's stream as the reference has it."""
import ctypes
import functools

import numpy as np
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd import sample_jobs as J

PRECISION_BITS = 22          # Resample.c, 8-bit images: 32 - 8 - 2
TAPS = 5                     # (int)ceil(BICUBIC's support 2.0) * 2 + 1


def _bicubic(x):
    """Resample.c bicubic_filter, a = -0.5, on an array of doubles"""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


# (both table caches: a key is (crop side, output side); a training run has one output side and at most output_size / 2 even crop sides
# -- ~240 entries of ~12 KB at 480 -- so the bound is never reached there and only guards a caller that sweeps sizes)
@functools.lru_cache(maxsize=1024)
def bicubic_table(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis of an ENLARGEMENT n_in -> n_out (BICUBIC): -> (xmin[n_out] i32,
    k[n_out, 5] i32): output x is clip8((2^21 + sum_i in[xmin[x] + i] * k[x, i]) >> 22); weights past the filter's reach are 0."""
    if not 1 <= n_in <= n_out:
        raise ValueError("only enlargement is provided: %d -> %d" % (n_in, n_out))
    scale = float(n_in) / n_out
    support = 2.0                                    # filterscale = max(scale, 1) = 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int) truncates; the arguments are > -2
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    w = np.zeros((n_out, TAPS), np.float64)
    ww = np.zeros(n_out, np.float64)
    for x in range(TAPS):
        wx = np.where(x < xmax, _bicubic((x + xmin).astype(np.float64) - center + 0.5), 0.0)
        w[:, x] = wx
        ww = ww + wx                                 # summed in tap order, as the C loop does
    assert int(xmax.max()) <= TAPS
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int64)      # (int) truncates
    return xmin.astype(np.int32), k.astype(np.int32)


@functools.lru_cache(maxsize=1024)
def nearest_table(n_in, n_out):
    """ImagingScaleAffine's index table of `resize(NEAREST)` n_in -> n_out: xo = scale * 0.5, index (int)xo, xo += scale accumulated in
    double"""
    if n_in < 1 or n_out < 1:
        raise ValueError("sizes must be positive")
    scale = float(n_in) / n_out
    xo = 0.0 + scale * 0.5
    idx = np.empty(n_out, np.int32)
    for x in range(n_out):
        idx[x] = -1 if xo < 0.0 else int(xo)
        xo += scale
    return idx


def resize_tables(side, out):
    """the table block of one sample as ape_seg_train_samples reads it: hmin[S], hk[S][5], vmin[S], vk[S][5], nx[S], ny[S] (the crop is
    square, so both axes share their tables) -> i32[14 * S]"""
    xmin, k = bicubic_table(int(side), int(out))
    near = nearest_table(int(side), int(out))
    return np.concatenate([xmin, k.reshape(-1), xmin, k.reshape(-1), near, near])


def make_job(params, h, w, rgb, label, class_id):
    """one `ape_seg_train_job` without its crop; the frames are addresses (device pointers for the kernels)"""
    job = _lib.SegTrainJob()
    job.rgb, job.label, job.class_id = rgb, label, int(class_id)
    J.fill_rotation(job.rot, params.get("angle"), h, w)
    J.fill_jitter(job.jit, params.get("ops"))
    return job


def set_crop(job, box, out):
    left, upper, right, lower = [int(v) for v in box]
    if right - left != lower - upper or right <= left:
        raise ValueError("the crop box %r is not a square" % (tuple(box),))
    if right - left > out:
        raise ValueError("crop side %d above the output side %d: only enlargement is provided" % (right - left, out))
    job.crop_x, job.crop_y, job.crop_side = left, upper, right - left


def _jobs(samples, params, class_ids):
    if not samples:
        raise ValueError("empty batch")
    if len(samples) != len(params) or len(samples) != len(class_ids):
        raise ValueError("%d samples, %d parameter sets, %d class ids" % (len(samples), len(params), len(class_ids)))
    lab0 = samples[0][1]
    if not torch.is_tensor(lab0) or lab0.dim() != 2:
        raise ValueError("label must be [H,W] (one band)")
    h, w = lab0.shape
    jobs = (_lib.SegTrainJob * len(samples))()
    for i, ((rgb, label), p, cid) in enumerate(zip(samples, params, class_ids)):
        jobs[i] = make_job(p, h, w, J.frame(rgb, torch.uint8, (h, w, 3), "frame"), J.frame(label, torch.uint8, (h, w), "label"), cid)
    return jobs, h, w, lab0.device


def build_samples(samples, params, class_ids, mean, std, crop, names=None):
    """samples: per sample (rgb[H,W,3] u8, label[H,W] u8) device tensors (views into a resident set; nothing is copied), params: one
    parameter dict per sample, crop: the CropAndZoom that draws the boxes -> img[B,3,S,S] f32, label[B,S,S] i64 (class id where the label
    is set), boxes (the crop boxes used, one (left, upper, right, lower) per sample)"""
    jobs, h, w, dev = _jobs(samples, params, class_ids)
    b, out = len(samples), int(crop.output_size)
    L = _lib.lib()
    ws = J.workspace("seg", dev, L.ape_seg_train_workspace_bytes(b, out))
    jp = ctypes.cast(jobs, ctypes.c_void_p)
    boxes = [p.get("box") for p in params]
    if any(bx is None for bx in boxes) or any(j.jit.n_ops for j in jobs):
        _lib.call.ape_seg_train_stats(jp, b, h, w, _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    if any(bx is None for bx in boxes):
        e0, e1 = L.ape_seg_train_extents_offset(b), L.ape_seg_train_tables_offset(b)
        ext = J.combine_extents(ws[e0:e1].view(torch.int32).cpu().numpy(), 5)     # the one read-back of the batch
        for i, p in enumerate(params):
            if boxes[i] is None:
                if ext[i, 4] == 0:
                    raise ValueError("the label of sample %s has no pixel equal to 255 after its rotation: CropAndZoom has no object to "
                                     "crop around" % (i if names is None else names[i],))
                boxes[i] = crop.params(ext[i, :4], (h, w), zoom=p.get("zoom"))
    tab = np.empty((b, 14 * out), np.int32)
    for i in range(b):
        set_crop(jobs[i], boxes[i], out)
        tab[i] = resize_tables(jobs[i].crop_side, out)
    t0 = L.ape_seg_train_tables_offset(b)
    ws[t0:t0 + tab.nbytes].view(torch.int32).copy_(torch.from_numpy(tab).view(-1))
    img = torch.empty(b, 3, out, out, dtype=torch.float32, device=dev)
    lab = torch.empty(b, out, out, dtype=torch.int64, device=dev)
    m, sd = J.norm(mean, std, 3)
    _lib.call.ape_seg_train_samples(jp, b, h, w, out, m, sd, _lib.dptr(img), _lib.dptr(lab), _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    return img, lab, [tuple(int(v) for v in bx) for bx in boxes]


def plain_samples(samples, class_ids, mean, std):
    """the un-augmented samples of mode 'test' -> img[B,3,H,W] f32, label[B,H,W] i64"""
    jobs, h, w, dev = _jobs(samples, [{}] * len(samples), class_ids)
    b = len(samples)
    img = torch.empty(b, 3, h, w, dtype=torch.float32, device=dev)
    lab = torch.empty(b, h, w, dtype=torch.int64, device=dev)
    m, sd = J.norm(mean, std, 3)
    _lib.call.ape_seg_plain_samples(ctypes.cast(jobs, ctypes.c_void_p), b, h, w, m, sd, _lib.dptr(img), _lib.dptr(lab), _lib.stream_ptr())
    return img, lab

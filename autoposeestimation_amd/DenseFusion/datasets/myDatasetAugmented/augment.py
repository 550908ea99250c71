"""Device builder of DenseFusion's training samples (csrc/pose_train.hip) and the host arithmetic between its two launches.

The reference builds a sample in Pillow and numpy on the host (dataset.py:158-326): colour jitter -> rotation of colour, label and depth ->
get_bbox -> `choose` -> back-projection -> normalised crop.  Here the host only DRAWS (PoseDataset.batch, the reference's generators in the
reference's order) and does get_bbox's integer arithmetic; `build_samples` runs a batch over frames that already live on the device:
`ape_pose_train_stats` (the L sums of the contrast ops, the extents of the rotated labels, the valid pixels per row), one read-back of
extents and row counts (a few KB per sample) -- the crop needs the extents and the `c_mask` draw needs the count --, one upload of the row
prefixes and the ranks to keep, `ape_pose_train_samples`.

A parameter set is a dict: ops (the ordered `(name, factor)` list of `ColorJitterPIL.params()`; [] = none), angle (the float given to
`Image.rotate`; None = no rotation), add_t (3 floats, the translation noise)."""
import ctypes

import numpy as np
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd import sample_jobs as J
from autoposeestimation_amd.DenseFusion.datasets import packed
from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import bbox_from_extents


def make_job(params, h, w, rgb, depth, label, intr, depth_scale, to_meter, add_noise):
    """one `ape_pose_train_job` without its crop and output offset; the frames are addresses (device pointers for the kernels)"""
    job = _lib.PoseTrainJob()
    job.rgb, job.depth, job.label = rgb, depth, label
    J.fill_rotation(job.rot, params.get("angle") if add_noise else None, h, w)
    J.fill_jitter(job.jit, params.get("ops") if add_noise else None)
    # numpy computes the cloud in float32: the Python floats of the meta file enter as float32 scalars
    job.ppx, job.ppy, job.fx, job.fy = float(intr["ppx"]), float(intr["ppy"]), float(intr["fx"]), float(intr["fy"])
    job.depth_scale = float(depth_scale)
    job.to_meter, job.add_noise = int(bool(to_meter)), int(bool(add_noise))
    if add_noise:
        for k in range(3):
            job.add_t[k] = float(params["add_t"][k])
    return job


def set_crop(job, box):
    job.rmin, job.rmax, job.cmin, job.cmax = [int(v) for v in box]


def build_samples(samples, params, cams, num_pt, to_meter, add_noise, mean, std, select, names=None):
    """samples: per sample (rgb[H,W,3] u8, depth[H,W] u16, label[H,W] u8) device tensors (views into a resident set; nothing is copied);
    params: one parameter dict per sample; cams: per sample (intr dict, depth_scale); select(k, count): called once per sample, in sample
    order, after the read-back, with the number of valid pixels -- the place of the draws that depend on it -- and returns the sorted ranks
    to keep when count > num_pt -> per sample (points[1,N,3] f32, choose[1,1,N] i64, img[1,3,Hc,Wc] f32): views into ONE packed block"""
    if not samples:
        raise ValueError("empty batch")
    if len(samples) != len(params) or len(samples) != len(cams):
        raise ValueError("%d samples, %d parameter sets, %d cameras" % (len(samples), len(params), len(cams)))
    lab0 = samples[0][2]
    if not torch.is_tensor(lab0) or lab0.dim() != 2:
        raise ValueError("label must be [H,W] (one band)")
    h, w = lab0.shape
    dev, b, n = lab0.device, len(samples), int(num_pt)
    name = lambda i: i if names is None else names[i]  # noqa: E731
    jobs = (_lib.PoseTrainJob * b)()
    for i, ((rgb, depth, label), p, (intr, scale)) in enumerate(zip(samples, params, cams)):
        jobs[i] = make_job(p, h, w, J.frame(rgb, torch.uint8, (h, w, 3), "frame"), J.frame(depth, torch.uint16, (h, w), "depth"),
                           J.frame(label, torch.uint8, (h, w), "label"), intr, scale, to_meter, add_noise)
    L = _lib.lib()
    ws = J.workspace("pose", dev, L.ape_pose_train_workspace_bytes(b, h, n))
    jp = ctypes.cast(jobs, ctypes.c_void_p)
    _lib.call.ape_pose_train_stats(jp, b, h, w, _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    e0, r0, t0 = L.ape_pose_train_extents_offset(b), L.ape_pose_train_rows_offset(b), L.ape_pose_train_tables_offset(b, h)
    back = ws[e0:t0].cpu().numpy()                               # the one read-back of the batch
    ext = J.combine_extents(back[:r0 - e0].view(np.int32), 4)
    rows = back[r0 - e0:r0 - e0 + b * h * 4].view(np.int32).reshape(b, h)
    sels = []
    for i in range(b):
        if ext[i, 1] < 0:
            raise ValueError("sample %s: the label has no pixel equal to 255%s: get_bbox has no object to crop around"
                             % (name(i), " after its rotation" if jobs[i].rot.mode else ""))
        count = int(rows[i].sum())               # whole rows: every labelled pixel lies inside the crop (csrc/pose_train.hip)
        if count == 0:
            raise ValueError("sample %s: no pixel of the label has a depth: there is no point to choose" % (name(i),))
        sels.append(packed.selection(count, n, select(i, count)))
        set_crop(jobs[i], bbox_from_extents(*ext[i]))
    offsets, total = packed.plan(jobs, [True] * b, n)
    packed.upload(ws, t0, packed.table(rows, sels, n))           # the one upload: row prefixes and ranks
    block = torch.empty(total, dtype=torch.uint8, device=dev)
    m, sd = J.norm(mean, std, 3)
    _lib.call.ape_pose_train_samples(jp, b, h, w, n, m, sd, _lib.dptr(block), block.numel(), _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
    return packed.views(block, offsets, jobs, n)

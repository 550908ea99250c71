"""What the three device builders of training samples share on the host (background_subtraction/augment.py, segmentation/augment.py,
DenseFusion/datasets/myDatasetAugmented/augment.py): the rotation and the colour-op list of a job (`ape_aug_rotation`, `ape_aug_jitter` of
include/ape_hip.h), the check of a resident frame, the per-stream workspace, the Normalize arrays and the extent partials."""
import ctypes
import math

import numpy as np
import torch

from autoposeestimation_amd import _lib

ROT_NONE, ROT_180, ROT_AFFINE, ROT_90, ROT_270 = 0, 1, 2, 3, 4
OP_CODES = {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4}
MAX_OPS = 4
PARTIALS = 64                # extent / sum partials per sample (csrc/sample_batch.h kBlocks)


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


def fill_rotation(rot, angle, h, w):
    """`Image.rotate(angle)` of an h x w image into an `_lib.AugRotation`"""
    rot.mode, rot.a[:], rot.fa[:] = rotation(angle, h, w)


def fill_jitter(jit, ops, what=""):
    """the ordered `(name, factor)` list of `ColorJitterPIL.params()` into an `_lib.AugJitter`; `what` names the list in the messages"""
    ops = list(ops or [])
    if len(ops) > MAX_OPS:
        raise ValueError("at most %d colour ops%s, got %d" % (MAX_OPS, what, len(ops)))
    if sum(1 for name, _ in ops if name == "contrast") > 1:
        raise ValueError("at most one contrast op%s (its mean is taken over the whole image in a pass of its own)" % what)
    jit.n_ops = len(ops)
    code, factor, shift = jit.code, jit.factor, jit.shift
    for k, (name, f) in enumerate(ops):
        if name not in OP_CODES:
            raise ValueError("unknown colour op %r" % (name,))
        code[k] = OP_CODES[name]
        if name == "hue":
            shift[k] = int(f * 255) & 0xFF                     # adjust_hue's uint8 shift
        else:
            factor[k] = float(f)                               # Image.blend takes a C float


def frame(t, dtype, shape, what):
    """the address of a resident frame, after the checks the kernels cannot make"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.ApeError("%s must be a device tensor (the sample builder has no CPU path)" % what)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (what, dtype, t.dtype))
    if tuple(t.shape) != shape:
        raise ValueError("%s must be %s, got %s" % (what, shape, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return t.data_ptr()


_ws = {}          # (builder, device, stream) -> workspace, kept for the life of the process: one entry per builder and stream that ever
                  # built a batch (the drivers use one stream), at most ~30 KB per sample of the largest batch seen there


def workspace(builder, dev, nbytes):
    """one per builder and stream: it carries a batch's sums and tables between its launches"""
    key = (builder, str(dev), _lib.stream_ptr().value)
    ws = _ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 64 * 1024), dtype=torch.uint8, device=dev)
        _ws[key] = ws
    return ws


def norm(mean, std, n):
    """Normalize's mean / std as the host pointers to C floats an entry point reads (each keeps its array alive)"""
    if len(mean) != n or len(std) != n:
        raise ValueError("mean and std must have %d entries" % n)
    return [ctypes.cast((ctypes.c_float * n)(*[float(v) for v in a]), ctypes.c_void_p) for a in (mean, std)]


def combine_extents(partials, width):
    """[B, PARTIALS, width] partials of a statistics pass -> [B, width]: (min row, max row, min column, max column[, count])"""
    p = np.asarray(partials).reshape(-1, PARTIALS, width)
    cols = [p[:, :, 0].min(1), p[:, :, 1].max(1), p[:, :, 2].min(1), p[:, :, 3].max(1)] + [p[:, :, k].sum(1) for k in range(4, width)]
    return np.stack(cols, 1)

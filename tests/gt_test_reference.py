"""numpy restatement of the two label-audit kernels' contracts (include/ape_hip.h, csrc/label_audit.hip), written from the contract:
what the GPU tests hold the device to, and what tests/test_gt_test_host.py holds to the values recorded from the reference."""
import numpy as np


def pair_counts(labels, pairs):
    """labels u8 [B,L,...], pairs [(a, b)] -> int64 [B,P,4]: a fg & b fg, a fg & b bg, a bg & b fg, both bg (fg = byte not zero)"""
    labels = np.asarray(labels)
    fg = labels.reshape(labels.shape[0], labels.shape[1], -1) != 0
    out = np.zeros((fg.shape[0], len(pairs), 4), dtype=np.int64)
    for j, (a, b) in enumerate(pairs):
        fa, fb = fg[:, a], fg[:, b]
        out[:, j, 0] = (fa & fb).sum(axis=1)
        out[:, j, 1] = (fa & ~fb).sum(axis=1)
        out[:, j, 2] = (~fa & fb).sum(axis=1)
        out[:, j, 3] = (~fa & ~fb).sum(axis=1)
    return out


def ratios(counts4):
    """[iou, accuracy, precision, recall] in the reference's naming, Python float division of the integers"""
    tp, fp, fn, tn = (int(v) for v in counts4)
    return [tp / (tp + fp + fn), (tp + tn) / (tp + tn + fp + fn), tp / (tp + fp), tp / (tp + fn)]


def pair_blend(rgb, labels, first, second, c0, c1):
    """rgb u8 [B,H,W,3], labels u8 [B,L,H,W] -> u8 [B,H,W,3]: per step `v*c0 + label*c1` in float64 (two roundings), truncated, in the
    step's channel where its plane is not zero; the second step reads the first's result"""
    out = np.array(rgb, dtype=np.uint8, copy=True)
    for plane, ch in (first, second):
        lab = np.asarray(labels)[:, plane]
        prod = out[..., ch].astype(np.float64) * np.float64(c0)
        add = lab.astype(np.float64) * np.float64(c1)
        val = np.trunc(prod + add).astype(np.int64).astype(np.uint8)
        out[..., ch] = np.where(lab != 0, val, out[..., ch])
    return out

"""Generates tests/golden/seg_train_metrics.npz from the REFERENCE's own segmentation/utils.py (jaccard_loss, ConfusionMatrix, IoU),
run on the CPU here through tools/ref_shim.py.  Only the numbers go into the fixture; nothing under tests/ reads the reference.

    python tools/gen_golden_segtrain.py

Loss cases: logits [B,C,H,W] (C in 1, 2, 5, 13; some classes absent from the labels; +-80 logits; labels [B,H,W] and [B,1,H,W]) ->
the loss value and d loss / d logits by torch autograd through the reference's function.  Metric cases: scores (with planted arg-max
ties) or labels as predictions, several add() calls, ignore_index, normalized=True -> the confusion matrix and IoU.value()."""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_shim  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "seg_train_metrics.npz")


def _ref_utils():
    ref_shim.install()
    path = os.path.join(ref_shim.REFERENCE_ROOT, "segmentation", "utils.py")
    spec = importlib.util.spec_from_file_location("_ref_segmentation_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


LOSS_CASES = [  # name, B, C, H, W, logit scale, classes present (None: all), label shape with the extra axis
    ("c1", 2, 1, 5, 7, 3.0, None, False),
    ("c2", 2, 2, 8, 6, 2.0, None, True),
    ("c5_absent", 3, 5, 6, 9, 4.0, (0, 2, 3), False),
    ("c13", 2, 13, 7, 8, 3.0, None, False),
    ("c13_absent", 1, 13, 9, 11, 2.0, (0, 1, 4, 7, 12), True),
    ("c5_pm80", 2, 5, 4, 6, 80.0, None, False),
    ("c1_pm80", 2, 1, 6, 5, 80.0, None, True),
    ("c13_single", 2, 13, 4, 4, 1.0, (3,), False),
]

METRIC_CASES = [  # name, K, list of (B, H, W) adds, prediction kind, ignore_index, normalized
    ("k5_scores", 5, [(2, 6, 7), (1, 8, 5), (3, 4, 4)], "scores", None, False),
    ("k13_scores_ties", 13, [(2, 9, 10), (2, 5, 6)], "ties", None, False),
    ("k4_labels", 4, [(2, 7, 7), (1, 3, 9)], "labels", None, False),
    ("k6_ignore", 6, [(2, 8, 8)], "scores", 0, False),
    ("k6_ignore_list", 6, [(2, 8, 8), (1, 4, 4)], "scores", (1, 5), False),
    ("k5_normalized", 5, [(2, 6, 6), (2, 3, 5)], "scores", None, True),
    ("k7_absent", 7, [(2, 6, 6)], "labels_absent", None, False),
]


def main():
    U = _ref_utils()
    g = torch.Generator().manual_seed(20261016)
    out = {}
    for name, b, c, h, w, scale, present, extra in LOSS_CASES:
        logits = (torch.randn(b, c, h, w, generator=g) * scale).float()
        pool = torch.tensor(present if present is not None else list(range(max(c, 2))))
        lab = pool[torch.randint(0, len(pool), (b, h, w), generator=g)]
        if present is None:
            lab.view(-1)[:len(pool)] = pool          # every class present
        lab = lab.long()
        x = logits.clone().requires_grad_(True)
        loss = U.jaccard_loss(lab.view(b, 1, h, w) if extra else lab, x)
        loss.backward()
        out["loss_%s_logits" % name] = logits.numpy()
        out["loss_%s_labels" % name] = lab.numpy()
        out["loss_%s_extra_axis" % name] = np.array(extra)
        out["loss_%s_value" % name] = np.array(float(loss.detach()), np.float64)
        out["loss_%s_grad" % name] = x.grad.numpy()
    for name, k, adds, kind, ignore, normalized in METRIC_CASES:
        m = U.IoU(k, normalized=normalized, ignore_index=ignore)
        for i, (b, h, w) in enumerate(adds):
            tgt = torch.randint(0, k, (b, h, w), generator=g).long()
            if kind == "labels_absent":
                tgt = tgt % 3 * 2                      # 0, 2, 4 only: 1, 3, 5, 6 never a target
            if kind in ("labels", "labels_absent"):
                pred = torch.randint(0, k, (b, h, w), generator=g).long()
            else:
                pred = torch.randn(b, k, h, w, generator=g).float()
                if kind == "ties":
                    # planted ties: the maximum repeated in a later channel (first maximum wins), whole-pixel constant scores
                    pred[:, 7] = pred.max(1).values
                    pred[0, :, 0, 0] = 0.5
                    pred[1, :, 2, :] = pred[1, :, 2, :].max(0).values
            m.add(pred, tgt)
            out["metric_%s_pred%d" % (name, i)] = pred.numpy()
            out["metric_%s_target%d" % (name, i)] = tgt.numpy()
        iou, miou = m.value()
        out["metric_%s_conf" % name] = np.array(m.conf_metric.value(), dtype=np.float64 if normalized else np.int64)
        out["metric_%s_iou" % name] = np.asarray(iou, np.float64)
        out["metric_%s_miou" % name] = np.array(miou, np.float64)
        out["metric_%s_adds" % name] = np.array(len(adds))
        out["metric_%s_k" % name] = np.array(k)
        out["metric_%s_ignore" % name] = np.array([] if ignore is None else np.atleast_1d(ignore), np.int64)
        out["metric_%s_normalized" % name] = np.array(normalized)
    out["loss_cases"] = np.array([c[0] for c in LOSS_CASES])
    out["metric_cases"] = np.array([c[0] for c in METRIC_CASES])
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, len(out), "arrays")


if __name__ == "__main__":
    main()

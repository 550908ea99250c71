"""The reference's label-quality test (experiments/gt_test.py): the three label sources -- the trained segmentor's relabelling
(`.new_pred.label.png`), the background-subtraction segmentor (`.pred.label.png`) and the classical RGB-D labeller (`.gen.label.png`) --
against hand-annotated masks and against each other: five label pairs, each scored by IoU, accuracy, "precision", "recall" and the share
of samples with IoU >= 0.5.

Naming: the counts keep the reference's names (gt_test.py:160-194).  With (ground_truth, label) they are the four values of its uint8
difference: 0 = both foreground (`tp`), 1 = ground truth foreground only (`fp`), 2 = label foreground only (`fn`), 3 = both background
(`tn`).  `fp` and `fn` are swapped against the textbook meaning, so "precision" = tp / (tp + fp) is the textbook recall and the other
way round.  Restated, not corrected: the printed table is the reference's.

On the device the counts of all five pairs of a batch come from one launch (`engine.label_pair_counts`, csrc/label_audit.hip); the ratios
are Python float divisions of those integers, bit-equal to `compute_IoU`.  `use_cuda=False` is the numpy path.

Not built: `change_contrast` (CLAHE through OpenCV; `main` never calls it) and the matplotlib figures.  The comparison images behind the
reference's `plot_labels` switch (dead code there: the switch is a constant False) are written as PNG files when `overlay_dir` is given."""
import os
import time

import numpy as np
from PIL import Image

TAG = ".color.mask.0.png"
PLANES = ("gt", "new_pred", "pred", "gen")                      # the label planes of one sample, in upload order
NAMES = ("gt_vs_new_pred", "gt_vs_pred", "pred_vs_new_pred", "gt_vs_gen", "gen_vs_pred")
PAIRS = ((0, 1), (0, 2), (2, 1), (0, 3), (3, 2))                # (ground_truth, label) of compute_IoU for NAMES, as plane indices
# the reference's five lines (:152-156): four of them end in a blank
LINES = ("gt_vs_new_pred:      iou = {}, accuracy = {}, precision = {}, recall = {}, iou >= 0.5: {}",
         "gt_vs_pred:          iou = {}, accuracy = {}, precision = {}, recall = {}, iou >= 0.5: {} ",
         "pred_vs_new_pred:    iou = {}, accuracy = {}, precision = {}, recall = {}, iou >= 0.5: {} ",
         "gt_vs_gen:           iou = {}, accuracy = {}, precision = {}, recall = {}, iou >= 0.5: {} ",
         "gen_vs_pred:         iou = {}, accuracy = {}, precision = {}, recall = {}, iou >= 0.5: {} ")
C0 = 0.7
C1 = 1.0 - C0
CH_PRED, CH_OTHER = 2, 0                                        # ch1 (pred) and ch2 (new_pred, gen) of :22-23
OVERLAYS = (("pred_vs_new_pred", 2, 1), ("pred_vs_gen", 2, 3))  # file tag, plane into CH_PRED, plane into CH_OTHER


def ratios(tp, fp, fn, tn):
    """[iou, accuracy, precision, recall] of four integer counts (:190-194); ZeroDivisionError where the reference raises it"""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    iou = float(tp) / float(tp + fp + fn)
    accuracy = (tp + tn) / (tp + tn + fp + fn)
    precision = float(tp) / float(tp + fp)
    recall = float(tp) / float(tp + fn)
    return [iou, accuracy, precision, recall]


def pixel_counts(ground_truth, label):
    """(tp, fp, fn, tn) of two host arrays of one size, non-zero = foreground; the inputs are not modified"""
    a = np.asarray(ground_truth).reshape(-1) != 0
    b = np.asarray(label).reshape(-1) != 0
    if a.size != b.size:
        raise ValueError("ground truth has %d pixels, the label %d" % (a.size, b.size))
    tp = int(np.count_nonzero(a & b))
    fp = int(np.count_nonzero(a)) - tp
    fn = int(np.count_nonzero(b)) - tp
    return tp, fp, fn, a.size - tp - fp - fn


def compute_IoU(ground_truth, label):
    """reference :160-194 for two host arrays -> [iou, accuracy, precision, recall]"""
    return ratios(*pixel_counts(ground_truth, label))


def pair_stats(labels, pairs=PAIRS):
    """labels[B,L,H,W] u8 on the device -> per sample, per pair (a, b): compute_IoU(plane a, plane b), from one launch"""
    from autoposeestimation_amd import engine as E
    counts = E.label_pair_counts(labels, pairs).cpu().tolist()
    return [[ratios(*c) for c in sample] for sample in counts]


def _decode(path):
    """the reference's own read (:60-63): whatever the PNG's mode, through RGB, channel 0"""
    return np.array(Image.open(path).convert("RGB"), dtype=np.uint8)[:, :, 0]


def _sample_paths(root, cls, rot, sample):
    lab = os.path.join(root, "label_generator", "data", cls, rot)
    return {"gt": os.path.join(root, "experiments", "data", "gt_test", cls, rot, "{}{}".format(sample, TAG)),
            "new_pred": os.path.join(lab, "{}.new_pred.label.png".format(sample)),
            "pred": os.path.join(lab, "{}.pred.label.png".format(sample)),
            "gen": os.path.join(lab, "{}.gen.label.png".format(sample)),
            "image": os.path.join(root, "data_generation", "data", cls, rot, "{}.color.png".format(sample))}


def _load(job):
    """decode one sample on a host thread -> (planes u8 [4,H,W], image u8 [H,W,3] or None, seconds)"""
    paths, with_image = job
    t0 = time.perf_counter()
    planes = [_decode(paths[k]) for k in PLANES]
    image = np.array(Image.open(paths["image"]).convert("RGB"), dtype=np.uint8) if with_image else None
    shapes = {p.shape for p in planes} | ({image.shape[:2]} if with_image else set())
    if len(shapes) != 1:
        raise ValueError("sample {}: its images differ in size: {}".format(paths["gt"], sorted(shapes)))
    return np.stack(planes), image, time.perf_counter() - t0


def _blend_host(image, planes, first, second):
    """the comparison image of :105-120 in numpy"""
    added = image.copy()
    for plane, ch in (first, second):
        lab = planes[plane]
        m = lab != 0
        added[:, :, ch][m] = added[:, :, ch][m] * C0 + lab[m] * C1
    return added


def _score_batch(items, device, overlay_dir):
    """items: [(cls, rot, sample, paths, planes, image)] of one size -> per item the five ratio lists; writes the overlays"""
    if device is not None:
        import torch
        from autoposeestimation_amd import engine as E
        labels = torch.from_numpy(np.stack([it[4] for it in items])).to(device)
        counts = E.label_pair_counts(labels, PAIRS).cpu().tolist()
    else:
        counts = [[pixel_counts(it[4][a], it[4][b]) for a, b in PAIRS] for it in items]
    out = []
    for it, sample_counts in zip(items, counts):
        try:
            out.append([ratios(*c) for c in sample_counts])
        except ZeroDivisionError:
            raise ZeroDivisionError("sample {}: a label pair has no foreground to divide by (counts tp, fp, fn, tn per pair: {})".format(
                it[3]["gt"], [tuple(int(v) for v in c) for c in sample_counts])) from None
    if overlay_dir is not None:
        if device is not None:
            rgb = torch.from_numpy(np.stack([it[5] for it in items])).to(device)
            painted = [E.label_pair_blend(rgb, labels, (pa, CH_PRED), (pb, CH_OTHER), C0, C1).cpu().numpy() for _, pa, pb in OVERLAYS]
        else:
            painted = [[_blend_host(it[5], it[4], (pa, CH_PRED), (pb, CH_OTHER)) for it in items] for _, pa, pb in OVERLAYS]
        for k, (tag, _, _) in enumerate(OVERLAYS):
            for i, it in enumerate(items):
                d = os.path.join(overlay_dir, it[0], it[1])
                os.makedirs(d, exist_ok=True)
                Image.fromarray(painted[k][i]).save(os.path.join(d, "{}.{}.png".format(it[2], tag)))
    return out


def main(root, classes=None, rotations=("foreground", "foreground180"), batch=32, use_cuda=True, overlay_dir=None, timing=None):
    """reference :9-156 over `<root>/experiments/data/gt_test/<cls>/<rot>/<id>.color.mask.0.png`,
    `<root>/label_generator/data/<cls>/<rot>/<id>.{new_pred,pred,gen}.label.png` and `<root>/data_generation/data/<cls>/<rot>/<id>.color.png`.

    Prints the reference's lines -- `classes`, `cls i/n, rot j/m` and after every directory the five cumulative rows -- and returns what
    it only prints: {"per_sample": one entry per sample with the five ratio lists, "directories": the unrounded cumulative means and
    IoU >= 0.5 shares after every directory, "final": the last of those, "order": the (cls, rot, id) walked}.

    `classes=None`: the directories of gt_test in sorted order (the reference takes os.listdir's order, which is arbitrary); samples are
    walked in sorted order.  The images are decoded on host threads, grouped into batches of up to `batch` samples of one size and scored
    by one launch per batch; `use_cuda=False` scores them with numpy on the host instead.  The colour frame is only read for
    `overlay_dir`, which receives `<cls>/<rot>/<id>.pred_vs_new_pred.png` and `<id>.pred_vs_gen.png` (pred into channel 2, the other label
    into channel 0, c0 = 0.7).  A sample whose label pair has nothing to divide by raises ZeroDivisionError naming the sample, as the
    reference does without the name; labels of different sizes within a sample raise ValueError.  `timing` (a dict) receives the
    seconds spent in all and in decoding, and the sample count."""
    from autoposeestimation_amd import sharding
    device = None
    if use_cuda:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("gt_test.main(use_cuda=True) needs the GPU; use_cuda=False is the numpy path")
        device = torch.device("cuda:0")
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    t_start, t_decode = time.perf_counter(), 0.0
    gt_path = os.path.join(root, "experiments", "data", "gt_test")
    if classes is None:
        classes = sorted(d for d in os.listdir(gt_path) if os.path.isdir(os.path.join(gt_path, d)))
    classes, rotations = list(classes), list(rotations)
    print("classes", classes)
    per_pair = [[] for _ in NAMES]
    hits = [0] * len(NAMES)
    per_sample, directories, order = [], [], []
    for i, cls in enumerate(classes):
        for j, rot in enumerate(rotations):
            print("cls {}/{}, rot {}/{}".format(i + 1, len(classes), j + 1, len(rotations)))
            samples = sorted(s[:-len(TAG)] for s in os.listdir(os.path.join(gt_path, cls, rot)) if TAG in s)
            jobs = [(_sample_paths(root, cls, rot, s), overlay_dir is not None) for s in samples]
            pending = []

            def flush():
                for it, five in zip(pending, _score_batch(pending, device, overlay_dir)):
                    for k, r in enumerate(five):
                        per_pair[k].append(r)
                        hits[k] += r[0] >= 0.5
                    per_sample.append(dict(zip(NAMES, five), cls=it[0], rot=it[1], sample=it[2]))
                    order.append((it[0], it[1], it[2]))
                del pending[:]

            for (planes, image, dt), s, job in zip(sharding.prefetched(jobs, _load, workers=8, window=2 * batch), samples, jobs):
                t_decode += dt
                if pending and (len(pending) >= batch or pending[-1][4].shape != planes.shape):
                    flush()
                pending.append((cls, rot, s, job[0], planes, image))
            if pending:
                flush()
            total = len(order)
            if total == 0:
                raise ZeroDivisionError("no sample up to {}/{}: nothing to average".format(cls, rot))
            means = [np.mean(np.array(v), axis=0) for v in per_pair]
            shares = [h / total for h in hits]
            for line, m, sh in zip(LINES, means, shares):
                print(line.format(*np.round(m, 4), np.round(sh, 4)))
            directories.append({"cls": cls, "rot": rot, "samples": len(samples), "total_samples": total,
                                "mean": {n: [float(x) for x in m] for n, m in zip(NAMES, means)},
                                "iou_ge_0.5": {n: float(sh) for n, sh in zip(NAMES, shares)}})
    if timing is not None:
        timing.update(seconds=time.perf_counter() - t_start, decode_seconds=t_decode, samples=len(order))
    return {"per_sample": per_sample, "directories": directories, "final": directories[-1] if directories else None, "order": order}

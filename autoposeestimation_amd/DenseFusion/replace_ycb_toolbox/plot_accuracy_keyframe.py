"""Drop-in for DenseFusion/replace_ycb_toolbox/plot_accuracy_keyframe.m (:31-56, :71-84, :150-170): per class and over all objects, per pose
source, the area under the accuracy-threshold curve (AUC) and the share of objects below 2 cm, of `distances_sys` (ADD-S) and of
`distances_non` (ADD).  The figures themselves are not drawn; the numbers are the ones their legends carry, as fractions.

As the toolbox: distances strictly above `max_distance` become inf (exactly `max_distance` stays); n counts every row, inf and NaN
included; `< 0.02` is strict; VOCap keeps the finite values, pads the recall with 0 and 0.1 and the precision with 0 and its last value,
takes the running maximum of the precision and adds (recall step) x (precision) over the positions where the recall CHANGES -- among
equal distances the first one's precision counts -- times 10.  The sort, the running maximum and the steps are torch float64 operations on
whatever device the distances are on (a CPU tensor too); the final sum over the steps is the correctly rounded one (math.fsum).

Departures.  An empty finite set is an index error in MATLAB (`prec(end)`); here the AUC is 0.  The toolbox falls back to ALL objects for a
class without an instance (`if isempty(index)`), which is also how its 22nd entry, "All 21 objects", gets its rows; here a class without an
instance gives NaN in its four figures, and "All 21 objects" stays all objects."""
import math

import torch

INDEX_PLOT = (2, 3, 1, 5)                     # the toolbox's columns, 1-based, in legend order
LEGEND = ("iterative", "PoseCNN+ICP", "per-pixel", "3DCoordinate", "3D")       # `leng`, by column
ALL = "All 21 objects"


def accuracy_curve(D, max_distance=None):
    """:41-46 -> (d sorted ascending with inf and NaN last, accuracy = (1..n) / n)"""
    D = torch.as_tensor(D, dtype=torch.float64).reshape(-1)
    if max_distance is not None:
        D = torch.where(D > max_distance, torch.full_like(D, float("inf")), D)
    d = torch.sort(D).values
    n = d.numel()
    return d, torch.arange(1, n + 1, dtype=torch.float64, device=d.device) / n


def VOCap(rec, prec):
    """:150-170"""
    index = torch.isfinite(rec)
    rec, prec = rec[index], prec[index]
    if rec.numel() == 0:
        return 0.0
    zero = rec.new_zeros(1)
    mrec = torch.cat([zero, rec, rec.new_full((1,), 0.1)])
    mpre = torch.cummax(torch.cat([zero, prec, prec[-1:]]), dim=0).values
    i = torch.nonzero(mrec[1:] != mrec[:-1]).reshape(-1) + 1
    return math.fsum(((mrec[i] - mrec[i - 1]) * mpre[i]).tolist()) * 10


def _figures(D, max_distance):
    d, accuracy = accuracy_curve(D, max_distance)
    n = d.numel()
    c = int((d < 0.02).sum())
    return VOCap(d, accuracy), c / n, (d, accuracy)


def plot_accuracy_keyframe(results, classes, max_distance=0.1, curves=False):
    """results: the dict evaluate_poses_keyframe returns (or loadmat of its file); classes: the class names, class k (1-based) is
    classes[k - 1] -> {class name | "All 21 objects": {column (1-based, of INDEX_PLOT): {"auc_sys", "lt2cm_sys", "auc_non", "lt2cm_non"}}};
    curves: also "curve_sys", "curve_non", "curve_rotation", "curve_translation" as (sorted values, accuracy)"""
    as64 = lambda a: torch.as_tensor(a, dtype=torch.float64)  # noqa: E731
    sys_, non, rot, tra = (as64(results[k]) for k in ("distances_sys", "distances_non", "errors_rotation", "errors_translation"))
    cls_ids = as64(results["results_cls_id"]).reshape(-1).to(sys_.device)
    out = {}
    for k, name in enumerate(list(classes) + [ALL]):
        index = torch.arange(cls_ids.numel(), device=sys_.device) if name == ALL and k == len(classes) else torch.nonzero(cls_ids == k + 1).reshape(-1)
        out[name] = {}
        for col in INDEX_PLOT:
            if index.numel() == 0:
                out[name][col] = {key: float("nan") for key in ("auc_sys", "lt2cm_sys", "auc_non", "lt2cm_non")}
                continue
            auc_s, lt_s, cur_s = _figures(sys_[index, col - 1], max_distance)
            auc_n, lt_n, cur_n = _figures(non[index, col - 1], max_distance)
            entry = {"auc_sys": auc_s, "lt2cm_sys": lt_s, "auc_non": auc_n, "lt2cm_non": lt_n}
            if curves:
                entry.update(curve_sys=cur_s, curve_non=cur_n, curve_rotation=accuracy_curve(rot[index, col - 1]),
                             curve_translation=accuracy_curve(tra[index, col - 1], max_distance))
            out[name][col] = entry
    return out


def legend_table(figures):
    """the lines of the figures' legends (:54, :82): per class one line per measure"""
    lines = []
    for name, cols in figures.items():
        for key, title in (("sys", "symmetry"), ("non", "non-symmetry")):
            lines.append("%s (%s): %s" % (name, title, " ".join("%s(AUC:%.2f)(<2cm:%.2f)" % (LEGEND[col - 1], e["auc_" + key] * 100, e["lt2cm_" + key] * 100)
                                                               for col, e in cols.items())))
    return lines

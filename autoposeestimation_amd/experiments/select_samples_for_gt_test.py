"""The reference's sample drawer for the label-quality test (experiments/select_samples_for_gt_test.py): per `<cls>_<rot>` a shuffled
list of the colour frames under `<root>/data_generation/data/<cls>/<rot>`, kept in `<root>/experiments/data/gt_test/meta.json` and
reused by later runs, and the first int(len * p) frames of each list re-saved as RGB PNG under `gt_test/<cls>/<rot>/` for annotation."""
import json
import os

import numpy as np
from PIL import Image

ROTATIONS = ("foreground", "foreground180")


def main(root, p=0.2, classes=None, rng=None):
    """reference :9-51.  `classes=None`: the directories of data_generation/data in sorted order (the reference takes os.listdir's
    order, which is arbitrary, and the shuffles consume one generator in that order).  `rng=None` shuffles with `np.random` as the
    reference does; a `np.random.RandomState` may be passed instead.  An existing meta.json keeps its `p` and its lists.  Returns meta."""
    path = os.path.join(root, "data_generation", "data")
    if classes is None:
        classes = sorted(d for d in os.listdir(path) if os.path.isdir(os.path.join(path, d)))
    classes = list(classes)
    rng = np.random if rng is None else rng
    gt_path = os.path.join(root, "experiments", "data", "gt_test")
    os.makedirs(gt_path, exist_ok=True)
    json_path = os.path.join(gt_path, "meta.json")
    if not os.path.exists(json_path):
        meta = {"p": p}
    else:
        with open(json_path) as f:
            meta = json.load(f)
    for i, cls in enumerate(classes):
        for j, rot in enumerate(ROTATIONS):
            print("cls {}/{}, rot {}/{}".format(i, len(classes), j, len(ROTATIONS)))
            rot_path = os.path.join(path, cls, rot)
            name = "{}_{}".format(cls, rot)
            if name not in meta:
                samples = np.array([s for s in sorted(os.listdir(rot_path)) if ".color.png" in s])
                rng.shuffle(samples)
                meta[name] = [str(s) for s in samples]
            save_path = os.path.join(gt_path, cls, rot)
            os.makedirs(save_path, exist_ok=True)
            n = int(len(meta[name]) * meta["p"])
            for sample in meta[name][:n]:
                with open(os.path.join(rot_path, sample), "rb") as f:
                    x = Image.open(f).convert("RGB")
                x.save(os.path.join(save_path, sample))
    with open(json_path, "w") as f:
        json.dump(meta, f)
    return meta

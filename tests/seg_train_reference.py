"""Shared pieces of the segmentor training-sample tests (test infrastructure): the host Pillow path of the package on arrays, synthetic
samples, and the reader of tests/golden/seg_train.npz (made by tools/gen_golden_seg_train.py by running the reference)."""
import os

import numpy as np
from PIL import Image

GOLDEN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seg_train.npz")
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def golden():
    return np.load(GOLDEN_PATH)


def crop_and_zoom(g, name):
    """the package's CropAndZoom set up as the golden case's reference instance was"""
    from autoposeestimation_amd.segmentation.utils import CropAndZoom
    cz = CropAndZoom(output_size=int(g["output_size"]))
    cz.min_l, cz.max_l = [int(v) for v in g["%s_lims" % name]]
    return cz


def pillow_sample(rgb, label, params, crop, class_id, mean=MEAN, std=STD):
    """segmentation/utils.py's transforms on one sample with given parameters (box included) -> img[3,S,S] f32, label[S,S] i64 (numpy)"""
    from autoposeestimation_amd.segmentation import utils as U
    data = U.colorJitter()([Image.fromarray(rgb, "RGB"), Image.fromarray(label, "L")], ops=params.get("ops") or [])
    if params.get("angle") is not None:
        data = U.rotate()(data, angle=params["angle"])
    img, lab = crop(data, box=params["box"])
    lab = np.array(lab)
    lab[lab != 0] = class_id
    img, lab = U.normalize(mean, std)(U.toTensor()([img, lab]))
    return img.numpy(), lab.numpy()


def normalise(u8, mean=MEAN, std=STD):
    """ToTensor + Normalize of an [H,W,3] u8 image -> [3,H,W] f32"""
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return (x - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]


def synthetic_sample(rng, h, w, shape="ellipse"):
    """random-noise frame (every filter tap matters) and a label with an object of the given shape, holes included"""
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = rng.uniform(0.35, 0.65) * h, rng.uniform(0.35, 0.65) * w
    ry, rx = {"ellipse": (0.2, 0.2), "tall": (0.4, 0.06), "wide": (0.08, 0.4)}[shape]
    label = np.where(((yy - cy) / (ry * h)) ** 2 + ((xx - cx) / (rx * w)) ** 2 <= 1.0, 255, 0).astype(np.uint8)
    label[::5, ::7] = 0
    label[int(cy), int(cx)] = 255
    return rgb, label


def write_tree(root, name, train, test, classes):
    """the reference's tree under `root`: train / test = lists of (entry, rgb, label)"""
    set_dir = os.path.join(root, "label_generator", "data_sets", "segmentation", name)
    os.makedirs(set_dir, exist_ok=True)
    for mode, items in (("train", train), ("test", test)):
        with open(os.path.join(set_dir, "%s_data_list.txt" % mode), "w") as f:
            f.write("".join(e + "\n" for e, _, _ in items))
        for e, rgb, label in items:
            for base, arr, suffix, m in ((os.path.join(root, "data_generation", "data"), rgb, ".color.png", "RGB"),
                                         (os.path.join(root, "label_generator", "data"), label, ".pred.label.png", "L")):
                os.makedirs(os.path.dirname(os.path.join(base, e)), exist_ok=True)
                Image.fromarray(arr, m).save(os.path.join(base, e + suffix))
    with open(os.path.join(set_dir, "classes.txt"), "w") as f:
        f.write("".join(c + "\n" for c in classes))

"""Generate tests/golden/seg_train.npz by RUNNING the reference's segmentation.utils.CropAndZoom and rotate (imported from the reference
tree through tools/ref_shim.py) on small synthetic samples.  Build container only.  Only data goes into the file: inputs, seeds, the
recorded crop boxes and the outputs.

CropAndZoom needs numpy, `random` and PIL only.  Its instance gets output_size = 48 and, per case, (min_l, max_l): (24, 48) -- the
reference's own relation max_l = output_size, min_l = output_size / max_zoom -- for the cases whose box fits, and (50, 64) for the "too big"
cases: with max_l = output_size the drawn side is always below the frame's 48 rows, so the `size[0] - 2` route is only reachable with a
larger draw (the crop it then takes has 46 rows: still an enlargement).  The box handed to `Image.crop` is recorded by wrapping
Image.Image.crop for the duration of the call; the route a case took is recorded from the number of get_bbox calls and from whether
np.random.randint was called, and asserted to be the one the case is meant to reach.

rotate: `transforms.functional.rotate(img, angle)` (torchvision is not installed) -> img.rotate(angle), its documented PIL path with default
arguments, set on the instance's `rotation` attribute."""
import os
import random
import sys

import numpy as np
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools import ref_shim  # noqa: E402

H, W, OUT = 48, 64, 48
FITS, BIG = (24, 48), (50, 64)
# name, object rows [r0, r1], columns [c0, c1] (inclusive), (min_l, max_l), expected route (square, too_big)
CASES = [
    ("square_fits", (14, 34), (22, 42), FITS, (True, False)),
    ("square_too_big", (14, 34), (22, 42), BIG, (True, True)),
    ("tall", (4, 44), (28, 36), FITS, (False, False)),
    ("tall_too_big", (4, 44), (28, 36), BIG, (False, True)),
    ("wide", (20, 28), (6, 58), FITS, (False, False)),
    ("wide_too_big", (20, 28), (6, 58), BIG, (False, True)),
    ("touch_top", (0, 12), (20, 33), FITS, (True, False)),
    ("touch_bottom", (35, 47), (20, 33), FITS, (True, False)),
    ("touch_left", (18, 30), (0, 12), FITS, (True, False)),
    ("touch_right", (18, 30), (51, 63), FITS, (True, False)),
]


def main():
    ref_shim.install()
    import segmentation.utils as ref

    rng = np.random.default_rng(20)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    out = {"rgb": rgb, "names": np.array([c[0] for c in CASES]), "output_size": np.int64(OUT)}
    for n, (name, (r0, r1), (c0, c1), (min_l, max_l), route) in enumerate(CASES):
        label = np.zeros((H, W), np.uint8)
        label[r0:r1 + 1, c0:c1 + 1] = 255
        label[r0 + 2:r1 - 1:3, c0 + 2:c1 - 1:3] = 0                      # holes: NEAREST has something to pick between
        cz = ref.CropAndZoom()
        cz.output_size, cz.min_l, cz.max_l = OUT, min_l, max_l
        boxes, sides, randints = [], [], []
        crop0, get_bbox0, randint0 = Image.Image.crop, cz.get_bbox, np.random.randint

        def crop(self, box=None):
            boxes.append([int(v) for v in box])
            return crop0(self, box)

        def get_bbox(c, l):  # noqa: E741
            sides.append(l)
            return get_bbox0(c, l)

        def randint(*a, **k):
            v = randint0(*a, **k)
            randints.append(int(v))
            return v

        seed = 100 + n
        random.seed(seed)
        np.random.seed(seed)
        Image.Image.crop, cz.get_bbox, np.random.randint = crop, get_bbox, randint
        try:
            img_o, lab_o = cz([Image.fromarray(rgb, "RGB"), Image.fromarray(label, "L")])
        finally:
            Image.Image.crop, np.random.randint = crop0, randint0
        h, w = r1 - r0, c1 - c0
        square = 0.8 <= (h / OUT) / (w / OUT) <= 1.2
        too_big = len(sides) == (3 if square else 4)                     # calls of get_bbox: 2 / 3 (square), 3 / 4 (not square)
        assert len(sides) in ((2, 3) if square else (3, 4)) and (not too_big or sides[-1] == H - 2), (name, sides)
        assert (square, too_big) == route, (name, square, too_big, sides)
        assert (len(randints) == 1) == (too_big or not square), (name, randints)
        assert boxes[0] == boxes[1] and len(boxes) == 2
        out.update({"%s_label" % name: label, "%s_seed" % name: np.int64(seed), "%s_lims" % name: np.array([min_l, max_l], np.int64),
                    "%s_box" % name: np.array(boxes[0], np.int64), "%s_img_out" % name: np.array(img_o), "%s_label_out" % name: np.array(lab_o)})
        print(name, "box", boxes[0], "randint", randints)
    # one rotate result
    rot = ref.rotate()
    rot.rotation = lambda img, angle: img.rotate(angle)
    label = np.zeros((H, W), np.uint8)
    label[10:30, 15:50] = 255
    random.seed(7)
    uniform0, angles = random.uniform, []

    def uniform(a, b):
        angles.append(uniform0(a, b))
        return angles[-1]

    random.uniform = uniform
    try:
        img_o, lab_o = rot([Image.fromarray(rgb, "RGB"), Image.fromarray(label, "L")])
    finally:
        random.uniform = uniform0
    out.update({"rotate_label": label, "rotate_seed": np.int64(7), "rotate_angle": np.float64(angles[0]), "rotate_img_out": np.array(img_o),
                "rotate_label_out": np.array(lab_o)})
    path = os.path.join(REPO, "tests", "golden", "seg_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

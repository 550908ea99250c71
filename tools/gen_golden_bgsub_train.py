"""Generate tests/golden/bgsub_train.npz by RUNNING the reference's background_subtraction.utils.load_subtraction / IoU_cca and
background_subtraction.dataset.SegmentationDataset (imported from the reference tree through tools/ref_shim.py) on small synthetic
trees.  Build container only.  Only data goes into the file: frames, seeds, parameters, recorded results.

What stands in for what (nothing here is copied reference code; torchvision and OpenCV are not installed):
  * transforms.functional.rotate(img, angle) -> img.rotate(angle), hflip / vflip -> Image.transpose(FLIP_LEFT_RIGHT / FLIP_TOP_BOTTOM):
    their documented PIL paths with default arguments, on the installed Pillow;
  * transforms.Resize(size) -> the image itself when it already has that size (what Pillow's resize returns then), else Pillow's bilinear
    resize; the reference's dataset hard-codes Resize([480, 640]): for the small frames of the fixture its `Resize` attribute is replaced
    after construction by Resize([h, w]) of the frames, so the step stays the identity it is for the reference's 480 x 640 frames;
  * transforms.ColorJitter(b, c, s, h) -> the package's ColorJitterPIL (restates torchvision 0.6.1's PIL path), wrapped to record the
    drawn op lists;
  * transforms.ToTensor / Normalize -> their documented definitions (HWC uint8 -> CHW float32 / 255; (x - mean) / std per channel);
  * cv2.connectedComponents -> scipy.ndimage.label with the 8-neighbourhood;
  * np.float -> float (alias removed from numpy; tools/ref_shim.py).
"""
import os
import random
import sys
import tempfile

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from tools import ref_shim  # noqa: E402
from tools.gen_golden_bgsub import _Normalize, _ToTensor  # noqa: E402

MEAN = [0.040278014, 0.04060352, 0.038310923, 0.0381776, 0.03656849, 0.03636289, 0.03556486]
STD = [0.059689723, 0.05965291, 0.056203008, 0.05619316, 0.054657422, 0.054514673, 0.05377024]
OPS = ["brightness", "contrast", "saturation", "hue"]


class _Resize:
    def __init__(self, size):
        self.size = tuple(size)

    def __call__(self, img):
        h, w = self.size
        return img if img.size == (w, h) else img.resize((w, h), Image.Resampling.BILINEAR)


def write_tree(root, key, frames_list):
    for sub in ("background", "foreground", "groundtruth"):
        os.makedirs(os.path.join(root, key, sub), exist_ok=True)
    for i, (f_rgb, b_rgb, f_depth, b_depth, label) in enumerate(frames_list):
        Image.fromarray(f_rgb, "RGB").save(os.path.join(root, key, "foreground", "img%06d.png" % i))
        Image.fromarray(b_rgb, "RGB").save(os.path.join(root, key, "background", "img%06d.png" % i))
        Image.fromarray(f_depth).save(os.path.join(root, key, "foreground", "depth%06d.png" % i))
        Image.fromarray(b_depth).save(os.path.join(root, key, "background", "depth%06d.png" % i))
        Image.fromarray(label, "L").save(os.path.join(root, key, "groundtruth", "img%06d.mask.0.png" % i))


def main():
    ref_shim.install()
    import scipy.ndimage as ndi
    import background_subtraction.utils as ref
    from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented.dataset import ColorJitterPIL
    import bgsub_train_reference as R

    drawn = []

    class _Jitter(ColorJitterPIL):
        def __call__(self, img):
            ops = self.params()
            drawn.append(ops)
            return self.apply(img, ops)

    tf = ref.transforms
    tf.ToTensor, tf.Normalize, tf.Resize, tf.ColorJitter = _ToTensor, _Normalize, _Resize, _Jitter
    tf.functional.rotate = lambda img, angle: img.rotate(angle)
    tf.functional.hflip = lambda img: img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    tf.functional.vflip = lambda img: img.transpose(Image.Transpose.FLIP_TOP_BOTTOM)

    def connected_components(mask, connectivity=8):
        assert connectivity == 8
        labels, n = ndi.label(mask != 0, structure=np.ones((3, 3), dtype=bool))
        return n + 1, labels.astype(np.int32)

    ref.cv2.connectedComponents = connected_components
    import background_subtraction.dataset as refds

    rng = np.random.default_rng(20261016)
    out = {"mean": np.asarray(MEAN, np.float32), "std": np.asarray(STD, np.float32)}
    sets = {"a": [R.synthetic_frames(rng, 48, 64) for _ in range(2)],          # 48 x 64
            "b": [R.synthetic_frames(rng, 37, 53) for _ in range(2)],          # odd, non-square
            "c": [R.synthetic_frames(rng, 40, 40) for _ in range(1)]}          # square: 90 / 270 degrees are transposes
    # depth differences above 255 (the uint8 cast wraps) and zeros on either side are part of synthetic_frames; make sure of it
    fa = sets["a"][0]
    assert (np.abs(fa[2].astype(int) - fa[3].astype(int)) > 255).any() and (fa[2] == 0).any() and (fa[3] == 0).any()
    for k, fl in sets.items():
        for j, name in enumerate(("f_rgb", "b_rgb", "f_depth", "b_depth", "label")):
            out["set_%s_%s" % (k, name)] = np.stack([f[j] for f in fl])

    with tempfile.TemporaryDirectory() as root:
        for k, fl in sets.items():
            write_tree(root, k, fl)
        rot, hf, vf = tf.functional.rotate, tf.functional.hflip, tf.functional.vflip
        cases = []          # (name, set, idx, fixed angle or None, kwargs)

        def run(name, key, idx, seed, fixed_angle=None, **kw):
            """one call of the reference's load_subtraction; fixed_angle replaces the drawn angle inside the rotate callable"""
            if fixed_angle is not None:
                kw["rotate"] = lambda img, angle: img.rotate(fixed_angle)
            random.seed(seed)
            np.random.seed(seed)
            del drawn[:]
            x, y = ref.load_subtraction(root, key, idx, **kw)
            assert x.dtype == np.uint8 and x.shape[2] == 7
            out["case_%s_x" % name] = x
            out["case_%s_y" % name] = (y != 0).astype(np.uint8)
            cases.append(name)
            # what the case asked for, as data: set, index, seed, rotate, jitter (0 none, 1 = (0.05, 0.05, 0.05, 0.02), 2 = (0.2, 0.2, 0.2,
            # 0.05)), hflip, vflip, fixed angle (NaN = the drawn one)
            out["case_%s_meta" % name] = np.array([ord(key), idx, seed, int("rotate" in kw), {None: 0, "weak": 1, "strong": 2}[getattr(kw.get("colorJitter"), "tag", None)], int("hflip" in kw),
                                                   int("vflip" in kw), np.nan if fixed_angle is None else fixed_angle], np.float64)
            return [list(o) for o in drawn]

        jit = _Jitter(brightness=0.05, contrast=0.05, saturation=0.05, hue=0.02)
        strong = _Jitter(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.05)
        jit.tag, strong.tag = "weak", "strong"
        run("plain", "a", 0, 1)
        run("plain_odd", "b", 1, 1)
        run("rotate", "a", 0, 2, rotate=rot)
        run("rotate_odd", "b", 0, 3, rotate=rot)
        for s in (4, 5, 6, 7):                  # both outcomes of each flip draw must occur
            run("hflip%d" % s, "a", 1, s, hflip=hf)
            run("vflip%d" % s, "a", 1, s, vflip=vf)
        run("jitter", "a", 0, 8, colorJitter=jit)
        run("jitter_strong", "b", 0, 9, colorJitter=strong)
        for tag, ang in (("0", 0.0), ("180", 180.0), ("m180", -180.0), ("90", 90.0), ("1em3", 1e-3), ("m90", -90.0), ("45", 45.0)):
            run("angle_" + tag, "a", 0, 10, fixed_angle=ang)
            run("angle_odd_" + tag, "b", 1, 10, fixed_angle=ang)
        for tag, ang in (("90", 90.0), ("270", 270.0), ("m90", -90.0), ("33", 33.0)):
            run("angle_sq_" + tag, "c", 0, 10, fixed_angle=ang)
        # everything together: seeds chosen so that every order of the four ops and both outcomes of both flips occur
        orders, flips, seed, kept = set(), set(), 100, []
        while len(orders) < 24 or len(flips) < 4:
            random.seed(seed)
            np.random.seed(seed)
            random.uniform(-180, 180)
            fl = (bool(np.random.rand() > 0.5), bool(np.random.rand() > 0.5))
            new = {tuple(n for n, _ in (strong if seed % 2 else jit).params()) for _ in range(2)}
            if not new <= orders or fl not in flips:
                got = run("all%d" % seed, "b", seed % 2, seed, rotate=rot, colorJitter=strong if seed % 2 else jit, hflip=hf, vflip=vf)
                assert {tuple(n for n, _ in o) for o in got} == new
                orders |= new
                flips.add(fl)
                kept.append(seed)
            seed += 1
        assert len(orders) == 24 and len(flips) == 4
        print("all-together seeds:", kept)
        out["cases"] = np.array(cases)

        # SegmentationDataset.__getitem__: two classes x two samples of the odd size, train mode, seeded
        dsroot = os.path.join(root, "ds")
        os.makedirs(dsroot)
        ds_sets = {"k0": sets["b"], "k1": [R.synthetic_frames(rng, 37, 53) for _ in range(2)]}
        for k, fl in ds_sets.items():
            write_tree(dsroot, k, fl)
            for j, name in enumerate(("f_rgb", "b_rgb", "f_depth", "b_depth", "label")):
                out["ds_%s_%s" % (k, name)] = np.stack([f[j] for f in fl])
        ds = refds.SegmentationDataset("train", dsroot, {"k0": [0, 1], "k1": [0, 1]}, ["k0", "k1"], mean=MEAN, std=STD)
        ds.Resize = _Resize([37, 53])
        items = []
        for seed in (1, 2, 3):
            random.seed(seed)
            np.random.seed(seed)
            for index in (0, 3, 2):             # consecutive draws from one seeding
                x, y = ds[index]
                assert x.dtype == torch.float32 and y.dtype == torch.int64
                out["item_%d_%d_x" % (seed, index)] = x.numpy()
                out["item_%d_%d_y" % (seed, index)] = y.numpy().astype(np.uint8)
                items.append((seed, index))
        out["items"] = np.array(items)
        dt = refds.SegmentationDataset("test", dsroot, {"k1": [0, 1]}, ["k0", "k1"], mean=MEAN, std=STD)
        dt.Resize = _Resize([37, 53])
        x, y = dt[1]                            # the key comes from `classes`: k0, sample 1
        out["item_test_1_x"], out["item_test_1_y"] = x.numpy(), y.numpy().astype(np.uint8)

        # mean=None statistics: 23 samples of one class, 16 x 24
        st = [R.synthetic_frames(rng, 16, 24) for _ in range(23)]
        write_tree(os.path.join(root, "st"), "s0", st)
        for j, name in enumerate(("f_rgb", "b_rgb", "f_depth", "b_depth", "label")):
            out["stat_%s" % name] = np.stack([f[j] for f in st])
        dm = refds.SegmentationDataset("test", os.path.join(root, "st"), {"s0": list(range(23))}, ["s0"], mean=None, std=None)
        out["stat_mean"], out["stat_std"] = np.array(dm.mean, np.float32), np.array(dm.std, np.float32)
        assert np.array_equal(out["stat_mean"], np.array(dm.mean)) and out["stat_mean"].shape == (7,)

    # IoU_cca: K = 2 with several blobs, exact ties, an empty prediction; K = 3 (non-zero labels merge)
    h, w = 48, 64
    p = np.zeros((4, 2, h, w), np.float32)
    for i in range(4):
        fg = rng.random((h, w)).astype(np.float32) * 0.35
        fg[5:20, 6:30] += 0.6
        fg[28:44, 34:60] += 0.55 + 0.03 * i
        fg[40:46, 2:9] += 0.7
        p[i, 1], p[i, 0] = np.clip(fg, 0, 1), 1 - np.clip(fg, 0, 1)
    p[2, 0], p[2, 1] = 1.0, 0.0                                 # empty prediction
    p[3, 0], p[3, 1] = 1.0, 0.0
    p[3, 1, 4:10, 4:10] = 3.0                                   # two identical blobs: the first in raster order wins
    p[3, 1, 30:36, 40:46] = 3.0
    t = np.zeros((4, h, w), np.int64)
    t[:, 26:46, 30:62] = 1
    t[3, 2:12, 2:12] = 1
    p3 = rng.random((2, 3, h, w)).astype(np.float32)
    p3[:, 0] += 0.45
    t3 = rng.integers(0, 2, (2, h, w)).astype(np.int64)
    for tag, pp, tt, k in (("k2", p, t, 2), ("k3", p3, t3, 3)):
        m = ref.IoU_cca(num_classes=k)
        half = len(pp) // 2                                     # two adds: the counts accumulate
        m.add(torch.from_numpy(pp[:half]), torch.from_numpy(tt[:half]))
        m.add(torch.from_numpy(pp[half:]), torch.from_numpy(tt[half:]))
        iou, miou = m.value()
        out["cca_%s_pred" % tag], out["cca_%s_target" % tag] = pp, tt.astype(np.uint8)
        out["cca_%s_conf" % tag] = m.conf_metric.value().astype(np.int64)
        out["cca_%s_iou" % tag], out["cca_%s_miou" % tag] = np.asarray(iou, np.float64), np.float64(miou)
    out["pillow_version"] = np.array(Image.__version__)
    path = os.path.join(REPO, "tests", "golden", "bgsub_train.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()

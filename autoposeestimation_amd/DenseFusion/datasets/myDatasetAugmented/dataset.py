"""Drop-in for DenseFusion/datasets/myDatasetAugmented/dataset.py: `get_bbox` (reference :338-380) and `PoseDataset`
(`__init__` :24-155, `__getitem__` :158-326) in **test** mode (what experiments/eval.py:37 uses) and in **train** mode with the
reference's augmentation: viewpoint sub-selection (`p_viewpoints`), extra-data mixing (`p_extra_data`), colour jitter, a random in-plane
rotation of colour / label / depth with the matching camera rotation, and translation noise (`noise_trans`).

The sample tuple is the reference's: (points[N,3] f32, choose[1,N] i64, img[3,Hc,Wc] f32, target[M,3] f32, model_points[M,3] f32,
idx[1] i64[, intr dict, np_img in test mode]).

Two paths to a sample: `ds[i]` / `ds.sample_host(i, params)` is the reference's, through Pillow and numpy on the host; `ds.batch(indices)`
keeps the decoded frames on the GPU and builds the same samples there (augment.py, csrc/pose_train.hip), shaped as
`DataLoader(batch_size=1)` delivers them.

Random draws.  The reference draws from the GLOBAL `random` / `numpy.random` states (viewpoint shuffle :66, extra-data shuffle :93,
ColorJitter, `random.uniform(-180, 180)` :211, three `random.uniform` for the translation noise :250, `np.random.shuffle(c_mask)` :257,
`random.sample(dellist, ...)` :287).  With `reference_rng=True` this class makes exactly those calls in exactly that order, so seeding
both global generators reproduces the reference's sample stream (`tests/test_pose_dataset_golden.py`, fixture made by running the
reference's class, `tools/gen_golden_dataset.py`).  By default (`reference_rng=False`) every sample draws from its own
`numpy.random.Generator` seeded by `(seed, index, epoch-free)`, which makes `ds[i]` reproducible regardless of access order.

Colour jitter: torchvision (0.6.1 in the reference's README) is third-party and absent from the reference tree; `ColorJitterPIL`
restates its published PIL path (`transforms.ColorJitter.get_params` + `functional.adjust_{brightness,contrast,saturation,hue}`)
-- parity unpinned for the jitter itself, everything around it is pinned with the jitter injected (`trancolor=`).

Model clouds: this file's own `.xyz` parser (:121-137) drops the LAST CHARACTER of every line's z value (`readline()[1:-2]` then
`[:-1]`), unlike pipeline/utils.py:667-684; restated as is, because the training targets of the reference are built from it."""
import json
import os
import random

import numpy as np
import torch
from PIL import Image, ImageEnhance

from autoposeestimation_amd.data_generation import sample_io as io
from autoposeestimation_amd.DenseFusion.datasets import packed

border_list = [-1, 40, 80, 120, 160, 200, 240, 280, 320, 360, 400, 440, 480, 520, 560, 600, 640, 680]
img_width = 480
img_length = 640
_MEAN = np.array([0.485, 0.456, 0.406], np.float32)
_STD = np.array([0.229, 0.224, 0.225], np.float32)


def bbox_from_extents(r0, r1, c0, c1):
    """get_bbox's arithmetic (reference :345-380) from the extents of the mask: the first / last row and column that hold a pixel (what
    the device path reads back, augment.py).  The crop covers the extents: see the argument at the top of csrc/pose_train.hip."""
    rmin, rmax, cmin, cmax = int(r0), int(r1) + 1, int(c0), int(c1) + 1

    def up(v):
        for tt in range(len(border_list) - 1):
            if border_list[tt] < v < border_list[tt + 1]:
                return border_list[tt + 1]
        return v

    r_b, c_b = up(rmax - rmin), up(cmax - cmin)
    center = [int((rmin + rmax) / 2), int((cmin + cmax) / 2)]
    rmin, rmax = center[0] - int(r_b / 2), center[0] + int(r_b / 2)
    cmin, cmax = center[1] - int(c_b / 2), center[1] + int(c_b / 2)
    if rmin < 0:
        rmax, rmin = rmax - rmin, 0
    if cmin < 0:
        cmax, cmin = cmax - cmin, 0
    if rmax > img_width:
        rmin, rmax = rmin - (rmax - img_width), img_width
    if cmax > img_length:
        cmin, cmax = cmin - (cmax - img_length), img_length
    return rmin, rmax, cmin, cmax


def get_bbox(label):
    """reference :342-380 (host twin of the device kernel seg_bbox_kernel)"""
    rows = np.where(np.any(label, axis=1))[0]
    cols = np.where(np.any(label, axis=0))[0]
    return bbox_from_extents(rows[0], rows[-1], cols[0], cols[-1])


def read_xyz_dataset(path, to_meter=True):
    """the reference dataset's own `.xyz` parser (dataset.py:121-137), quirk included: `line[1:-2]` strips '[' and ']\\n', then
    `[:-1]` drops one more character -- the last digit of z"""
    pts = []
    with open(path) as f:
        while True:
            line = f.readline()[1:-2]
            if not line:
                break
            xyz = [float(v) / 1000 if to_meter else float(v) for v in line[:-1].split(" ") if v != ""]
            pts.append([xyz[0], xyz[1], xyz[2]])
    return np.array(pts)


class ColorJitterPIL:
    """torchvision 0.6.1 `transforms.ColorJitter(brightness, contrast, saturation, hue)` on PIL images (published algorithm: factors
    from `random.uniform`, the four adjustments in `random.shuffle`d order; brightness / contrast / saturation through
    `PIL.ImageEnhance`, hue as a uint8 shift of the H channel in HSV)."""

    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0):
        self.brightness = (max(0.0, 1 - brightness), 1 + brightness) if brightness else None
        self.contrast = (max(0.0, 1 - contrast), 1 + contrast) if contrast else None
        self.saturation = (max(0.0, 1 - saturation), 1 + saturation) if saturation else None
        self.hue = (-hue, hue) if hue else None

    @staticmethod
    def adjust_hue(img, hue_factor):
        mode = img.mode
        if mode in {"L", "1", "I", "F"}:
            return img
        h, s, v = img.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        np_h += np.uint8(int(hue_factor * 255) & 0xFF)           # `np.uint8(hue_factor * 255)` of the original: truncate, wrap mod 256
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert(mode)

    def params(self, uniform=random.uniform, shuffle=random.shuffle):
        ops = []
        if self.brightness is not None:
            ops.append(("brightness", uniform(*self.brightness)))
        if self.contrast is not None:
            ops.append(("contrast", uniform(*self.contrast)))
        if self.saturation is not None:
            ops.append(("saturation", uniform(*self.saturation)))
        if self.hue is not None:
            ops.append(("hue", uniform(*self.hue)))
        shuffle(ops)
        return ops

    @classmethod
    def apply(cls, img, ops):
        for name, f in ops:
            if name == "brightness":
                img = ImageEnhance.Brightness(img).enhance(f)
            elif name == "contrast":
                img = ImageEnhance.Contrast(img).enhance(f)
            elif name == "saturation":
                img = ImageEnhance.Color(img).enhance(f)
            else:
                img = cls.adjust_hue(img, f)
        return img

    def __call__(self, img, uniform=random.uniform, shuffle=random.shuffle):
        return self.apply(img, self.params(uniform, shuffle))


class _GlobalDraws:
    """the reference's generators: module-level `random` and `numpy.random`"""
    uniform = staticmethod(random.uniform)
    shuffle_list = staticmethod(random.shuffle)
    shuffle_array = staticmethod(np.random.shuffle)

    @staticmethod
    def sample(n, k):
        return random.sample([j for j in range(n)], k)


class _SeededDraws:
    def __init__(self, *key):
        self.g = np.random.default_rng([int(k) & 0x7fffffff for k in key])

    def uniform(self, a, b):
        return float(self.g.uniform(a, b))

    def shuffle_list(self, x):
        order = self.g.permutation(len(x))
        x[:] = [x[i] for i in order]

    def shuffle_array(self, x):
        self.g.shuffle(x)

    def sample(self, n, k):
        return self.g.choice(n, size=k, replace=False).tolist()


class PoseDataset(torch.utils.data.Dataset):
    def __init__(self, mode, num_pt, add_noise, noise_trans, refine, data_set_name, root, show_sample=False, to_meter=True,
                 label_mode="new_pred", p_extra_data=0.0, p_viewpoints=1.0, seed=0, reference_rng=False, trancolor=None, device="cuda:0"):
        if mode not in ("train", "test"):
            raise ValueError("mode must be 'train' or 'test'")
        ds = os.path.join(root, "label_generator/data_sets/pose_estimation", data_set_name)
        self.mode, self.to_meter, self.num_pt, self.label_mode, self.refine, self.seed = mode, to_meter, num_pt, label_mode, refine, seed
        self.add_noise, self.noise_trans, self.show_sample = add_noise, noise_trans, show_sample
        self.p_extra_data, self.p_viewpoints, self.reference_rng = p_extra_data, p_viewpoints, reference_rng
        self.root = os.path.join(root, "data_generation/data")
        self.label_root = os.path.join(root, "label_generator/data")
        draws = _GlobalDraws if reference_rng else _SeededDraws(seed, 0x5eed)
        with open(os.path.join(ds, "train_data_list.txt" if mode == "train" else "test_data_list.txt")) as f:
            self.list = [ln.strip() for ln in f if ln.strip()]
        self.n_extra_samples, self.extra_data = 0, []
        if mode == "train":
            # viewpoint sub-selection (:57-74): the ids of the FIRST directory's samples are the view points
            start_l = self.list[0].split("/")[1]
            viewpoint_ids = []
            for ln in self.list:
                if ln.split("/")[1] != start_l:
                    break
                viewpoint_ids.append(ln[-6:])
            viewpoint_ids = np.array(viewpoint_ids)
            draws.shuffle_array(viewpoint_ids)
            viewpoints = viewpoint_ids[:int(len(viewpoint_ids) * self.p_viewpoints)]
            self.list = [ln for ln in self.list if ln[-6:] in viewpoints]
            if self.p_extra_data >= 0:                           # :77-97 (the reference's test is >= 0, so the list file must exist)
                ids = [int(v) for v in viewpoints]
                with open(os.path.join(ds, "extra_train_data_list.txt")) as f:
                    for ln in (x.strip() for x in f):
                        if ln and io.read_meta(os.path.join(self.root, os.path.dirname(ln)), os.path.basename(ln))["view_point_id"] in ids:
                            self.extra_data.append(ln)
                self.len_extra_data = len(self.extra_data)
                self.extra_data_ids = np.arange(self.len_extra_data)
                draws.shuffle_array(self.extra_data_ids)
                self.extra_data_index = 0
                self.n_extra_samples = int(len(self.list) * p_extra_data)
        self.len_data = len(self.list)
        self.length = self.len_data + self.n_extra_samples
        self.class_id_names, self.cld, self.symmetry_obj_idx = [], {}, []
        with open(os.path.join(ds, "classes.txt")) as f:
            for class_id, name in enumerate(ln.strip() for ln in f if ln.strip()):
                self.class_id_names.append(name)
                # the reference reads the `symmetric` flag from the first meta.json of the first listed directory (:109-117);
                # directory order is unspecified there, so take the first directory that holds a sample
                for sub in sorted(os.listdir(os.path.join(self.root, name))):
                    metas = sorted(m for m in os.listdir(os.path.join(self.root, name, sub)) if m.endswith(".meta.json"))
                    if metas:
                        with open(os.path.join(self.root, name, sub, metas[0])) as mf:
                            if bool(json.load(mf).get("symmetric", False)):
                                self.symmetry_obj_idx.append(class_id)
                        break
                self.cld[class_id] = read_xyz_dataset(os.path.join(root, "pc_reconstruction/data", name, "{}.xyz".format(name)), to_meter)
        self.num_classes = len(self.class_id_names)
        self.trancolor = trancolor if trancolor is not None else ColorJitterPIL(0.2, 0.2, 0.2, 0.05)
        self.num_pt_mesh = 1000
        self.minimum_num_pt = 50
        self.front_num = 2
        self.device = torch.device(device)
        self._res, self._meta_res = {}, {}

    def __len__(self):
        return self.length

    def get_sym_list(self):
        return self.symmetry_obj_idx

    def get_num_points_mesh(self):
        return self.num_pt_mesh

    # ---- which files a sample reads ------------------------------------------------------------------------------------------------------
    def _entry(self, index):
        """-> (list entry, label mode, wrapped).  Extra samples are handed out round-robin from the (filtered) extra list (:176-192; note
        the reference indexes `extra_data[extra_data_index]`, not the shuffled ids); `wrapped` tells that the round-robin index went back
        to 0, after which the reference reshuffles `extra_data_ids`: `_reshuffle_extra`, a draw of its own."""
        if index < self.len_data:
            return self.list[index], self.label_mode, False
        if index >= self.length:
            raise ValueError
        rel = self.extra_data[self.extra_data_index]
        self.extra_data_index += 1
        wrapped = self.extra_data_index >= self.len_extra_data
        if wrapped:
            self.extra_data_index = 0
        return rel, "new_pred", wrapped

    def _reshuffle_extra(self, index):
        self.extra_data_ids = np.arange(self.len_extra_data)
        (_GlobalDraws if self.reference_rng else _SeededDraws(self.seed, index, 1)).shuffle_array(self.extra_data_ids)

    def _metas(self, rel):
        d, sid = os.path.dirname(rel), os.path.basename(rel)
        image_meta = io.read_meta(os.path.join(self.root, d), sid)
        with open(os.path.join(self.label_root, d, "{}.meta.json".format(sid))) as f:
            meta = json.load(f)
        return image_meta, meta

    def _open(self, rel, lmode):
        d, sid = os.path.dirname(rel), os.path.basename(rel)
        return (Image.open(os.path.join(self.root, d, "{}.color.png".format(sid))),
                Image.open(os.path.join(self.root, d, "{}.depth.png".format(sid))),
                Image.open(os.path.join(self.label_root, d, "{}.{}.label.png".format(sid, lmode))))

    # ---- what depends on no pixel ---------------------------------------------------------------------------------------------------------
    def _draw_dellist(self, draws, obj):
        cld = self.cld[obj]
        return draws.sample(len(cld), len(cld) - self.num_pt_mesh) if len(cld) > self.num_pt_mesh else []   # (the reference raises below 1000)

    def _targets(self, meta, obj, angle, add_t, dellist):
        """model points and target (:216-229, :280-290): numpy's float64 throughout, cast once -> (target f32[M,3], model_points f32[M,3])"""
        cam2robot = np.array(meta["cam2robot"]).reshape(4, 4)
        if self.add_noise:
            a = np.deg2rad(0.0 if angle is None else angle)
            augment_rotation = np.identity(4)
            augment_rotation[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]   # euler2mat(0, 0, a) = Rz(a)
            cam2robot = np.dot(np.linalg.inv(augment_rotation), cam2robot)
        cam2object = np.dot(cam2robot, np.array(meta["robot2object"]).reshape(4, 4))
        target_r, target_t = cam2object[:3, :3], cam2object[:3, 3]
        if self.to_meter:
            target_t = target_t / 1000
        model_points = np.delete(self.cld[obj], dellist, axis=0)
        target = np.dot(model_points, target_r.T)
        target = np.add(target, target_t + add_t) if self.add_noise else np.add(target, target_t)
        return target.astype(np.float32), model_points.astype(np.float32)

    # ---- host path ------------------------------------------------------------------------------------------------------------------------
    def __getitem__(self, index):
        """draw, then `sample_host`: every parameter is drawn from the sample's generator at the place where the reference draws it"""
        return self.sample_host(index, None, _draws=_GlobalDraws if self.reference_rng else _SeededDraws(self.seed, index))

    def sample_host(self, index, params, _draws=None):
        """The sample through Pillow and numpy on the host, with injected parameters: a dict with `ops` (the ordered `(name, factor)` list
        of the jitter; [] = none), `angle` (the float given to `Image.rotate`; None = no rotation), `add_t` (3 floats), `subset` (the
        sorted ranks, among the valid pixels of the crop, that `choose` keeps; read only when there are more than num_pt), `dellist` (the
        model points dropped) and optionally `entry` ((list entry, label mode): the files to read; without it an index past the list
        advances the extra-data round-robin).  `ops`, `angle` and `add_t` are read only with add_noise.  `ds.batch(..., return_params=
        True)` returns such dicts."""
        p = dict(params or {})

        def need(key, draw):
            if key not in p:
                if _draws is None:
                    raise ValueError("sample_host: parameter %r is missing" % (key,))
                p[key] = draw()
            return p[key]

        if "entry" in p:
            rel, lmode = p["entry"]
        else:
            rel, lmode, wrapped = self._entry(index)
            if wrapped:
                self._reshuffle_extra(index)
        img, depth, label = self._open(rel, lmode)
        image_meta, meta = self._metas(rel)
        intr = image_meta["intr"]
        obj = self.class_id_names.index(meta["cls_name"])
        angle = None
        if self.add_noise:
            if "ops" in p or hasattr(self.trancolor, "params"):
                img = ColorJitterPIL.apply(img, need("ops", lambda: self.trancolor.params(_draws.uniform, _draws.shuffle_list)))
            else:
                img = self.trancolor(img)                        # a bare callable draws what it draws, where the reference calls it
            angle = need("angle", lambda: _draws.uniform(-180, 180))     # :211-217: in-plane rotation, PIL's default nearest resampling
            if angle is not None:
                img, label, depth = img.rotate(angle), label.rotate(angle), depth.rotate(angle)
        img, label, depth = np.array(img), np.array(label), np.array(depth)
        mask_label = label == 255
        if not mask_label.any():
            raise ValueError("sample %s: the label has no pixel equal to 255%s: get_bbox has no object to crop around"
                             % (rel, " after its rotation" if angle is not None else ""))
        rmin, rmax, cmin, cmax = get_bbox(mask_label)
        mask = mask_label * (depth != 0)
        add_t = np.array(need("add_t", lambda: [_draws.uniform(-self.noise_trans, self.noise_trans) for _ in range(3)]),
                         dtype=np.float64) if self.add_noise else None
        choose = mask[rmin:rmax, cmin:cmax].flatten().nonzero()[0]
        if len(choose) == 0:
            raise ValueError("sample %s: no pixel of the label has a depth: there is no point to choose" % (rel,))
        if len(choose) > self.num_pt:
            def draw_subset():
                c_mask = np.zeros(len(choose), dtype=int)
                c_mask[:self.num_pt] = 1
                _draws.shuffle_array(c_mask)
                return c_mask.nonzero()[0]
            choose = choose[np.asarray(need("subset", draw_subset))]
        else:
            choose = np.pad(choose, (0, self.num_pt - len(choose)), "wrap")
        wc = cmax - cmin
        d_m = depth[rmin:rmax, cmin:cmax].flatten()[choose][:, None].astype(np.float32)
        rows = (choose // wc + rmin)[:, None].astype(np.float32)
        cols = (choose % wc + cmin)[:, None].astype(np.float32)
        pt2 = d_m * image_meta["depth_scale"]
        if not self.to_meter:
            pt2 = pt2 * 1000
        cloud = np.concatenate(((cols - intr["ppx"]) * pt2 / intr["fx"], (rows - intr["ppy"]) * pt2 / intr["fy"], pt2), axis=1)
        if self.add_noise:
            cloud = np.add(cloud, add_t)
        target, model_points = self._targets(meta, obj, angle, add_t, need("dellist", lambda: self._draw_dellist(_draws, obj)))
        img_masked = np.transpose(img[:, :, :3], (2, 0, 1))[:, rmin:rmax, cmin:cmax].astype(np.float32)
        img_n = (torch.from_numpy(img_masked) - torch.from_numpy(_MEAN)[:, None, None]) / torch.from_numpy(_STD)[:, None, None]
        out = (torch.from_numpy(cloud.astype(np.float32)), torch.LongTensor(choose[None].astype(np.int64)), img_n,
               torch.from_numpy(target), torch.from_numpy(model_points), torch.LongTensor([int(obj)]))
        return out + (intr, img.copy()) if self.mode == "test" else out

    # ---- device path ----------------------------------------------------------------------------------------------------------------------
    def _resident(self, rel, lmode):
        """the decoded frames of one entry on the device (u8 [H,W,3], u16 [H,W], u8 [H,W]), decoded once and kept"""
        key = (rel, lmode)
        r = self._res.get(key)
        if r is None:
            img, depth, label = (np.array(x) for x in self._open(rel, lmode))
            if (img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8 or depth.dtype != np.uint16 or label.dtype != np.uint8
                    or img.shape[:2] != (img_width, img_length) or depth.shape != img.shape[:2] or label.shape != img.shape[:2]):
                raise ValueError("sample %s: the builder takes %d x %d frames (get_bbox and the reference's xmap / ymap are fixed to that "
                                 "size): 8-bit RGB, 16-bit depth and a one-band 8-bit label, got %s %s, %s %s and %s %s"
                                 % (rel, img_width, img_length, img.shape, img.dtype, depth.shape, depth.dtype, label.shape, label.dtype))
            r = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(self.device) for x in (img, depth, label))
            self._res[key] = r
        return r

    def batch(self, indices, params=None, return_params=False):
        """The samples `[ds[i] for i in indices]` built on the device (augment.py, csrc/pose_train.hip) -> a list of the reference's
        6-tuples as `DataLoader(batch_size=1)` delivers them: points[1,N,3] f32, choose[1,1,N] i64, img[1,3,Hc,Wc] f32, target[1,M,3] f32,
        model_points[1,M,3] f32, idx[1,1] i64 -- views into one packed block per batch (+ intr and the resident u8 frame [1,H,W,3] in
        mode 'test').  Every file is decoded once, on first use, and stays on the GPU.

        Draws.  Without `params` the batch draws what the samples would draw and leaves the generators as `[ds[i] for i in indices]`
        leaves them.  Before the first launch, per sample in order: jitter, angle, the three `add_t` uniforms; after the read-back of
        the pixel counts, per sample in order: the `c_mask` shuffle (only with more than num_pt valid pixels), then the model-point
        sample.  That is the one order a seeded sample's own generator allows.  With reference_rng the two global streams are
        independent: `random` carries jitter, angle, add_t and `random.sample`, none of which depends on a pixel, so all of them are
        drawn before the first launch, sample by sample as the reference interleaves them; `numpy.random` carries the `c_mask` shuffles
        and the reshuffle of `extra_data_ids` when the round-robin wraps, drawn after the read-back in sample order.
        return_params adds the parameter dicts used (see `sample_host`), entries included."""
        from autoposeestimation_amd.DenseFusion.datasets.myDatasetAugmented import augment as G
        indices = packed.batch_indices(self, indices, params, self.add_noise)
        if not indices:
            return ([], []) if return_params else []
        given = params is not None
        ps, draws, wraps, metas, frames, cams = [], [], [], [], [], []
        for k, i in enumerate(indices):                          # everything that depends on no pixel
            p = dict(params[k]) if given else {}
            d = None if given else (_GlobalDraws if self.reference_rng else _SeededDraws(self.seed, i))
            if "entry" in p:
                rel, lmode, wrapped = p["entry"][0], p["entry"][1], False
            else:
                rel, lmode, wrapped = self._entry(i)
                p["entry"] = (rel, lmode)
            if rel not in self._meta_res:                        # like the frames: read once, kept
                self._meta_res[rel] = self._metas(rel)
            image_meta, meta = self._meta_res[rel]
            obj = self.class_id_names.index(meta["cls_name"])
            if self.add_noise:
                if not given:
                    p["ops"] = self.trancolor.params(d.uniform, d.shuffle_list)
                    p["angle"] = d.uniform(-180, 180)
                    p["add_t"] = [d.uniform(-self.noise_trans, self.noise_trans) for _ in range(3)]
                for key in ("ops", "angle", "add_t"):
                    if key not in p:
                        raise ValueError("batch: parameter %r of sample %d is missing" % (key, k))
            if not given and self.reference_rng:
                p["dellist"] = self._draw_dellist(d, obj)
            ps.append(p)
            draws.append(d)
            wraps.append(wrapped)
            metas.append((meta, obj))
            frames.append(self._resident(rel, lmode))
            cams.append((image_meta["intr"], image_meta["depth_scale"]))

        def select(k, count):
            """the draws of sample k that wait for its pixel count -> the ranks kept, or None"""
            p, d = ps[k], draws[k]
            if wraps[k]:
                self._reshuffle_extra(indices[k])
            if count > self.num_pt and "subset" not in p:
                if d is None:
                    raise ValueError("batch: sample %d has %d valid pixels, more than num_pt = %d, and its parameters give no 'subset'"
                                     % (k, count, self.num_pt))
                p["subset"] = packed.draw_subset(d, count, self.num_pt)
            if "dellist" not in p:
                if d is None:
                    raise ValueError("batch: parameter 'dellist' of sample %d is missing" % k)
                p["dellist"] = self._draw_dellist(d, metas[k][1])
            return p.get("subset") if count > self.num_pt else None

        views = G.build_samples(frames, ps, cams, self.num_pt, self.to_meter, self.add_noise, _MEAN, _STD, select,
                                names=[p["entry"][0] for p in ps])
        # target, model points and idx: numpy's float64 on the host as __getitem__ has them, one upload per batch
        host = []
        for p, (meta, obj) in zip(ps, metas):
            add_t = np.array(p["add_t"], dtype=np.float64) if self.add_noise else None
            target, model_points = self._targets(meta, obj, p.get("angle") if self.add_noise else None, add_t, p["dellist"])
            host.append((target, model_points, obj))
        up = packed.upload_targets(host, self.device)
        out = []
        for k, ((points, choose, img), (target, model_points, idx)) in enumerate(zip(views, up)):
            s = (points, choose, img, target, model_points, idx)
            out.append(s + (cams[k][0], frames[k][0].unsqueeze(0)) if self.mode == "test" else s)
        return (out, ps) if return_params else out

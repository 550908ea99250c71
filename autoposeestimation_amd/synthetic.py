"""Deterministic synthetic weights and RGB-D frames (no datasets, no checkpoints, no network).

The reference ships no weights ("Checkpoint / resume"), so parity tests, the golden
generator (tools/gen_golden.py) and bench.py all need weights that

  * carry exactly the reference's state-dict key names and shapes
    (PoseNet: 77 tensors, PoseRefineNet: 24 tensors -- DenseFusion/lib/network.py:70-132,170-206,
    pspnet.py:40-62, extractors.py:78-112), so they load into the reference modules with strict=True
    (that is how gen_golden.py proves the key layout), and
  * can be regenerated bit-identically anywhere from (name, seed) alone -- an 86 MB PoseNet state
    dict cannot be committed as a fixture.  numpy's PCG64 `default_rng` stream is stable across
    platforms and numpy versions, torch's generator is not guaranteed to be.

Scales are chosen so that activations stay O(1..100) from the raw 0-255 ImageNet-"normalised" crop
(pipeline/utils.py:559-560 feeds (rgb-0.485)/0.229, i.e. values up to ~1100) down to O(0.1) pose
outputs, the way a trained network's would; He-style fan-in scaling elsewhere.
"""
import zlib
from collections import OrderedDict

import numpy as np
import torch

_BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def _rng(seed, key):
    return np.random.default_rng([int(seed), zlib.crc32(key.encode())])


def _normal(seed, key, shape, std):
    return torch.from_numpy((_rng(seed, key).standard_normal(shape, dtype=np.float32) * np.float32(std)))


def _uniform(seed, key, shape, bound):
    return torch.from_numpy(((_rng(seed, key).random(shape, dtype=np.float32) * 2 - 1) * np.float32(bound)))


def pspnet_spec(backend="resnet18", n_classes=21, in_channels=3):
    """[(key, shape)] of DenseFusion/lib/pspnet.py:PSPNet with a BasicBlock encoder, in state_dict order.
    in_channels != 3 only for the segmentor stand-ins (the background-subtraction network reads 7 channels)."""
    spec = [("feats.conv1.weight", (64, in_channels, 7, 7))]
    inplanes = 64
    for li, (planes, nblk, stride) in enumerate(zip((64, 128, 256, 512), _BLOCKS[backend], (1, 2, 1, 1)), start=1):
        for b in range(nblk):
            cin = inplanes if b == 0 else planes
            spec.append((f"feats.layer{li}.{b}.conv1.weight", (planes, cin, 3, 3)))
            spec.append((f"feats.layer{li}.{b}.conv2.weight", (planes, planes, 3, 3)))
            if b == 0 and (stride != 1 or inplanes != planes):
                spec.append((f"feats.layer{li}.{b}.downsample.0.weight", (planes, inplanes, 1, 1)))
        inplanes = planes
    for s in range(4):
        spec.append((f"psp.stages.{s}.1.weight", (512, 512, 1, 1)))
    spec += [("psp.bottleneck.weight", (1024, 2560, 1, 1)), ("psp.bottleneck.bias", (1024,))]
    for name, cin, cout in (("up_1", 1024, 256), ("up_2", 256, 64), ("up_3", 64, 64)):
        spec += [(f"{name}.conv.1.weight", (cout, cin, 3, 3)), (f"{name}.conv.1.bias", (cout,)),
                 (f"{name}.conv.2.weight", (1,))]
    spec += [("final.0.weight", (32, 64, 1, 1)), ("final.0.bias", (32,))]
    spec += [("classifier.0.weight", (256, 256)), ("classifier.0.bias", (256,)),
             ("classifier.2.weight", (n_classes, 256)), ("classifier.2.bias", (n_classes,))]
    return spec


def _fill(spec, seed, prefix="", overrides=None):
    """He-normal (fan-in) weights, small uniform biases, PReLU slope 0.25; `overrides[key]` scales std."""
    overrides = overrides or {}
    sd = OrderedDict()
    for key, shape in spec:
        full = prefix + key
        if len(shape) == 1 and key.endswith(".conv.2.weight"):  # nn.PReLU single slope (pspnet.py:33)
            sd[full] = torch.full(shape, 0.25, dtype=torch.float32)
            continue
        if key.endswith(".bias"):
            sd[full] = _uniform(seed, full, shape, 0.05 * overrides.get(key, 1.0))
            continue
        fan_in = int(np.prod(shape[1:]))
        std = (2.0 / fan_in) ** 0.5 * overrides.get(key, 1.0)
        sd[full] = _normal(seed, full, shape, std)
    return sd


def pspnet_state_dict(backend="resnet18", seed=0, prefix="", n_classes=21, stem_gain=1.0 / 256.0, in_channels=3):
    """stem_gain: the PoseNet crop encoder sees raw 0-255-scale pixels (pipeline/utils.py:559-560), so its stem is scaled
    by 1/256 to bring them to O(1) like a trained first layer would; a SEGMENTOR sees ToTensor'd [0,1] pixels
    (pipeline/utils.py:421-424) -> use stem_gain=1.0 there."""
    spec = pspnet_spec(backend, n_classes, in_channels)
    over = {"feats.conv1.weight": stem_gain, "final.0.weight": 0.35}
    # residual branches at half gain so 8..16 un-normalised blocks do not blow the variance up
    over.update({k: 0.5 for k, _ in spec if k.startswith("feats.layer") and k.endswith("conv2.weight")})
    return _fill(spec, seed, prefix, over)



def unet_spec(encoder="resnet34", in_channels=3, classes=1):
    """[(key, shape)] of smp 0.1.3's Unet (segmentation/unet.py) in state_dict order; BatchNorm layers as (prefix, (C,), 'bn')"""
    spec = [("encoder.conv1.weight", (64, in_channels, 7, 7)), ("encoder.bn1", (64,), "bn")]
    cin = 64
    for li, (planes, n) in enumerate(zip((64, 128, 256, 512), _BLOCKS[encoder]), 1):
        for b in range(n):
            p = "encoder.layer%d.%d." % (li, b)
            spec += [(p + "conv1.weight", (planes, cin, 3, 3)), (p + "bn1", (planes,), "bn"),
                     (p + "conv2.weight", (planes, planes, 3, 3)), (p + "bn2", (planes,), "bn")]
            if b == 0 and li > 1:
                spec += [(p + "downsample.0.weight", (planes, cin, 1, 1)), (p + "downsample.1", (planes,), "bn")]
            cin = planes
    for i, (c1, c2, co) in enumerate(zip((512, 256, 128, 64, 32), (256, 128, 64, 64, 0), (256, 128, 64, 32, 16))):
        p = "decoder.blocks.%d." % i
        spec += [(p + "conv1.0.weight", (co, c1 + c2, 3, 3)), (p + "conv1.1", (co,), "bn"),
                 (p + "conv2.0.weight", (co, co, 3, 3)), (p + "conv2.1", (co,), "bn")]
    spec += [("segmentation_head.0.weight", (classes, 16, 3, 3)), ("segmentation_head.0.bias", (classes,))]
    return spec


def unet_state_dict(encoder="resnet34", seed=0, in_channels=3, classes=1):
    """Synthetic weights for segmentation/unet.py with every key of smp's Unet: He-normal convolutions, BatchNorm layers with non-trivial
    running statistics (mean +-0.2, variance 0.5..2, gamma / beta), the residual branches' last BN at half gain so that the 8..16 blocks do
    not blow the variance up; activations stay O(1) through all ~45 layers"""
    sd = OrderedDict()
    for item in unet_spec(encoder, in_channels, classes):
        key, shape = item[0], item[1]
        if len(item) == 3:                               # BatchNorm2d(C): weight, bias, running_mean, running_var, num_batches_tracked
            c = shape[0]
            g = 0.5 if (key.endswith("bn2") and ".layer" in key) else 1.0
            sd[key + ".weight"] = (0.8 + 0.4 * _rng(seed, key + "g").random(c)).astype(np.float32) * np.float32(g)
            sd[key + ".bias"] = _uniform(seed, key + "b", (c,), 0.1)
            sd[key + ".running_mean"] = _uniform(seed, key + "m", (c,), 0.2)
            sd[key + ".running_var"] = torch.from_numpy((0.5 + 1.5 * _rng(seed, key + "v").random(c)).astype(np.float32))
            sd[key + ".num_batches_tracked"] = torch.tensor(1000, dtype=torch.int64)
            sd[key + ".weight"] = torch.from_numpy(sd[key + ".weight"])
            continue
        if key.endswith(".bias"):
            sd[key] = _uniform(seed, key, shape, 0.05)
            continue
        fan_in = int(np.prod(shape[1:]))
        sd[key] = _normal(seed, key, shape, (2.0 / fan_in) ** 0.5)
    return sd

def segnet_state_dict(seed=0, input_nbr=3, label_nbr=22):
    """Synthetic weights with every key of DenseFusion/vanilla_segmentation/segnet.py:SegNet, in its state-dict order: He-normal
    convolutions, biases ~ N(0, 0.1), gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1), running statistics away from (0, 1) (mean +-0.2, variance
    0.5..2): activations stay O(1) through the 26 layers"""
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation.segnet import layer_table
    sd = OrderedDict()
    for name, cin, cout, has_bn in layer_table(input_nbr, label_nbr):
        k = "conv" + name
        sd[k + ".weight"] = _normal(seed, k + "w", (cout, cin, 3, 3), (2.0 / (9 * cin)) ** 0.5)
        sd[k + ".bias"] = _normal(seed, k + "b", (cout,), 0.1)
        if has_bn:
            k = "bn" + name
            sd[k + ".weight"] = torch.from_numpy((0.5 + _rng(seed, k + "g").random(cout)).astype(np.float32))
            sd[k + ".bias"] = _normal(seed, k + "b", (cout,), 0.1)
            sd[k + ".running_mean"] = _uniform(seed, k + "m", (cout,), 0.2)
            sd[k + ".running_var"] = torch.from_numpy((0.5 + 1.5 * _rng(seed, k + "v").random(cout)).astype(np.float32))
            sd[k + ".num_batches_tracked"] = torch.tensor(1000, dtype=torch.int64)
    return sd


def _pointnet_spec(refine):
    c5 = 384 if refine else 256
    return [("feat.conv1.weight", (64, 3, 1)), ("feat.conv1.bias", (64,)),
            ("feat.conv2.weight", (128, 64, 1)), ("feat.conv2.bias", (128,)),
            ("feat.e_conv1.weight", (64, 32, 1)), ("feat.e_conv1.bias", (64,)),
            ("feat.e_conv2.weight", (128, 64, 1)), ("feat.e_conv2.bias", (128,)),
            ("feat.conv5.weight", (512, c5, 1)), ("feat.conv5.bias", (512,)),
            ("feat.conv6.weight", (1024, 512, 1)), ("feat.conv6.bias", (1024,))]


def posenet_state_dict(num_obj, seed=0):
    """77 tensors with the key names of DenseFusion/lib/network.py:PoseNet (incl. `cnn.model.module.`)."""
    sd = pspnet_state_dict("resnet18", seed, prefix="cnn.model.module.")
    spec = _pointnet_spec(False)
    for i, (cin, cout) in enumerate(((1408, 640), (640, 256), (256, 128)), start=1):
        for h in "rtc":
            spec += [(f"conv{i}_{h}.weight", (cout, cin, 1)), (f"conv{i}_{h}.bias", (cout,))]
    for h, m in (("r", 4), ("t", 3), ("c", 1)):
        spec += [(f"conv4_{h}.weight", (num_obj * m, 128, 1)), (f"conv4_{h}.bias", (num_obj * m,))]
    # point coordinates are metres (O(0.5)): lift conv1 so geometry and colour features have equal weight;
    # keep translation offsets ~cm and confidence logits O(1)
    over = {"feat.conv1.weight": 2.0, "conv4_t.weight": 0.02, "conv4_t.bias": 0.2, "conv4_c.weight": 0.5}
    sd.update(_fill(spec, seed, "", over))
    return sd


def refiner_state_dict(num_obj, seed=0):
    """24 tensors with the key names of DenseFusion/lib/network.py:PoseRefineNet."""
    spec = _pointnet_spec(True)
    for i, (cin, cout) in enumerate(((1024, 512), (512, 128)), start=1):
        for h in "rt":
            spec += [(f"conv{i}_{h}.weight", (cout, cin)), (f"conv{i}_{h}.bias", (cout,))]
    for h, m in (("r", 4), ("t", 3)):
        spec += [(f"conv3_{h}.weight", (num_obj * m, 128)), (f"conv3_{h}.bias", (num_obj * m,))]
    over = {"feat.conv1.weight": 2.0, "conv3_t.weight": 0.02, "conv3_t.bias": 0.2}
    sd = _fill(spec, seed + 1, "", over)
    # a refiner predicts a *residual* rotation: bias the quaternion head towards identity (w dominant)
    b = sd["conv3_r.bias"].view(num_obj, 4)
    b[:, 0] += 1.0
    return sd


# ----------------------------------------------------------------------------------------------
# synthetic RGB-D frames
# ----------------------------------------------------------------------------------------------
REALSENSE_META = {"intr": {"fx": 615.0, "fy": 615.0, "ppx": 320.0, "ppy": 240.0}, "depth_scale": 0.001}
YCB_META = {"intr": {"fx": 1066.778, "fy": 1067.487, "ppx": 312.9869, "ppy": 241.3109}, "depth_scale": 1.0 / 10000}

CLASS_COLOURS = np.array([[230, 40, 40], [40, 200, 60], [50, 80, 230], [230, 210, 40], [200, 50, 200],
                          [40, 210, 210], [250, 140, 30], [130, 60, 20], [120, 120, 250], [20, 120, 70],
                          [250, 160, 200], [90, 90, 90]], dtype=np.uint8)


def synthetic_frame(frame_id, cls=1, box=(150, 250), size=(150, 150), h=480, w=640):
    """One 640x480 RGB u8 + depth u16 frame with a single painted box "object" of class `cls` (1-based).

    Returns (rgb[h,w,3] u8, depth[h,w] u16, label[h,w] u8 with {0, cls}).  The default 150x150 box
    makes `get_bbox` (myDatasetAugmented/dataset.py:342-380) round the crop up to 160x160.
    Background: uniform noise in [96,160); depth: plane at 600 mm, object 80 mm closer with a
    smooth bump, 2 % of all pixels invalid (0).
    """
    return synthetic_frame_multi(frame_id, [(cls, box, size)], h, w)


def synthetic_frame_multi(frame_id, objects, h=480, w=640):
    """synthetic_frame with several painted boxes: objects = [(cls, (r0, c0), (rh, rw)), ...] (non-overlapping, distinct classes -- the
    live path keeps one detection per class and frame, pipeline/utils.py:444-470).  One object gives exactly synthetic_frame's arrays
    (same generator, same draw order: background, per object its colour jitter, then the invalid-depth mask)."""
    rng = np.random.default_rng(int(frame_id))
    rgb = rng.integers(96, 160, size=(h, w, 3), dtype=np.uint8)
    label = np.zeros((h, w), np.uint8)
    depth = np.full((h, w), 600, np.uint16)
    for cls, (r0, c0), (rh, rw) in objects:
        label[r0:r0 + rh, c0:c0 + rw] = cls
        col = CLASS_COLOURS[(cls - 1) % len(CLASS_COLOURS)].astype(np.int16)
        jitter = rng.integers(-12, 13, size=(rh, rw, 3), dtype=np.int16)
        rgb[r0:r0 + rh, c0:c0 + rw] = np.clip(col + jitter, 0, 255).astype(np.uint8)
        yy, xx = np.mgrid[0:rh, 0:rw]
        bump = 40.0 * np.exp(-(((yy - rh / 2) / (rh / 3)) ** 2 + ((xx - rw / 2) / (rw / 3)) ** 2))
        depth[r0:r0 + rh, c0:c0 + rw] = (520 - bump).astype(np.uint16)
    depth[rng.random((h, w)) < 0.02] = 0
    return rgb, depth, label


# SURVEY.md 8d's crop sweep {80^2, 120x160, 160^2, 240^2, 320x400}: painted sizes that get_bbox (myDatasetAugmented/dataset.py:342-380) rounds
# up to those crops
MIXED_SIZES = ((70, 70), (110, 150), (150, 150), (230, 230), (310, 390))


def mixed_frame(frame_id, h=480, w=640, margin=24):
    """A frame of the `bench.py --mixed` sweep: 1-3 objects of distinct classes (1..3), sizes drawn from MIXED_SIZES, placed at random
    without overlap (a draw that does not fit after 40 tries is dropped, so a frame holds at least its first object).  Seeded by
    frame_id alone.  Returns (rgb, depth, label, objects)."""
    rng = np.random.default_rng([4242, int(frame_id)])
    n_obj = int(rng.integers(1, 4))
    classes = rng.permutation(3)[:n_obj] + 1
    placed = []
    for cls in classes.tolist():
        for _ in range(40):
            rh, rw = MIXED_SIZES[int(rng.integers(0, len(MIXED_SIZES)))]
            r0 = int(rng.integers(margin, h - margin - rh + 1)) if h - 2 * margin - rh >= 0 else -1
            c0 = int(rng.integers(margin, w - margin - rw + 1)) if w - 2 * margin - rw >= 0 else -1
            if r0 < 0 or c0 < 0:
                continue
            if all(r0 + rh + margin <= pr or pr + ph + margin <= r0 or c0 + rw + margin <= pc or pc + pw + margin <= c0
                   for _, (pr, pc), (ph, pw) in placed):
                placed.append((cls, (r0, c0), (rh, rw)))
                break
    rgb, depth, label = synthetic_frame_multi(900000 + int(frame_id), placed, h, w)
    return rgb, depth, label, placed


def model_cloud(cls, m=1000, seed=1234):
    """`m` model points uniform in a 0.1 m cube (metres), per class."""
    rng = np.random.default_rng([seed, int(cls)])
    return ((rng.random((m, 3), dtype=np.float32) - 0.5) * np.float32(0.1)).astype(np.float32)


def fit_final_layer(feats, labels, n_out, margin=8.0, ridge=1e-2):
    """Least-squares "training" of a segmentor's final 1x1 conv on frozen random features, so that synthetic frames
    segment into their painted object with real logit margins (random weights alone give a random label map).
    feats[P,C] float tensor (any device; C = 64 for the PSPNet), labels[P] int64 in [0,n_out) -> (W[n_out,C], b[n_out]) float32 on CPU.
    Targets: +margin for the pixel's class, -margin for every other class."""
    f = feats.double()
    p = f.shape[0]
    a = torch.cat([f, torch.ones(p, 1, dtype=torch.float64, device=f.device)], 1)
    t = torch.full((p, n_out), -float(margin), dtype=torch.float64, device=f.device)
    t[torch.arange(p, device=f.device), labels.to(f.device)] = float(margin)
    ata = a.t() @ a + ridge * p * torch.eye(a.shape[1], dtype=torch.float64, device=f.device)
    sol = torch.linalg.solve(ata, a.t() @ t)          # [C + 1, n_out]
    c = f.shape[1]
    return sol[:c].t().float().cpu().contiguous(), sol[c].float().cpu().contiguous()


# ---- label path (BASELINE configs[4]): synthetic multi-view depth renders of a known object --------------------------------------
LABEL_INTR = {"fx": 615.0, "fy": 615.0, "ppx": 320.0, "ppy": 240.0}
LABEL_CENTRE = np.array([400.0, -20.0, 150.0])


def rigid(rx, ry, rz, t):
    """4x4 from Euler ZYX angles (R = Rz Ry Rx) and a translation"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def bumpy_sphere(n, seed, radius=60.0, centre=LABEL_CENTRE):
    """a sphere with bumps (SURVEY.md 8d, config 5's known object), n surface samples in the robot frame (mm)"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = radius * (1 + 0.15 * np.sin(3 * v[:, 0]) * np.cos(4 * v[:, 1]) + 0.1 * np.sin(5 * v[:, 2]))
    return v * r[:, None] + np.asarray(centre)


def render_depth(points, cam2robot, intr=LABEL_INTR, h=480, w=640):
    """z-buffer render of a robot-frame cloud into a uint16 depth image (mm) for a pin-hole camera at `cam2robot`"""
    Tinv = np.linalg.inv(cam2robot)
    pc = points @ Tinv[:3, :3].T + Tinv[:3, 3]
    pc = pc[pc[:, 2] > 50]
    u = np.round(pc[:, 0] * intr["fx"] / pc[:, 2] + intr["ppx"]).astype(int)
    v = np.round(pc[:, 1] * intr["fy"] / pc[:, 2] + intr["ppy"]).astype(int)
    ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    depth = np.zeros((h, w), np.float64)
    order = np.argsort(-pc[ok, 2])
    depth[v[ok][order], u[ok][order]] = np.round(pc[ok, 2][order])
    return depth.astype(np.uint16)


def label_views(n_views, seed=0, cloud=None, distance=500.0, poses=None):
    """`n_views` (label u8, depth u16, robot2cam 4x4) of the bumpy sphere.  `poses` = robot2cam matrices to render from (the reference's
    own capture path: `capture_path()`); without them the cameras sit on a cap around the object (looking at it from `distance` mm,
    tilted by up to +-1 rad about y and +-0.5 rad about x, drawn from `seed`)."""
    cloud = bumpy_sphere(300000, 21) if cloud is None else cloud
    rng = np.random.default_rng(seed)
    views = []
    for i in range(n_views):
        if poses is not None:
            cam = np.asarray(poses[i % len(poses)], dtype=np.float64)
        else:
            ang_y, ang_x = rng.uniform(-1.0, 1.0), rng.uniform(-0.5, 0.5)
            cam = rigid(np.pi, 0.0, 0.0, tuple(LABEL_CENTRE + [0, 0, distance]))
            cam = rigid(0, 0, 0, tuple(LABEL_CENTRE)) @ rigid(ang_x, ang_y, 0.0, (0, 0, 0)) @ rigid(0, 0, 0, tuple(-LABEL_CENTRE)) @ cam
        depth = render_depth(cloud, cam)
        views.append(((depth != 0).astype(np.uint8) * 255, depth, cam))
    return views


def capture_path():
    """(robot2cam[164, 4, 4], focus[3]): the camera poses of the reference's capture run (robot_controller/robot_path/
    viewpointsPath2.json through the hand-eye calibration) and the point its optical axes meet in, from the committed fixture
    tests/golden/viewpoints_path2.npz (tools/gen_golden_viewpoints.py); None when the fixture is absent."""
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "viewpoints_path2.npz")
    if not os.path.exists(path):
        return None
    d = np.load(path)
    return d["robot2cam"], d["focus"]


def pose_dataset_tree(root, data_set_name="synth", n_view=5, n_extra=3, seed=3):
    """A small pose-estimation data set in the reference's on-disk layout (data_generation/getData.py:177-221,
    label_generator/create_labels.py:422-429, create_pointcloud.py:373-376, make_train_and_test_dataset): two classes (the second
    symmetric), `n_view` view-point samples each under `<cls>/foreground`, `n_extra` extra samples under `<cls>/extra`, label PNGs in
    all three label modes, pose-label JSONs, `.xyz` model clouds (1200 points, mm) and the list files.  Deterministic in `seed`;
    shared by tools/gen_golden_dataset.py (which runs the REFERENCE's PoseDataset on it) and tests/test_pose_dataset_golden.py."""
    import json
    import os
    from PIL import Image
    rng = np.random.default_rng(seed)
    classes = ["objA", "objB"]
    ds = os.path.join(root, "label_generator/data_sets/pose_estimation", data_set_name)
    os.makedirs(ds, exist_ok=True)
    train, test, extra = [], [], []
    for ci, cls in enumerate(classes):
        cloud = (rng.uniform(-40, 40, (1200, 3)) * [1.0, 0.7, 0.5]).round(3)
        os.makedirs(os.path.join(root, "pc_reconstruction/data", cls), exist_ok=True)
        with open(os.path.join(root, "pc_reconstruction/data", cls, cls + ".xyz"), "w") as f:
            for item in cloud:
                f.write("%s\n" % item)                          # numpy's repr of the point, as create_pointcloud.py:373-376 writes it
        for sub, n in (("foreground", n_view), ("extra", n_extra)):
            ddir = os.path.join(root, "data_generation/data", cls, sub)
            ldir = os.path.join(root, "label_generator/data", cls, sub)
            os.makedirs(ddir, exist_ok=True)
            os.makedirs(ldir, exist_ok=True)
            for i in range(n):
                sid = "%06d" % i
                h, w = 480, 640
                r0, c0 = int(rng.integers(60, 250)), int(rng.integers(80, 380))
                hh, ww = int(rng.integers(70, 150)), int(rng.integers(70, 170))
                yy, xx = np.mgrid[0:h, 0:w]
                inside = (((yy - r0 - hh / 2) / (hh / 2)) ** 2 + ((xx - c0 - ww / 2) / (ww / 2)) ** 2) < 1
                rgb = (rng.integers(0, 60, (h, w, 3)) + 90).astype(np.uint8)
                rgb[inside] = (CLASS_COLOURS[ci] * 0.8).astype(np.uint8) + rng.integers(0, 40, (int(inside.sum()), 3)).astype(np.uint8)
                depth = np.full((h, w), 620, np.uint16) + (xx // 40).astype(np.uint16)
                depth[inside] = (560 + 25 * np.sin(xx[inside] / 17.0) + 15 * np.cos(yy[inside] / 13.0)).astype(np.uint16)
                depth[rng.random((h, w)) < 0.03] = 0
                Image.fromarray(rgb).save(os.path.join(ddir, sid + ".color.png"))
                Image.fromarray(depth).save(os.path.join(ddir, sid + ".depth.png"))
                meta = {"intr": dict(REALSENSE_META["intr"]), "depth_scale": 0.001, "symmetric": bool(ci == 1), "view_point_id": i % n_view,
                        "robot2endEff_tf": np.eye(4).flatten().tolist(), "hand_eye_calibration": np.eye(4).flatten().tolist(),
                        "object_pose": np.eye(4).flatten().tolist()}
                with open(os.path.join(ddir, sid + ".meta.json"), "w") as f:
                    json.dump(meta, f)
                lab = inside.astype(np.uint8) * 255
                for mode in ("gen", "pred", "new_pred"):
                    Image.fromarray(lab).save(os.path.join(ldir, "%s.%s.label.png" % (sid, mode)))
                cam2robot = rigid(rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-3, 3), tuple(rng.uniform(-50, 50, 3)))
                robot2object = rigid(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-1, 1), tuple(rng.uniform(-30, 30, 2)) + (float(rng.uniform(500, 650)),))
                with open(os.path.join(ldir, sid + ".meta.json"), "w") as f:
                    json.dump({"cls_name": cls, "cam2robot": cam2robot.flatten().tolist(), "robot2object": robot2object.flatten().tolist()}, f)
                rel = "%s/%s/%s" % (cls, sub, sid)
                if sub == "extra":
                    extra.append(rel)
                elif i == n - 1:
                    test.append(rel)
                else:
                    train.append(rel)
    with open(os.path.join(ds, "classes.txt"), "w") as f:
        f.write("".join(c + "\n" for c in classes))
    for name, items in (("train_data_list.txt", train), ("test_data_list.txt", test), ("extra_train_data_list.txt", extra)):
        with open(os.path.join(ds, name), "w") as f:
            f.write("".join(x + "\n" for x in items))
    return classes, train, test, extra


# ---- a LineMOD-shaped tree (DenseFusion/datasets/linemod/dataset.py:24-88) ----------------------------------------------------------------
LINEMOD_OBJECTS = [1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15]
# lines of test.txt per object.  The reference's keep-every-tenth counter runs on across the objects and is incremented before the
# end-of-file check, so an end of file that does not fall on a multiple of ten is read again until one does: mode 'test' keeps the tenth
# line of the objects that have one -- here objects 2, 5, 11 (symmetric) and 13
LINEMOD_TEST_LINES = [1, 10, 2, 10, 1, 1, 2, 1, 10, 1, 10, 1, 2]


# The objects whose 'eval' samples are counted: the segnet_results labels of the others are empty (lost detections).  These are the objects
# whose confidence head, with the seeded weights posenet_state_dict(13, 0), answers a far point with a maximum at least 1e-2 above the
# second confidence; the heads of the others saturate (object 2: every confidence within 2e-5 of 1.0) or answer it with their minimum, so
# that no frame gives their arg-max a margin.  Object 11 is one of the symmetric pair.
LINEMOD_EVAL_OBJECTS = (1, 5, 6, 9, 11)


def linemod_tree(root, seed=0):
    """A small LineMOD_preprocessed tree: for each of the 13 objects `data/%02d/{rgb,depth,mask}/%04d.png` (480 x 640; the mask with three
    bands), `gt.yml` (object 2 with two records per frame, the first of another object), `train.txt`, `test.txt`, `models/obj_%02d.ply`
    (more than 500 vertices, mm) and `segnet_results/%02d_label/%04d_label.png` (one band; for LINEMOD_EVAL_OBJECTS it differs from the mask: most of
    the object cut off, a hole, an extra blob, a region of another value, one far depth value; for the other objects it is empty = a lost
    detection), and `models/models_info.yml` with
    diameters chosen so that random networks pass the ADD threshold for some objects and fail it for others.  `obj_bb` is the mask's
    box moved and resized by a few pixels, so mask pixels fall outside the crop.  Deterministic in `seed`.
    Shared by tools/gen_golden_linemod.py (which runs the REFERENCE's PoseDataset on it) and the LineMOD tests.
    -> {object id: [frame names of test.txt]}"""
    import os
    from PIL import Image
    rng = np.random.default_rng([77, int(seed)])
    h, w = 480, 640
    yy, xx = np.mgrid[0:h, 0:w]
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    frames_of, info = {}, []
    for oi, obj in enumerate(LINEMOD_OBJECTS):
        d = os.path.join(root, "data", "%02d" % obj)
        seg = os.path.join(root, "segnet_results", "%02d_label" % obj)
        for sub in ("rgb", "depth", "mask"):
            os.makedirs(os.path.join(d, sub), exist_ok=True)
        os.makedirs(seg, exist_ok=True)
        n_vtx = 520 + 7 * oi
        vtx = (rng.uniform(-1, 1, (n_vtx, 3)) * [40.0 + 3 * oi, 30.0, 25.0 + oi]).round(4)
        with open(os.path.join(root, "models", "obj_%02d.ply" % obj), "w") as f:
            f.write("ply\nformat ascii 1.0\ncomment synthetic\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                    "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                    "element face 0\nproperty list uchar int vertex_indices\nend_header\n" % n_vtx)
            for v in vtx:
                f.write("%.4f %.4f %.4f 0.0 0.0 1.0 %d %d %d\n" % (v[0], v[1], v[2], 200, 100, 50))
        info.append("%d: {diameter: %.8f, min_x: 0.0, min_y: 0.0, min_z: 0.0, size_x: 1.0, size_y: 1.0, size_z: 1.0}\n"
                    % (obj, 40000.0 if oi % 2 == 0 else 90.0 + oi))
        names, gt = [], []
        for k in range(LINEMOD_TEST_LINES[oi]):
            fid = 3 * k + oi                                     # frame ids with gaps, like the real lists
            name = "%04d" % fid
            names.append(name)
            hh, ww = int(rng.integers(24, 130)), int(rng.integers(30, 170))
            r0, c0 = int(rng.integers(5, h - hh - 5)), int(rng.integers(5, w - ww - 5))
            inside = (((yy - r0 - hh / 2) / (hh / 2)) ** 2 + ((xx - c0 - ww / 2) / (ww / 2)) ** 2) < 1
            rgb = (rng.integers(0, 60, (h, w, 3)) + 90).astype(np.uint8)
            rgb[inside] = (CLASS_COLOURS[oi % len(CLASS_COLOURS)] * 0.8).astype(np.uint8) + rng.integers(0, 40, (int(inside.sum()), 3)).astype(np.uint8)
            depth = np.full((h, w), 1100, np.uint16) + (xx // 40).astype(np.uint16)
            depth[inside] = (900 + 25 * np.sin(xx[inside] / 17.0) + 15 * np.cos(yy[inside] / 13.0)).astype(np.uint16)
            depth[rng.random((h, w)) < 0.03] = 0
            Image.fromarray(rgb).save(os.path.join(d, "rgb", name + ".png"), compress_level=1)
            Image.fromarray(depth).save(os.path.join(d, "depth", name + ".png"), compress_level=1)
            mask = np.repeat((inside.astype(np.uint8) * 255)[:, :, None], 3, axis=2)
            Image.fromarray(mask).save(os.path.join(d, "mask", name + ".png"))
            lab = np.zeros((h, w), np.uint8)
            if obj in LINEMOD_EVAL_OBJECTS:
                # the segmentation result: a 16 x 24 window of the object (the rest cut off) with a hole -- between 250 and 500 valid
                # pixels, so `choose` keeps every one of them and its wrap pad repeats only the first
                wr, wc = r0 + hh // 2 - 8, c0 + ww // 2 - 12
                lab[wr:wr + 16, wc:wc + 24] = inside[wr:wr + 16, wc:wc + 24] * 255
                lab[wr + 7:wr + 9, wc + 11:wc + 13] = 0                                       # a hole
                br, bc = (r0 + hh + 40) % (h - 12), (c0 + ww + 60) % (w - 12)
                lab[br:br + 6, bc:bc + 9] = 255                                               # an extra blob, far from the object
                lab[5:9, 5:30] = 128                                                          # another value: not the object
                # and one far point, the last of the window in raster order: the confidence head answers it with a maximum that stands
                # clear of the second (tests/test_linemod_host.py::test_eval_fixture_guard)
                lab[wr + 15, wc + 23] = 255
                depth[wr + 15, wc + 23] = 63000
                Image.fromarray(depth).save(os.path.join(d, "depth", name + ".png"), compress_level=1)
            Image.fromarray(lab).save(os.path.join(seg, name + "_label.png"))
            R = rigid(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3, 3), (0, 0, 0))[:3, :3]
            z = 900.0
            t = [float((c0 + ww / 2 - 325.2611) * z / 572.4114), float((r0 + hh / 2 - 242.04899) * z / 573.57043), z]
            bb = [c0 + int(rng.integers(-6, 7)), r0 + int(rng.integers(-6, 7)), ww + int(rng.integers(-8, 9)), hh + int(rng.integers(-8, 9))]
            recs = [(obj, R, t, bb)]
            if obj == 2:                                         # several objects are annotated in object 2's frames; its own is not first
                recs.insert(0, (5, rigid(0.3, -0.2, 1.0, (0, 0, 0))[:3, :3], [10.0, -20.0, 1000.0], [30, 40, 50, 60]))
            gt.append("%d:\n" % fid + "".join(
                "- cam_R_m2c: [%s]\n  cam_t_m2c: [%s]\n  obj_bb: [%s]\n  obj_id: %d\n"
                % (", ".join("%.8f" % v for v in Rm.flatten()), ", ".join("%.8f" % v for v in tm), ", ".join("%d" % v for v in b4), oid)
                for oid, Rm, tm, b4 in recs))
        with open(os.path.join(d, "gt.yml"), "w") as f:
            f.write("".join(gt))
        with open(os.path.join(d, "test.txt"), "w") as f:
            f.write("".join(n + "\n" for n in names))
        with open(os.path.join(d, "train.txt"), "w") as f:
            f.write("".join(n + "\n" for n in names[:2]))
        frames_of[obj] = names
    with open(os.path.join(root, "models", "models_info.yml"), "w") as f:
        f.write("".join(info))
    return frames_of


YCB_CLASSES = ["%03d_object" % (k + 1) for k in range(21)]
# entries of the tree below, by what they are there for
YCB_REAL_A, YCB_REAL_B, YCB_CAM2, YCB_SMALL, YCB_NONE = ("data/0001/000001", "data/0001/000002", "data/0061/000001", "data/0001/000003",
                                                         "data/0001/000004")
YCB_SYN_MULTI, YCB_SYN_SINGLE, YCB_SYN_COVER = "data_syn/000000", "data_syn/000001", "data_syn/000002"
YCB_EDGE, YCB_SYN_HOLE = "data/0001/000005", "data_syn/000003"    # the over-1000 test of a front candidate at its threshold
YCB_TRAIN = [YCB_REAL_A, YCB_REAL_B, YCB_CAM2, YCB_SYN_MULTI, YCB_SYN_SINGLE, YCB_SMALL]
YCB_TRAIN_REJECTING = [YCB_REAL_A, YCB_REAL_B, YCB_SYN_SINGLE, YCB_SYN_COVER, YCB_NONE]
YCB_TRAIN_THRESHOLD = [YCB_REAL_B, YCB_EDGE, YCB_SYN_HOLE]
YCB_TEST = [YCB_REAL_A, YCB_CAM2, YCB_REAL_B]
YCB_FAR_DEPTH = 15000
# The classes of the test-list entries are those whose confidence head, with the seeded weights posenet_state_dict(21, 0), leaves at least
# 1e-3 between its best pixel and the next on these shapes; the heads of others (2, 3, 8, 16, 20 ...) saturate and give no frame a margin.
# Classes 13, 19 and 21 are among the symmetric five.
# rois (class, x1, y1, x2, y2) beyond the objects': a class PoseCNN's labels hold no pixel of, a roi of no height
YCB_LOST_ROIS = {YCB_REAL_A: [(17, 400.0, 100.0, 470.0, 160.0)], YCB_CAM2: [(7, 300.0, 200.0, 360.0, 201.0)]}
# (class, 'e' ellipse | 'r' rectangle, first row, rows, first column, columns) per entry, painted in this order
YCB_OBJECTS = {
    YCB_REAL_A: [(1, "e", 0, 130, 0, 170), (9, "e", 200, 60, 300, 50), (5, "r", 300, 3, 400, 17), (21, "r", 350, 5, 100, 10)],
    YCB_REAL_B: [(11, "r", 100, 40, 200, 40), (19, "r", 200, 80, 300, 80), (4, "e", 390, 90, 520, 120)],
    YCB_CAM2: [(7, "e", 150, 100, 0, 90), (13, "e", 60, 70, 400, 110), (15, "e", 300, 120, 250, 60)],
    YCB_SMALL: [(21, "r", 350, 5, 100, 10), (5, "r", 300, 3, 400, 17)],
    YCB_NONE: [(21, "r", 350, 5, 100, 10)],
    YCB_SYN_MULTI: [(3, "e", 40, 50, 50, 60), (9, "e", 215, 30, 310, 30), (12, "e", 380, 60, 500, 80)],
    YCB_SYN_SINGLE: [(6, "e", 100, 80, 100, 90)],
    YCB_SYN_COVER: [(13, "r", 0, 480, 0, 330), (14, "r", 0, 480, 330, 310)],
    YCB_EDGE: [(19, "r", 200, 80, 300, 80), (2, "r", 100, 40, 100, 40)],
    YCB_SYN_HOLE: [(13, "r", 0, 480, 0, 330), (14, "r", 0, 480, 330, 310)],
}
# (first row, rows, first column, columns) left unlabelled after the objects are painted: as a front, YCB_SYN_HOLE uncovers 25 x 40 = 1000
# pixels inside class 19 of YCB_REAL_B and YCB_EDGE, and one more pixel that only YCB_EDGE labels
YCB_HOLES = {YCB_SYN_HOLE: [(200, 25, 300, 40), (110, 1, 110, 1)]}


def ycb_tree(root, seed=0):
    """A small YCB_Video_Dataset tree (480 x 640 frames): `data/0001/...` and `data/0061/...` (the second camera), `data_syn/...`, each entry
    with `-color.png`, `-depth.png`, `-label.png` and `-meta.mat` (`cls_indexes`, `poses` [3,4,n], `factor_depth` as uint16);
    `models/<class>/points.xyz` for 21 classes (2600 points and more, within 7 cm); `results_PoseCNN_RSS2018/%06d.mat` for the test list;
    and three config directories with `classes.txt` and the lists: `dataset_config` (YCB_TRAIN, YCB_TEST), `dataset_config_rejecting`
    (YCB_TRAIN_REJECTING: every front candidate is skipped or rejected) and `dataset_config_threshold` (YCB_TRAIN_THRESHOLD: the only front
    candidate leaves exactly 1000 labelled pixels of one frame and 1001 of the other).  What the entries hold, YCB_OBJECTS:
      YCB_REAL_A     an object with pixels in row 0 and in column 0, one with exactly 51 valid pixels and one with exactly 50;
      YCB_REAL_B     objects with extents of exactly 40 and 80, one with pixels in row 479 and in column 639;
      YCB_CAM2       video 61: the second camera; an object with a pixel in column 0;
      YCB_SMALL      the 51-pixel object behind the 50-pixel one (the object draw repeats; `choose` wraps); YCB_NONE: the 50-pixel one only;
      YCB_SYN_MULTI  three classes over a bright background, so that the composite onto a real frame wraps modulo 256;
      YCB_SYN_SINGLE one class: the front candidate that is skipped; YCB_SYN_COVER: two classes over the whole frame: as a front it leaves
                     no labelled pixel, so it is rejected;
      YCB_SYN_HOLE   the same two classes with YCB_HOLES left open: as a front it leaves exactly 1000 labelled pixels of YCB_REAL_B
                     (rejected: not more than 1000) and exactly 1001 of YCB_EDGE (accepted).
    The function asserts the border pixels and the two counts.  Deterministic in `seed`.  Shared by tools/gen_golden_ycb.py (which runs the REFERENCE's PoseDataset on it) and the YCB tests.
    -> {"config": dir, "config_rejecting": dir, "config_threshold": dir, "toolbox": dir}"""
    import os
    import scipy.io as scio
    from PIL import Image
    rng = np.random.default_rng([78, int(seed)])
    h, w = 480, 640
    yy, xx = np.mgrid[0:h, 0:w]
    for k, name in enumerate(YCB_CLASSES):
        os.makedirs(os.path.join(root, "models", name), exist_ok=True)
        pts = rng.uniform(-1, 1, (2600 + 11 * k, 3)) * [0.05 + 0.001 * k, 0.04, 0.03 + 0.002 * k]
        with open(os.path.join(root, "models", name, "points.xyz"), "w") as f:
            f.write("".join("%.6f %.6f %.6f\n" % tuple(p) for p in pts))
    frames = {}
    for line, objects in YCB_OBJECTS.items():
        syn = line.startswith("data_syn")
        os.makedirs(os.path.join(root, os.path.dirname(line)), exist_ok=True)
        cam = (323.7872, 279.6921, 1077.836, 1078.189) if line == YCB_CAM2 else (312.9869, 241.3109, 1066.778, 1067.487)
        label = np.zeros((h, w), np.uint8)
        rgb = (rng.integers(0, 60, (h, w, 3)) + (150 if line == YCB_SYN_MULTI else 90)).astype(np.uint8)
        depth = np.full((h, w), 11000, np.uint16) + (xx // 40).astype(np.uint16)
        keep = np.zeros((h, w), bool)
        poses = []
        for cls, kind, r0, hh, c0, ww in objects:
            if kind == "e":
                q = ((yy - r0 - hh / 2) / (hh / 2)) ** 2 + ((xx - c0 - ww / 2) / (ww / 2)) ** 2
                inside, ends = q < 1, q == 1
                # the ends of the axes belong to the object, so that it touches its box (and with it the frame's border): painted without
                # pixel noise, so that no other pixel of the tree depends on how many they are
                label[ends] = cls
                rgb[ends] = (CLASS_COLOURS[cls % len(CLASS_COLOURS)] * 0.8).astype(np.uint8)
                depth[ends] = (8000 + 250 * np.sin(xx[ends] / 17.0) + 150 * np.cos(yy[ends] / 13.0)).astype(np.uint16)
            else:
                inside = (yy >= r0) & (yy < r0 + hh) & (xx >= c0) & (xx < c0 + ww)
            label[inside] = cls
            rgb[inside] = (CLASS_COLOURS[cls % len(CLASS_COLOURS)] * 0.8).astype(np.uint8) + rng.integers(0, 40, (int(inside.sum()), 3)).astype(np.uint8)
            depth[inside] = (8000 + 250 * np.sin(xx[inside] / 17.0) + 150 * np.cos(yy[inside] / 13.0)).astype(np.uint16)
            if hh * ww < 100:
                keep |= inside                                   # the 51- and 50-pixel objects keep every depth value
            R = rigid(rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-3, 3), (0, 0, 0))[:3, :3]
            t = [(c0 + ww / 2 - cam[0]) * 0.8 / cam[2], (r0 + hh / 2 - cam[1]) * 0.8 / cam[3], 0.8]
            poses.append(np.concatenate([R, np.array(t)[:, None]], axis=1))
        for r0, hh, c0, ww in YCB_HOLES.get(line, []):
            label[r0:r0 + hh, c0:c0 + ww] = 0
        depth[(rng.random((h, w)) < 0.03) & ~keep] = 0
        Image.fromarray(rgb).save(os.path.join(root, line + "-color.png"), compress_level=1)
        Image.fromarray(depth).save(os.path.join(root, line + "-depth.png"), compress_level=1)
        Image.fromarray(label).save(os.path.join(root, line + "-label.png"))
        scio.savemat(os.path.join(root, line + "-meta.mat"),
                     {"cls_indexes": np.array([[o[0]] for o in objects], np.uint8), "poses": np.stack(poses, axis=2),
                      "factor_depth": np.array([[10000]], np.uint16), "intrinsic_matrix": np.array([[cam[2], 0, cam[0]], [0, cam[3], cam[1]], [0, 0, 1.0]])})
        frames[line] = (label, depth)
    # the fixture holds what its docstring says
    top_left, bottom_right, left = frames[YCB_REAL_A][0], frames[YCB_REAL_B][0], frames[YCB_CAM2][0]
    assert top_left[0].any() and top_left[:, 0].any() and bottom_right[h - 1].any() and bottom_right[:, w - 1].any() and left[:, 0].any()
    uncovered = frames[YCB_SYN_HOLE][0] == 0
    assert int((frames[YCB_REAL_B][0][uncovered] != 0).sum()) == 1000 and int((frames[YCB_EDGE][0][uncovered] != 0).sum()) == 1001
    dirs = {"config": os.path.join(root, "dataset_config"), "config_rejecting": os.path.join(root, "dataset_config_rejecting"),
            "config_threshold": os.path.join(root, "dataset_config_threshold"), "toolbox": os.path.join(root, "YCB_Video_toolbox")}
    # PoseCNN's detections of the test list: a roi a few pixels around every object, and as segmentation a 24 x 32 window of the object
    # with a hole -- between 500 and 1000 valid pixels, so `choose` keeps every one and its wrap pad repeats only the first ones -- plus ONE pixel in the last corner of the roi's crop, on the
    # background behind the object (YCB_FAR_DEPTH = 1.5 m against the object's 0.8 m): the confidence head answers that point with a
    # maximum that stands clear of the second (tests/test_ycb_host.py::test_eval_fixture_guard).  The 51- and 50-pixel objects keep their
    # pixels (no window); YCB_LOST_ROIS adds a roi whose class has no pixel in `labels` and one of no height: lost detections.
    from autoposeestimation_amd.DenseFusion.datasets.ycb.dataset import bbox_from_extents
    os.makedirs(os.path.join(dirs["toolbox"], "results_PoseCNN_RSS2018"), exist_ok=True)
    for now, line in enumerate(YCB_TEST):
        gt, depth = frames[line]
        labels = np.zeros((h, w), np.uint8)
        rois = []
        for cls, kind, r0, hh, c0, ww in YCB_OBJECTS[line]:
            roi = [0.0, float(cls), c0 - 4.5, r0 - 4.5, c0 + ww + 4.5, r0 + hh + 4.5]
            rois.append(roi)
            if hh * ww < 100:
                labels[gt == cls] = cls
                continue
            wr, wc = r0 + hh // 2 - 12, c0 + ww // 2 - 16
            labels[wr:wr + 24, wc:wc + 32][gt[wr:wr + 24, wc:wc + 32] == cls] = cls
            labels[wr + 11:wr + 13, wc + 15:wc + 17] = 0
            rmin, rmax, cmin, cmax = bbox_from_extents(int(roi[3]) + 1, int(roi[5]) - 2, int(roi[2]) + 1, int(roi[4]) - 2)
            assert gt[rmax - 1, cmax - 1] == 0 and labels[rmax - 1, cmax - 1] == 0, (line, cls)
            labels[rmax - 1, cmax - 1] = cls
            depth[rmax - 1, cmax - 1] = YCB_FAR_DEPTH
        for extra in YCB_LOST_ROIS.get(line, []):
            rois.append([0.0] + [float(v) for v in extra])
        Image.fromarray(depth).save(os.path.join(root, line + "-depth.png"), compress_level=1)
        scio.savemat(os.path.join(dirs["toolbox"], "results_PoseCNN_RSS2018", "%06d.mat" % now), {"labels": labels, "rois": np.array(rois, np.float32)})
    for key, train in (("config", YCB_TRAIN), ("config_rejecting", YCB_TRAIN_REJECTING), ("config_threshold", YCB_TRAIN_THRESHOLD)):
        os.makedirs(dirs[key], exist_ok=True)
        with open(os.path.join(dirs[key], "classes.txt"), "w") as f:
            f.write("".join(n + "\n" for n in YCB_CLASSES))
        with open(os.path.join(dirs[key], "train_data_list.txt"), "w") as f:
            f.write("".join(n + "\n" for n in train))
        with open(os.path.join(dirs[key], "test_data_list.txt"), "w") as f:
            f.write("".join(n + "\n" for n in YCB_TEST))
    return dirs


def ycb_poses_files(root, dirs, result_dir, perturb=None, lost=()):
    """`poses` files as tools/eval_ycb.py writes them (`%04d.mat`, [n_rois, 7]: quaternion wxyz, translation) for the test list of a tree made
    by `ycb_tree(root)` (`dirs`: what it returned), taken from the ground truth instead of the networks: row k of frame `now` is the
    ground-truth pose of the object whose class roi k of PoseCNN's file carries, followed by `perturb[(now, k)]` = (Euler angles (rx, ry,
    rz) of `rigid`, translation offset): R_est = R_gt R(angles), t_est = t_gt + offset.  A roi whose class the frame does not hold, and
    every (now, k) of `lost`, is the seven zeros of a lost detection.  -> {(now, k): pose f64[7]} as written"""
    import os
    import scipy.io as scio
    from autoposeestimation_amd.DenseFusion.lib.transformations import quaternion_from_matrix
    perturb = perturb or {}
    os.makedirs(result_dir, exist_ok=True)
    written = {}
    for now, line in enumerate(YCB_TEST):
        rois = np.asarray(scio.loadmat(os.path.join(dirs["toolbox"], "results_PoseCNN_RSS2018", "%06d.mat" % now))["rois"]).reshape(-1, 6)
        meta = scio.loadmat(os.path.join(root, line + "-meta.mat"))
        gt_cls = [int(c) for c in np.asarray(meta["cls_indexes"]).reshape(-1)]
        gt_poses = np.asarray(meta["poses"], np.float64).reshape(3, 4, -1)
        poses = np.zeros((rois.shape[0], 7))
        for k in range(rois.shape[0]):
            cls = int(rois[k, 1])
            if cls in gt_cls and (now, k) not in lost:
                rt = gt_poses[:, :, gt_cls.index(cls)]
                angles, offset = perturb.get((now, k), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
                T = np.eye(4)
                T[:3, :3] = rt[:, :3] @ rigid(angles[0], angles[1], angles[2], (0, 0, 0))[:3, :3]
                poses[k, :4] = quaternion_from_matrix(T, True)
                poses[k, 4:] = rt[:, 3] + np.asarray(offset, np.float64)
            written[(now, k)] = poses[k].copy()
        scio.savemat(os.path.join(result_dir, "%04d.mat" % now), {"poses": poses})
    return written


# ---- the label-quality test's three directory trees (experiments/gt_test.py:12-14,49-57) ---------------------------------------------
GT_TEST_ROTATIONS = ("foreground", "foreground180")


def gt_test_tree(root, classes=("Disk", "Joint"), n=3, h=12, w=16, seed=0):
    """`experiments/data/gt_test`, `label_generator/data` and `data_generation/data` under `root` for `n` samples per class and rotation
    directory: the hand annotation is a random rectangle, saved as an RGBA PNG (red and opaque inside, transparent black outside: what
    annotation tools write); `new_pred`, `pred` and `gen` are its vertical, horizontal and double flip, each with a different edge of
    the rectangle trimmed (so the two one-sided counts of a pair differ), saved as `L` PNGs with the values 255, 255 and 1; the colour
    frame is uniform noise.  Deterministic in `seed`.  -> {(cls, rot): [sample ids]}"""
    import os
    from PIL import Image
    ids = {}
    for cls in classes:
        for rot in GT_TEST_ROTATIONS:
            gt_dir = os.path.join(root, "experiments", "data", "gt_test", cls, rot)
            lab_dir = os.path.join(root, "label_generator", "data", cls, rot)
            img_dir = os.path.join(root, "data_generation", "data", cls, rot)
            for d in (gt_dir, lab_dir, img_dir):
                os.makedirs(d, exist_ok=True)
            ids[(cls, rot)] = []
            for i in range(n):
                sid = "%06d" % i
                rng = _rng(seed, "gt_test/%s/%s/%s" % (cls, rot, sid))
                r0, c0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
                r1, c1 = int(rng.integers(r0 + max(1, h // 3), h + 1)), int(rng.integers(c0 + max(1, w // 3), w + 1))
                mask = np.zeros((h, w), dtype=bool)
                mask[r0:r1, c0:c1] = True
                rgba = np.zeros((h, w, 4), dtype=np.uint8)
                rgba[mask] = (255, 0, 0, 255)
                Image.fromarray(rgba, "RGBA").save(os.path.join(gt_dir, sid + ".color.mask.0.png"))
                trimmed = []
                for dr0, dc0, dr1, dc1 in ((1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 1, 1)):
                    m = np.zeros((h, w), dtype=bool)
                    m[r0 + dr0:r1 - dr1, c0 + dc0:c1 - dc1] = True
                    trimmed.append(m)
                for kind, lab, value in (("new_pred", trimmed[0][::-1], 255), ("pred", trimmed[1][:, ::-1], 255),
                                         ("gen", trimmed[2][::-1, ::-1], 1)):
                    Image.fromarray(lab.astype(np.uint8) * np.uint8(value), "L").save(os.path.join(lab_dir, "%s.%s.label.png" % (sid, kind)))
                Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(os.path.join(img_dir, sid + ".color.png"))
                ids[(cls, rot)].append(sid)
    return ids

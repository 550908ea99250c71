"""CPU checks of SegNet's device sample path: `SegDataset.draw_params` makes `__getitem__`'s draws in its order, `sample_host` of those
parameters is `__getitem__` bit for bit, csrc/segnet_px.h -- built for the host by tools/check_segnet_px.py -- equals Pillow / numpy
exactly (tests/segnet_samples_reference.py), the job structure has the C layout, and what the builder refuses.  The kernels themselves:
tests/test_gpu_segnet_samples.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import segnet_samples_reference as R
from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))


class _Script:
    """draws that replay a script and record what was asked (as tests/test_segnet_host.py's)"""

    def __init__(self, ints, seed):
        self.ints, self.asked, self.order = list(ints), [], []
        self.g = np.random.default_rng(seed)

    def randint(self, a, b):
        self.asked.append((a, b))
        self.order.append("randint")
        return self.ints.pop(0)

    def uniform(self, a, b):
        self.order.append("uniform")
        return float(self.g.uniform(a, b))

    def shuffle_list(self, x):
        self.order.append("shuffle")
        order = self.g.permutation(len(x))
        x[:] = [x[i] for i in order]

    def normal(self, shape):
        self.order.append("normal%r" % (tuple(shape),))
        return self.g.normal(0.0, 5.0, shape)


@pytest.fixture(scope="module")
def ycb(tmp_path_factory):
    from autoposeestimation_amd import synthetic as S
    root = str(tmp_path_factory.mktemp("ycb_seg_samples"))
    S.ycb_tree(root)
    lines = [S.YCB_REAL_A, S.YCB_SYN_MULTI, S.YCB_REAL_B, S.YCB_CAM2] + [S.YCB_REAL_A] * 9      # 13 lines, 12 of them real
    txt = os.path.join(root, "seg_list.txt")
    with open(txt, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))
    return root, txt, lines


def _dataset(ycb, use_noise, draws=None, **kw):
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation.data_controller import SegDataset
    return SegDataset(ycb[0], ycb[1], use_noise, 7, draws=draws, **kw)


@pytest.mark.parametrize("use_noise,ints", [(False, [0]), (True, [2, 1]), (True, [1, 2, 3]), (False, [1, 1]), (True, [1, 0, 0])])
def test_draw_params_makes_the_draws_of_getitem_in_its_order(ycb, use_noise, ints):
    """real and `data_syn` entries (index 1), with and without use_noise: the same calls in the same order with the same randint ranges,
    and `sample_host` of the drawn parameters is the sample"""
    host = _dataset(ycb, use_noise, _Script(ints, 11))
    want = host[3]
    ds = _dataset(ycb, use_noise, _Script(ints, 11))
    params = ds.draw_params()
    assert ds.draws.order == host.draws.order and ds.draws.asked == host.draws.asked and not ds.draws.ints
    syn = ycb[2][ints[0]].startswith("data_syn")
    assert ds.draws.asked[0] == (0, 3) and (not syn or ds.draws.asked[1] == (0, 2)) and (not use_noise or ds.draws.asked[-1] == (0, 3))
    assert params["index"] == ints[0] and params["flip"] == (ints[-1] if use_noise else None)
    assert ("noise" in params) == syn and ("discarded" in params) == (syn and use_noise)
    if syn:
        assert params["back"] == ints[1] and params["noise"].shape == (3, 480, 640) and params["noise"].dtype == np.float64
    got = ds.sample_host(params)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64


@pytest.mark.parametrize("use_noise", [False, True])
def test_sample_host_of_draw_params_equals_getitem_under_the_global_generators(ycb, use_noise):
    import random
    ds = _dataset(ycb, use_noise)
    seen = set()
    for seed in range(5):
        random.seed(seed)
        np.random.seed(seed)
        want = ds[0]
        state = (random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2])
        random.seed(seed)
        np.random.seed(seed)
        params = ds.draw_params()
        assert (random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2]) == state
        got = ds.sample_host(params)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), seed
        seen.add(ds.is_syn(params["index"]))
    assert seen == {False, True}


def test_blur_weights_are_pillows():
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation import augment as G
    assert G.blur_weights(0.8) == (13198076, 1789570)
    ww, fw = G.blur_weights(0.8)
    assert ww + 2 * fw <= 1 << 24


@pytest.mark.parametrize("h,w", R.SIZES + [(32, 40)])
def test_header_blur_equals_pillow(h, w):
    import check_segnet_px as C
    for seed in range(3):
        rgb = np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(C.host_blur(rgb), R.blur(rgb)), seed
    flat = np.full((h, w, 3), 255, np.uint8)
    assert np.array_equal(C.host_blur(flat), R.blur(flat))


@pytest.mark.parametrize("h,w", R.SIZES)
def test_header_samples_equal_pillow_and_numpy(h, w):
    """each op alone, four ops with the contrast first and last, the four flips, `data_syn` with and without use_noise, a label without a
    zero and one that is all zero -- exact on both outputs"""
    import check_segnet_px as C
    for name, rgb, label, params, back in R.cases(h, w):
        want = R.sample(rgb, label, params, back)
        got = C.host_sample(rgb, label, params, back)
        assert got[0].dtype == np.float32 and got[1].dtype == np.int64
        assert np.array_equal(got[0], want[0]), (name, int((got[0] != want[0]).sum()))
        assert np.array_equal(got[1], want[1]), name


def test_header_is_exact_over_the_synthetic_tree():
    import check_segnet_px as C
    assert C.run(quick=True, verbose=False) == (len(C.BLUR_SIZES), 6)


def test_segnet_job_mirror_has_the_c_layout(tmp_path):
    """the ctypes mirror of `ape_segnet_job` lives next to its one user; same check as tests/test_abi.py makes for the mirrors of _lib.py"""
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation import augment as G
    names = [f[0] for f in G.SegnetJob._fields_]
    src = ["#include <stddef.h>", "#include <stdio.h>", '#include "ape_hip.h"', "int main() {",
           '    printf("%%zu%s\\n", sizeof(ape_segnet_job)%s);' % (" %zu" * len(names), "".join(", offsetof(ape_segnet_job, %s)" % n for n in names)),
           "    return 0;", "}"]
    (tmp_path / "layout.cpp").write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.cpp"), "-o", exe])
    want = "%d%s" % (ctypes.sizeof(G.SegnetJob), "".join(" %d" % getattr(G.SegnetJob, n).offset for n in names))
    assert subprocess.check_output([exe]).decode().split("\n")[0] == want
    assert ctypes.sizeof(G.SegnetJob) == 168 and 16 * 168 + 24 <= 3900          # 16 jobs per launch as kernel arguments


def test_refusals(ycb, tmp_path):
    import shutil
    from PIL import Image
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation import augment as G
    with pytest.raises(ValueError, match="integer radius"):
        G.blur_weights(3.0)
    with pytest.raises(ValueError, match="integer radius"):
        G.make_job((1, 1), 4, 4, {"blur_radius": 2.0}, (1, 1))
    with pytest.raises(ValueError, match="at most one contrast"):
        G.make_job((1, 1), 4, 4, {"ops": [("contrast", 1.1), ("hue", 0.01), ("contrast", 0.9)]})
    with pytest.raises(ValueError, match="flip"):
        G.make_job((1, 1), 4, 4, {"flip": 4})
    # a host tensor: the builder has no CPU path
    host = (torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(_lib.ApeError, match="device tensor"):
        G.build_samples([host], [{}])
    with pytest.raises(_lib.ApeError, match="device"):
        _dataset(ycb, False).batch(1)
    # a tree of its own with one frame of another size and one two-band label
    root = str(tmp_path / "tree")
    shutil.copytree(ycb[0], root)
    lines = ycb[2]
    real_b, cam2 = lines[2], lines[3]
    for kind in ("color", "label"):
        p = "%s/%s-%s.png" % (root, real_b, kind)
        Image.open(p).crop((0, 0, 96, 64)).save(p)
    p = "%s/%s-label.png" % (root, cam2)
    Image.open(p).convert("LA").save(p)
    from autoposeestimation_amd.DenseFusion.vanilla_segmentation.data_controller import SegDataset
    txt = os.path.join(root, "seg_list.txt")
    ds = SegDataset(root, txt, False, 7, device="cpu")
    real = {"index": 0, "ops": None, "flip": None}
    with pytest.raises(ValueError, match="share one size"):
        ds.batch(2, params=[real, dict(real, index=2)])
    noise = np.zeros((3, 480, 640))
    with pytest.raises(ValueError, match="background .* share one size"):
        ds.batch(1, params=[{"index": 1, "ops": [], "flip": None, "back": 2, "ops_back": [], "noise": noise}])
    with pytest.raises(ValueError, match="one-band 8-bit label"):
        ds.batch(1, params=[dict(real, index=3)])
    with pytest.raises(ValueError, match="parameter sets"):
        ds.batch(2, params=[real])
    with pytest.raises(_lib.ApeError, match="device tensor"):           # frames on the host
        ds.batch(1, params=[real])

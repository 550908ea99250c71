"""The YCB-Video data set's host path (DenseFusion/datasets/ycb/dataset.py) without a GPU: the file lists and `sample_host` against
tests/golden/ycb_dataset.npz (made by running the reference's class, tools/gen_golden_ycb.py) bit for bit, `get_bbox` against values
recorded from the reference's function, the refusals, the layout of the job struct, the host check of csrc/ycb_px.h, and the guard of the
eval fixture that tests/test_gpu_ycb.py relies on."""
import ctypes
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import ycb_reference as R
from conftest import REPO
from autoposeestimation_amd import synthetic as S

GOLD = R.GOLD


@pytest.mark.parametrize("name", list(R.CASES))
def test_lists_and_samples_equal_the_reference(name):
    """plain: a real frame, the second camera, a `data_syn` frame composited onto a real background (uint8 wrap) with float64 noise, the
    51-pixel object (wrap pad); noise: jitter, translation noise and front candidates; reject: all five candidates skipped or rejected,
    more valid pixels than num_pt = 60; threshold: the one front candidate leaves exactly 1000 labelled pixels of the first frame (rejected
    five times) and exactly 1001 of the second (accepted); refine: 2600 model points"""
    assert int(GOLD["tree_seed"]) == R.TREE_SEED
    random.seed(int(GOLD["seed"]))
    np.random.seed(int(GOLD["seed"]))
    ds = R.dataset(name, reference_rng=True)
    assert [len(ds), ds.len_real, ds.len_syn, ds.get_num_points_mesh()] == GOLD[name + "_len"].tolist()
    for key in ("list", "real", "syn"):
        assert getattr(ds, key) == GOLD["%s_%s" % (name, key)].tolist(), key
    assert ds.get_sym_list() == GOLD[name + "_sym"].tolist() == [12, 15, 18, 19, 20]
    assert [len(ds.cld[k]) for k in sorted(ds.cld)] == GOLD[name + "_cld_len"].tolist() and sorted(ds.cld) == list(range(1, 22))
    sizes = set()
    for k, idx in enumerate(GOLD[name + "_order"].tolist()):
        got, want = ds[idx], R.golden_sample(name, k)
        assert len(got) == 6
        for g, w, what in zip(got, want, R.NAMES):
            assert g.dtype == w.dtype and torch.equal(g, w), "%s sample %d (%d): %s differs" % (name, k, idx, what)
        sizes.add(tuple(got[2].shape[1:]))
    assert len(sizes) > 1 or name in ("reject", "threshold")
    assert got[4].shape[0] == (2600 if name == "refine" else 500)


def test_the_front_is_accepted_above_1000_pixels_only():
    """`> 1000`, not `>=`: the one candidate uncovers exactly 1000 labelled pixels of YCB_REAL_B and exactly 1001 of YCB_EDGE, all but one
    of them a 25 x 40 block of class 19.  Accepted, it leaves that block as the only object a sample can be about (crop 40 x 40);
    rejected, class 19 keeps its 80 x 80 extent.  The golden (the reference's decision) and the seeded host path both show it."""
    ds = R.dataset("threshold", seed=2)
    assert ds.syn == [S.YCB_SYN_HOLE] and ds.list[:2] == [S.YCB_REAL_B, S.YCB_EDGE] and GOLD["threshold_order"].tolist() == [0, 1]
    hole = np.array(Image.open(os.path.join(ds.root, S.YCB_SYN_HOLE + "-label.png")))
    assert np.unique(hole).tolist() == [0, 13, 14]
    for i, left in ((0, 1000), (1, 1001)):
        lab = np.array(Image.open(os.path.join(ds.root, ds.list[i] + "-label.png")))
        assert len((lab * ((hole != 13) * (hole != 14))).nonzero()[0]) == left
    for rejected, accepted in ((R.golden_sample("threshold", 0), R.golden_sample("threshold", 1)), (ds[0], ds[1])):
        assert int(accepted[5]) == 18 and tuple(accepted[2].shape) == (3, 40, 40)
        assert int(rejected[5]) in (3, 10) or (int(rejected[5]) == 18 and tuple(rejected[2].shape) == (3, 80, 80))


def test_the_cases_hold_what_they_are_there_for():
    """the golden's composite does wrap, its front is accepted / rejected where the case says so, and the second camera is in use"""
    ds = R.dataset("plain")
    k = GOLD["plain_order"].tolist().index(ds.list.index(S.YCB_SYN_MULTI))
    assert "plain_%d_img" % k in GOLD                            # noise: stored as float32
    syn = np.array(Image.open(os.path.join(ds.root, S.YCB_SYN_MULTI + "-color.png"))).astype(np.int64)
    lab = np.array(Image.open(os.path.join(ds.root, S.YCB_SYN_MULTI + "-label.png")))
    back = np.array(Image.open(os.path.join(ds.root, S.YCB_REAL_A + "-color.png"))).astype(np.int64)
    assert ((syn + back)[lab == 0] > 255).mean() > 0.3           # a bright background under `mask_back`: the sum wraps
    assert ds._cam(S.YCB_CAM2) == (323.7872, 279.6921, 1077.836, 1078.189) and ds._cam(S.YCB_REAL_A)[0] == 312.9869
    assert ds._cam(S.YCB_SYN_MULTI)[0] == 312.9869 and ds._cam("data/0059/000001")[0] == 312.9869 and ds._cam("data/0060/000001")[0] == 323.7872
    assert (ds.minimum_num_pt, ds.front_num, ds.num_pt_mesh_small, ds.num_pt_mesh_large) == (50, 2, 500, 2600)
    small = R.dataset("plain", seed=1)
    s = small[small.list.index(S.YCB_SMALL)]                     # 51 valid pixels: the pad wraps, the 50-pixel object is never drawn
    assert int(s[5]) == 4 and len(set(s[1].view(-1).tolist())) == 51 and s[1].view(-1)[:51].tolist() == s[1].view(-1)[51:102].tolist()


def test_get_bbox_equals_the_reference():
    from autoposeestimation_amd.DenseFusion.datasets.ycb.dataset import bbox_from_extents, border_list, get_bbox
    assert border_list == GOLD["border_list"].tolist()
    boxes = GOLD["bbox_in"].tolist()
    assert any(b[0] == 0 for b in boxes) and any(b[1] == 480 for b in boxes) and any(b[2] == 0 for b in boxes) and any(b[3] == 640 for b in boxes)
    assert any(b[1] - b[0] == 40 for b in boxes) and any(b[3] - b[2] == 80 for b in boxes) and any(b[1] - b[0] == 41 for b in boxes)
    for (r0, r1, c0, c1), want in zip(boxes, GOLD["bbox_out"].tolist()):
        m = np.zeros((480, 640), bool)
        m[r0:r1, c0:c1] = True
        got = get_bbox(m)
        assert [int(v) for v in got] == want == [int(v) for v in bbox_from_extents(r0, r1 - 1, c0, c1 - 1)], (r0, r1, c0, c1)
        rmin, rmax, cmin, cmax = got
        assert 0 <= rmin <= r0 and r1 <= rmax <= 480 and 0 <= cmin <= c0 and c1 <= cmax <= 640         # the crop holds the mask
        assert (rmax - rmin) % 40 == 0 and (cmax - cmin) % 40 == 0
    m = np.zeros((480, 640), np.uint8)
    m[440:480, 600:640] = 9
    assert get_bbox(m) == (440, 480, 600, 640)                   # clamps to 480 / 640, not LineMOD's 479 / 639


def _copy_tree(tmp_path):
    root, dirs = R.tree()
    new = str(tmp_path / "ycb")
    shutil.copytree(root, new)
    return new, os.path.join(new, "dataset_config")


def test_refusals(tmp_path):
    from autoposeestimation_amd.DenseFusion.datasets.ycb.dataset import PoseDataset
    ds = R.dataset("reject", seed=0)
    with pytest.raises(ValueError, match=S.YCB_NONE):            # no object above 50 pixels: the reference draws forever
        ds[ds.list.index(S.YCB_NONE)]
    assert "loops forever" in " ".join(PoseDataset.sample_host.__doc__.split())
    with pytest.raises(ValueError, match="mode"):
        PoseDataset("eval", 500, False, ds.root, 0.0, False, dataset_config_dir=os.path.dirname(ds.path))
    with pytest.raises(ValueError, match="missing"):
        ds.sample_host(0, {})
    root, config = _copy_tree(tmp_path)
    lab = np.array(Image.open(os.path.join(root, S.YCB_REAL_A + "-label.png")))
    lab[0, 0] = 22
    Image.fromarray(lab).save(os.path.join(root, S.YCB_REAL_A + "-label.png"))
    Image.fromarray(np.zeros((240, 320, 3), np.uint8)).save(os.path.join(root, S.YCB_REAL_B + "-color.png"))
    Image.fromarray(np.zeros((480, 640, 4), np.uint8)).save(os.path.join(root, S.YCB_CAM2 + "-color.png"))
    bad = PoseDataset("train", 500, False, root, 0.0, False, dataset_config_dir=config, device="cpu")
    with pytest.raises(ValueError, match="class 22"):            # at decode time, on the host array
        bad._resident(S.YCB_REAL_A)
    with pytest.raises(ValueError, match="480 x 640"):
        bad._resident(S.YCB_REAL_B)
    with pytest.raises(ValueError, match="480 x 640"):
        bad._resident(S.YCB_CAM2)
    r = bad._resident(S.YCB_SYN_MULTI)                           # a good entry: the sorted class list is cached with it
    assert r[3] == [0, 3, 9, 12] and r[0].dtype == torch.uint8 and r[1].dtype == torch.uint16 and bad._resident(S.YCB_SYN_MULTI) is r


def test_ycb_job_mirror_has_the_c_layout(tmp_path):
    """the ctypes mirrors of `ape_ycb_job`, `ape_ycb_jitter` and `ape_ycb_pair` live next to their one user; same check as tests/test_abi.py
    makes for the mirrors of _lib.py"""
    from autoposeestimation_amd.DenseFusion.datasets.ycb import augment as G
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "ape_hip.h"', "int main() {"]
    want = []
    for c_name, cls in (("ape_ycb_job", G.YcbJob), ("ape_ycb_jitter", G.YcbJitter), ("ape_ycb_pair", G.YcbPair)):
        names = [f[0] for f in cls._fields_]
        src.append('    printf("%%zu%s\\n", sizeof(%s)%s);' % (" %zu" * len(names), c_name, "".join(", offsetof(%s, %s)" % (c_name, n) for n in names)))
        want.append("%d%s" % (ctypes.sizeof(cls), "".join(" %d" % getattr(cls, n).offset for n in names)))
    src += ["    return 0;", "}"]
    (tmp_path / "layout.cpp").write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-I", os.path.join(REPO, "include"), str(tmp_path / "layout.cpp"), "-o", exe])
    assert subprocess.check_output([exe]).decode().split("\n")[:-1] == want
    assert ctypes.sizeof(G.YcbJob) == 240 and 16 * 240 + 24 <= 3900          # 16 jobs per launch as kernel arguments


def test_ycb_px_header_is_exact_on_the_host():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_ycb_px
    assert check_ycb_px.run(quick=True, verbose=False) == 6


def test_eval_fixture_guard():
    """the inputs of tests/test_gpu_ycb.py's driver tests: with the seeded weights, every counted detection of the synthetic tree leaves at
    least 1e-3 between the confidence of its best pixel and that of the next (the wrap pad repeats pixels, so the gap is taken between
    pixels), and no cloud reaches beyond 1.5 m -- a condition on the inputs, so that the arg-max does not hang on the last bits.  Random
    heads do not give such a gap by themselves: the tree plants it (`synthetic.ycb_tree`)."""
    res = R.restated_eval(S.posenet_state_dict(21, 0), S.refiner_state_dict(21, 0))
    assert [len(fr) for fr in res] == [5, 4, 3]
    counted = [r for fr in res for r in fr if r is not None]
    assert len(counted) == 10 and [(now, k) for now, fr in enumerate(res) for k, r in enumerate(fr) if r is None] == [(0, 4), (1, 3)]
    for r in counted:
        assert r["gap"] >= 1e-3 and r["cloud_max"] <= 1.5 + 1e-6, r
    assert {r["cls"] for r in counted} == {1, 4, 5, 7, 9, 11, 13, 15, 19, 21}


def test_roi_get_bbox_and_lost_crops():
    from autoposeestimation_amd.DenseFusion.tools import eval_ycb as D
    assert D.get_bbox([0, 3, 99.5, 49.5, 180.5, 131.5]) == (50, 130, 99, 179)        # 80 rows stay 80; 79 columns go up to 80
    assert D.get_bbox([0, 3, -10.0, -10.0, 30.0, 30.0]) == (0, 40, 0, 40) and D.get_bbox([0, 3, 600.0, 440.0, 660.0, 500.0]) == (400, 480, 560, 640)
    assert D.crop_ok((0, 40, 0, 40)) and not D.crop_ok(D.get_bbox([0, 7, 300.0, 200.0, 360.0, 201.0]))     # a roi of no height
    assert (D.num_points, D.num_obj, D.cam_scale) == (1000, 21, 10000.0)
    doc = " ".join(D.__doc__.split())
    assert "ZeroDivisionError" in doc and "numpy 2 raises `ValueError`" in doc

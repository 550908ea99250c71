"""The label-quality test (experiments/gt_test.py, select_samples_for_gt_test.py) on the host: `compute_IoU` and the numpy restatement
of the count kernel's contract against every value recorded from the reference (tests/golden/gt_test.npz, tools/gen_golden_gt_test.py),
ratios bit-equal; the numpy path of the driver against the reference's recorded stdout; the sample drawer against its recorded
meta.json.  No GPU."""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import golden

import gt_test_reference as R
from autoposeestimation_amd import synthetic as S
from autoposeestimation_amd.experiments import gt_test as G
from autoposeestimation_amd.experiments import select_samples_for_gt_test as SEL

GOLD = golden("gt_test")
CLASSES = [str(c) for c in GOLD["classes"]]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("gt_test_tree"))
    S.gt_test_tree(root)
    return root


def _planes(root, rel):
    cls, rot, sid = rel.split("/")
    paths = G._sample_paths(root, cls, rot, sid)
    return [G._decode(paths[k]) for k in G.PLANES]


def test_compute_iou_and_the_restatement_equal_the_recorded_edge_values():
    eg, el, want, raises = GOLD["edge_gt"], GOLD["edge_label"], GOLD["edge_out"], GOLD["edge_raises"]
    assert raises.sum() == 3 and not raises[3] and (eg[3] != 0).all() and (el[3] != 0).all()      # both empty, gt empty, label empty; all fg
    for k in range(len(eg)):
        a, b = eg[k].copy(), el[k].copy()
        counts = R.pair_counts(np.stack([a, b])[None], [(0, 1)])[0, 0]
        assert counts.sum() == a.size
        if raises[k]:
            with pytest.raises(ZeroDivisionError):
                G.compute_IoU(a, b)
            with pytest.raises(ZeroDivisionError):
                R.ratios(counts)
        else:
            got = G.compute_IoU(a, b)
            assert all(isinstance(v, float) for v in got)
            assert got == want[k].tolist() and R.ratios(counts) == want[k].tolist()
            assert tuple(counts) == G.pixel_counts(a, b)
        assert np.array_equal(a, eg[k]) and np.array_equal(b, el[k])                              # the inputs are not modified


def test_zero_division_where_each_denominator_is_zero():
    z, s = np.zeros((3, 4), np.uint8), np.eye(3, 4, dtype=np.uint8) * 255
    for a, b in ((z, z), (z, s), (s, z)):          # tp + fp + fn, tp + fp, tp + fn
        with pytest.raises(ZeroDivisionError):
            G.compute_IoU(a, b)
    assert G.compute_IoU(s, s) == [1.0, 1.0, 1.0, 1.0]
    with pytest.raises(ValueError):
        G.compute_IoU(z, np.zeros((3, 5), np.uint8))


def test_every_sample_of_the_tree_equals_the_recorded_values(tree):
    want = GOLD["per_sample"]
    for i, rel in enumerate(GOLD["samples"]):
        planes = np.stack(_planes(tree, str(rel)))
        counts = R.pair_counts(planes[None], G.PAIRS)[0]
        for k, (a, b) in enumerate(G.PAIRS):
            assert G.compute_IoU(planes[a], planes[b]) == want[i, k].tolist(), (rel, G.NAMES[k])
            assert R.ratios(counts[k]) == want[i, k].tolist(), (rel, G.NAMES[k])
    assert (want[:, :, 2] != want[:, :, 3]).any()          # "precision" and "recall" differ somewhere: their swap would show


def test_host_driver_prints_the_recorded_stdout(tree, capsys):
    res = G.main(tree, classes=CLASSES, use_cuda=False)
    got = capsys.readouterr().out
    want = str(GOLD["stdout"])
    assert got.split("\n") == want.split("\n")
    assert ["/".join(o) for o in res["order"]] == [str(s) for s in GOLD["samples"]]
    assert [[s[n] for n in G.NAMES] for s in res["per_sample"]] == GOLD["per_sample"].tolist()
    assert res["final"] is res["directories"][-1] and res["final"]["total_samples"] == len(GOLD["samples"])
    assert len(res["directories"]) == 2 * len(CLASSES)
    per = GOLD["per_sample"]
    for k, n in enumerate(G.NAMES):
        assert res["final"]["mean"][n] == np.mean(per[:, k], axis=0).tolist()
        assert res["final"]["iou_ge_0.5"][n] == float((per[:, k, 0] >= 0.5).sum()) / len(per)
    assert sum(line.endswith(" ") for line in got.split("\n")) == 4 * len(res["directories"])      # the reference's trailing blanks


def test_default_class_order_is_sorted_and_small_batches_change_nothing(tree, capsys):
    a = G.main(tree, use_cuda=False, batch=1)
    b = G.main(tree, classes=CLASSES, use_cuda=False, batch=5)
    capsys.readouterr()
    assert sorted(CLASSES) == CLASSES and a == b


def test_host_overlays_equal_the_restatement(tree, tmp_path, capsys):
    out = str(tmp_path / "overlays")
    timing = {}
    G.main(tree, classes=CLASSES[:1], rotations=("foreground",), use_cuda=False, overlay_dir=out, timing=timing)
    capsys.readouterr()
    assert timing["samples"] == 3 and 0 <= timing["decode_seconds"] and timing["seconds"] > 0
    for sid in ("000000", "000001", "000002"):
        planes = np.stack(_planes(tree, "%s/foreground/%s" % (CLASSES[0], sid)))
        rgb = np.array(Image.open(os.path.join(tree, "data_generation", "data", CLASSES[0], "foreground", sid + ".color.png")).convert("RGB"))
        for tag, pa, pb in G.OVERLAYS:
            got = np.array(Image.open(os.path.join(out, CLASSES[0], "foreground", "%s.%s.png" % (sid, tag))))
            assert np.array_equal(got, R.pair_blend(rgb[None], planes[None], (pa, 2), (pb, 0), 0.7, 1.0 - 0.7)[0])
    assert set(os.listdir(os.path.join(out, CLASSES[0], "foreground"))) == {"%06d.%s.png" % (i, t) for i in range(3) for t, _, _ in G.OVERLAYS}


def test_driver_errors_name_the_sample(tmp_path, capsys):
    root = str(tmp_path)
    S.gt_test_tree(root, classes=("Disk",), n=2)
    lab = os.path.join(root, "label_generator", "data", "Disk", "foreground180")
    with pytest.raises(ValueError, match="batch"):
        G.main(root, use_cuda=False, batch=0)
    Image.fromarray(np.zeros((12, 16), np.uint8)).save(os.path.join(lab, "000001.gen.label.png"))
    with pytest.raises(ZeroDivisionError, match=r"foreground180.000001\.color\.mask\.0\.png"):
        G.main(root, use_cuda=False)
    Image.fromarray(np.ones((12, 17), np.uint8)).save(os.path.join(lab, "000001.gen.label.png"))
    with pytest.raises(ValueError, match=r"foreground180.000001\.color\.mask\.0\.png.*differ in size"):
        G.main(root, use_cuda=False)
    capsys.readouterr()


def test_use_cuda_without_a_device_is_a_clear_error(tree, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="use_cuda=False"):
        G.main(tree, use_cuda=True)


def test_engine_wrappers_check_their_arguments():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    labels = torch.zeros(1, 2, 3, 4, dtype=torch.uint8)
    rgb = torch.zeros(1, 3, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        E.label_pair_counts(labels[0], [(0, 1)])
    with pytest.raises(ValueError):
        E.label_pair_counts(labels, [])
    with pytest.raises(ValueError):
        E.label_pair_counts(labels, [(0, 1, 1)])
    with pytest.raises(_lib.ApeError, match="no CPU fallback"):
        E.label_pair_counts(labels, [(0, 1)])
    with pytest.raises(ValueError):
        E.label_pair_blend(rgb, labels[:, :, :2], (0, 2), (1, 0), 0.7, 0.3)
    with pytest.raises(ValueError):
        E.label_pair_blend(rgb[..., :2], labels, (0, 2), (1, 0), 0.7, 0.3)
    with pytest.raises(_lib.ApeError, match="no CPU fallback"):
        E.label_pair_blend(rgb, labels, (0, 2), (1, 0), 0.7, 0.3)


def test_the_two_symbols_are_in_the_library_and_the_table():
    from autoposeestimation_amd import _lib
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ape_label_pair_counts_u8", "ape_label_pair_blend_u8"):
        assert hasattr(h, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 18


def test_sample_drawer_writes_the_recorded_meta_and_reuses_it(tmp_path, capsys):
    root = str(tmp_path)
    S.gt_test_tree(root, n=10)
    classes = [str(c) for c in GOLD["select_classes"]]
    want = json.loads(str(GOLD["select_meta"]))
    meta = SEL.main(root, classes=classes, rng=np.random.RandomState(5))
    gt_path = os.path.join(root, "experiments", "data", "gt_test")
    with open(os.path.join(gt_path, "meta.json")) as f:
        on_disk = json.load(f)
    assert meta == want and on_disk == want and want["p"] == 0.2
    saved = sorted(os.path.relpath(os.path.join(d, f), gt_path) for d, _, fs in os.walk(gt_path) for f in fs if f.endswith(".color.png"))
    assert saved == [str(s) for s in GOLD["select_saved"]] and len(saved) == 2 * 2 * len(classes)
    first = saved[0]
    src = Image.open(os.path.join(root, "data_generation", "data", first))
    assert np.array_equal(np.array(Image.open(os.path.join(gt_path, first))), np.array(src.convert("RGB")))
    again = SEL.main(root, p=0.9, classes=classes, rng=np.random.RandomState(99))          # the lists and p of meta.json are reused
    assert again == want
    assert "cls 0/%d, rot 0/2" % len(classes) in capsys.readouterr().out


def test_the_reference_import_names_resolve_after_install_dropin():
    import autoposeestimation_amd as A
    assert "experiments.gt_test" not in A.DROPIN_MODULES and "experiments.select_samples_for_gt_test" not in A.DROPIN_MODULES
    A.install_dropin()
    for name in ("gt_test", "select_samples_for_gt_test"):
        mod = importlib.import_module("experiments." + name)
        assert mod.__file__.startswith(os.path.dirname(A.__file__)) and callable(mod.main)
    assert callable(importlib.import_module("experiments.gt_test").compute_IoU)

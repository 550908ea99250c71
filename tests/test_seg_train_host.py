"""CPU side of the segmentor's training surface: the NumPy path of ConfusionMatrix / IoU against the reference's own numbers
(tests/golden/seg_train_metrics.npz, tools/gen_golden_segtrain.py), the refusals, and the checkpoint dict of segmentation/train.py."""
import os

import numpy as np
import pytest
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd import synthetic as S
from autoposeestimation_amd.segmentation import utils as U
from autoposeestimation_amd.segmentation.train import checkpoint

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "seg_train_metrics.npz"))
METRIC_CASES = [str(c) for c in GOLD["metric_cases"]]


def _metric(name):
    k = int(GOLD["metric_%s_k" % name])
    ign = [int(i) for i in GOLD["metric_%s_ignore" % name]]
    m = U.IoU(k, normalized=bool(GOLD["metric_%s_normalized" % name]), ignore_index=None if not ign else (ign[0] if len(ign) == 1 else ign))
    return m, int(GOLD["metric_%s_adds" % name])


@pytest.mark.parametrize("name", METRIC_CASES)
@pytest.mark.parametrize("kind", ["torch_cpu", "numpy"])
def test_numpy_metric_matches_the_reference(name, kind):
    m, n = _metric(name)
    for i in range(n):
        pred, tgt = GOLD["metric_%s_pred%d" % (name, i)], GOLD["metric_%s_target%d" % (name, i)]
        if kind == "torch_cpu":
            m.add(torch.from_numpy(pred), torch.from_numpy(tgt))
        else:                                 # ConfusionMatrix.add on flattened arrays, as IoU.add feeds it
            p = pred.transpose(0, 2, 3, 1).reshape(-1, pred.shape[1]) if pred.ndim == 4 else pred.reshape(-1)
            m.conf_metric.add(p, tgt.reshape(-1))
    iou, miou = m.value()
    conf = m.conf_metric.value()
    want = GOLD["metric_%s_conf" % name]
    if m.conf_metric.normalized:
        np.testing.assert_allclose(conf, want, rtol=1e-6)
    else:
        assert conf.dtype == np.int64
        np.testing.assert_array_equal(conf, want)
    np.testing.assert_allclose(iou, GOLD["metric_%s_iou" % name], rtol=1e-6, equal_nan=True)
    np.testing.assert_allclose(miou, GOLD["metric_%s_miou" % name], rtol=1e-6, equal_nan=True)


def test_confusion_counts_do_not_wrap_at_int32():
    m = U.ConfusionMatrix(2)
    m.conf[0, 0] = (1 << 31) - 1
    m.add(np.zeros(4, np.int64), np.zeros(4, np.int64))
    assert int(m.value()[0, 0]) == (1 << 31) + 3


def test_metric_refuses_out_of_range_and_mismatched_inputs():
    m = U.ConfusionMatrix(3)
    with pytest.raises(ValueError, match="target values"):
        m.add(np.zeros(4, np.int64), np.array([0, 1, 3, 0]))
    with pytest.raises(ValueError, match="predicted values"):
        m.add(np.array([0, -1, 0, 0]), np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="do not match"):
        m.add(np.zeros(4, np.int64), np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="size of confusion matrix"):
        m.add(np.zeros((4, 5), np.float32), np.zeros(4, np.int64))
    iou = U.IoU(3)
    with pytest.raises(ValueError, match="dimension"):
        iou.add(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="ignore_index"):
        U.IoU(3, ignore_index=1.5)


def test_loss_refuses_host_tensors_and_bad_shapes():
    logits, lab = torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    with pytest.raises(_lib.ApeError, match="device"):
        U.jaccard_loss(lab, logits)
    with pytest.raises(TypeError):
        U.jaccard_loss(lab.numpy(), logits)


def test_imagenet_unet_refuses_to_train_without_weights():
    m = U.get_model("Unet", {"encoder_name": "resnet18", "encoder_weights": "imagenet", "activation": "softmax", "in_channels": 3,
                             "classes": 3})
    m.train()
    assert all(p.requires_grad for p in m.parameters())
    with pytest.raises(RuntimeError, match="load a checkpoint"):
        m(torch.zeros(1, 3, 32, 32))
    m.eval()
    assert not any(p.requires_grad for p in m.parameters())


def test_checkpoint_dict_has_the_reference_keys():
    cfg = {"encoder_name": "resnet18", "encoder_weights": None, "activation": "softmax", "in_channels": 3, "classes": 3}
    m = U.get_model("Unet", cfg)
    m.load_state_dict(S.unet_state_dict("resnet18", 3, 3, 3))
    cp = checkpoint(m, 4, 0.5, [0.1], [0.9], [0.5], [0.8], {"lr": 1e-4}, "Unet", cfg)
    assert set(cp) == {"state_dict", "epoch", "iou", "train_iou_scores", "train_losses", "train_loss", "valid_iou_scores", "valid_losses",
                       "training_config", "name", "segmentation_config"}
    assert cp["train_loss"] == 0.9 and cp["name"] == "Unet" and cp["segmentation_config"] == cfg
    back = U.get_model(cp["name"], cp["segmentation_config"])
    back.load_state_dict(cp["state_dict"])


def test_package_names_shadow_the_reference_copy():
    import autoposeestimation_amd.segmentation.metrics as M
    assert U.jaccard_loss is M.jaccard_loss and U.IoU is M.IoU and U.ConfusionMatrix is M.ConfusionMatrix

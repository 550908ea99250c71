"""CPU checks of the smp Unet drop-in (segmentation/unet.py): constructor, state-dict keys and loading, the BN fold, the synthetic weights
against the fp64 restatement (tests/unet_reference.py), and a static ISA audit of csrc/unet.hip's kernels."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import unet_reference as R  # noqa: E402
from autoposeestimation_amd import engine as E  # noqa: E402
from autoposeestimation_amd import synthetic as S  # noqa: E402
from autoposeestimation_amd.segmentation.utils import get_model  # noqa: E402

CFG = {"encoder_name": "resnet34", "encoder_weights": "imagenet", "activation": "softmax", "in_channels": 3, "classes": 13}
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _want_keys(in_ch, classes, blocks=(3, 4, 6, 3)):
    """the smp 0.1.3 Unet-resnet34 key list of the issue, written out independently of synthetic.unet_spec"""
    k = {"encoder.conv1.weight": (64, in_ch, 7, 7)}
    k.update({"encoder.bn1." + n: (64,) for n in BN})
    cin = 64
    for li, (pl, n) in enumerate(zip((64, 128, 256, 512), blocks), 1):
        for b in range(n):
            p = "encoder.layer%d.%d." % (li, b)
            k[p + "conv1.weight"] = (pl, cin, 3, 3)
            k[p + "conv2.weight"] = (pl, pl, 3, 3)
            for bn in ("bn1", "bn2"):
                k.update({p + bn + "." + n: (pl,) for n in BN})
            if b == 0 and li > 1:
                k[p + "downsample.0.weight"] = (pl, cin, 1, 1)
                k.update({p + "downsample.1." + n: (pl,) for n in BN})
            cin = pl
    for i, (cin, cout) in enumerate(zip((768, 384, 192, 128, 32), (256, 128, 64, 32, 16))):
        for c, ci in (("conv1", cin), ("conv2", cout)):
            k["decoder.blocks.%d.%s.0.weight" % (i, c)] = (cout, ci, 3, 3)
            k.update({"decoder.blocks.%d.%s.1.%s" % (i, c, n): (cout,) for n in BN})
    k["segmentation_head.0.weight"] = (classes, 16, 3, 3)
    k["segmentation_head.0.bias"] = (classes,)
    return {n: (tuple(s) if n.split(".")[-1] != "num_batches_tracked" else ()) for n, s in k.items()}


@pytest.mark.parametrize("in_ch,classes", [(3, 13), (7, 2)])
def test_state_dict_keys_and_shapes(in_ch, classes):
    m = get_model("Unet", dict(CFG, in_channels=in_ch, classes=classes))
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    want = _want_keys(in_ch, classes)
    assert len(want) == 278 and got == want
    assert set(S.unet_state_dict("resnet34", 0, in_ch, classes)) == set(want)


def test_strict_loading_rejects_missing_and_extra_keys():
    m = get_model("Unet", CFG)
    sd = S.unet_state_dict("resnet34", 0, 3, 13)
    m.load_state_dict(sd)
    bad = dict(sd)
    del bad["decoder.blocks.2.conv1.1.running_var"]
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)
    bad = dict(sd)
    bad["module.segmentation_head.0.bias"] = bad["segmentation_head.0.bias"]
    with pytest.raises(RuntimeError):
        m.load_state_dict(bad)


def test_reference_checkpoint_round_trip(tmp_path):
    """the dict main.py / segmentation/__init__.py save ({'state_dict', 'name', 'segmentation_config', ...}), read back as main.py:609-610 does"""
    sd = S.unet_state_dict("resnet34", 3, 3, 13)
    path = str(tmp_path / "Unet_resnet34.ckpt")
    torch.save({"state_dict": sd, "name": "Unet", "segmentation_config": dict(CFG), "epoch": 7}, path)
    cp = torch.load(path, map_location="cpu")
    m = get_model(cp["name"], cp["segmentation_config"])
    m.load_state_dict(cp["state_dict"])
    back = m.state_dict()
    assert list(back) == list(sd)               # smp's key order (module registration order)
    for k, v in sd.items():
        assert torch.equal(back[k].cpu(), v), k


def test_imagenet_config_constructs_but_refuses_to_run_unloaded():
    m = get_model("Unet", CFG)
    assert m.encoder_weights == "imagenet"
    with pytest.raises(RuntimeError, match="load"):
        m.plan()


@pytest.mark.parametrize("cfg,exc,match", [({"encoder_name": "resnet50"}, NotImplementedError, "encoder 'resnet50'"),
                                           ({"in_channels": 9}, NotImplementedError, "in_channels"),
                                           ({"activation": "sigmoid"}, NotImplementedError, "activation 'sigmoid'"),
                                           ({"encoder_weights": "ssl"}, NotImplementedError, "encoder_weights 'ssl'"),
                                           ({"classes": 0}, ValueError, "classes"),
                                           ({"decoder_channels": (128, 64, 32, 16, 8)}, NotImplementedError, "decoder_channels"),
                                           ({"encoder_depth": 4}, NotImplementedError, "encoder_depth"),
                                           ({"decoder_attention_type": "scse"}, NotImplementedError, "attention")])
def test_bad_configs_are_refused(cfg, exc, match):
    get_model("Unet", CFG)                          # the base config constructs: what is refused is the changed keyword
    with pytest.raises(exc, match=match):
        get_model("Unet", dict(CFG, **cfg))


def test_linknet_still_raises():
    with pytest.raises(NotImplementedError):
        get_model("LinkNet", CFG)


@pytest.mark.parametrize("enc", ["resnet18", "resnet34"])
def test_other_activations_and_encoders_construct(enc):
    for act in (None, "identity", "softmax", "softmax2d"):
        get_model("Unet", dict(CFG, encoder_name=enc, activation=act))


def test_bn_fold_matches_conv_then_batchnorm():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 24, 9, 11, generator=g, dtype=torch.float64)
    w = torch.randn(32, 24, 3, 3, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(32, generator=g, dtype=torch.float64) + 0.5, torch.randn(32, generator=g, dtype=torch.float64)
    mean, var = torch.randn(32, generator=g, dtype=torch.float64), torch.rand(32, generator=g, dtype=torch.float64) + 0.1
    want = F.batch_norm(F.conv2d(x, w, None, 1, 1), mean, var, gamma, beta, False, 0.0, 1e-5)
    wf, bf = E.bn_fold(w, gamma, beta, mean, var, 1e-5)
    got = F.conv2d(x, wf, bf, 1, 1)
    assert (got - want).abs().max() <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("enc,in_ch,classes", [("resnet34", 3, 13), ("resnet34", 7, 2), ("resnet18", 3, 5)])
def test_synthetic_weights_give_bounded_logits(enc, in_ch, classes):
    sd = S.unet_state_dict(enc, 1, in_ch, classes)
    x = torch.randn(1, in_ch, 64, 96, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out = R.logits(sd, x, enc)
    assert torch.isfinite(out).all()
    assert 1e-2 < float(out.abs().max()) < 1e3
    assert float(out.std()) > 1e-2                 # not collapsed to a constant


def test_unet_kernels_isa_has_no_wait_findings_spills_or_src1_swizzles():
    import isa_audit
    if not os.path.exists(isa_audit.HIPCC):
        pytest.skip("hipcc not present")
    out_dir = os.path.join(REPO, "autoposeestimation_amd", "csrc", "build", "isa_audit")
    asm = isa_audit.compile_to_asm(os.path.join(isa_audit.CSRC, "unet.hip"), out_dir)
    syms = [s for s in isa_audit.kernel_symbols(asm) if "unet_conv3x3_kernel" in s]
    assert len(syms) == 16                          # nsplit {1,3} x ups {0,1} x (3 ReLU tiles + head)
    for s in syms:
        r = isa_audit.audit(asm, s)
        assert r["n_mfma"] >= 8
        assert not r["findings"], (s, r["findings"])
        meta = r["meta"]
        assert meta["vgpr_spill_count"] == 0 and meta["private_segment_fixed_size"] == 0, (s, meta)
        assert meta["vgpr_count"] <= 256, (s, meta)
        assert isa_audit.pk_src1_swizzles(asm, s, asm_only=False) == [], s
        assert isa_audit.mfma_asm_hazards(asm, s) == [], s
    for s in isa_audit.kernel_symbols(asm):
        assert isa_audit.pk_src1_swizzles(asm, s, asm_only=False) == [], s

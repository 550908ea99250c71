"""GPU checks of csrc/unet.hip (the smp-Unet decoder conv and its fused head) at its edge shapes, against the float64 sum of the kernel's
own products (tests/conv_products_reference.py) on the inputs of tests/conv_edge_cases.py -- whose guards and branch-reached claims
tests/test_conv_edges_host.py proves on the CPU.  Operands go through the C ABI directly: they are wider than the channels read (the
engine wrapper refuses a wide `a`), the unread channels are NaN, and every output is a window of a sentinel-filled buffer with guards.

Bounds, all derived, none measured:
 * outputs / logits: |got - restatement| <= d = 2e-6 max(1, max|restatement|).  The restatement holds the kernel's very products, so
   only the float32 accumulation order remains (the project's bar for "same products, other summation order"); the plain float64
   convolution of the unsplit operands is held at test_gpu_conv.py's TOL (5e-5 bf16x3, 2e-2 bf16).
 * labels: equal to the float64 first-maximum label wherever the two largest first-softmax probabilities (duplicated classes counted
   once) differ by at least tau.  Let g be the float64 logit gap of the top class to a rival; p_top - p_rival = p_top (1 - exp(-g)) <= g,
   so a probability gap >= tau means g >= tau, and on the device g' >= g - 2 d.
     one softmax:  the head names the lowest class whose exp(l - max) is exactly 1; its fast exponential may return 1 for arguments above
       -2^-22 (a true expf: 2^-25).  g' > 2^-22 leaves the maximum alone:            tau = 2 d + 2^-22.
     two softmaxes: it names the lowest class whose exp(p - p_max) is exactly 1.  p_top - p_rival >= (1 - exp(-g')) / C >= g' / (2 C)
       (p_top >= 1 / C; g' <= 1), each device probability is within 2^-20 of that (a few ulp of a value <= 1), so the computed difference
       exceeds 2^-22 when g' > 2 C (2 * 2^-20 + 2^-22):                            tau = 2 d + 2 C (2^-19 + 2^-22).
   At most 0.1 % of a case's pixels may lie inside the band; every case here has fewer than 1000 pixels, so none does (asserted on the
   restatement by the host test and again here).
 * scores: softmax is 1/2-Lipschitz in the max norm (sum_j |dp_i / dl_j| = 2 p_i (1 - p_i) <= 1/2), once per softmax, plus the 1e-5
   relative that test_gpu_segpost_edges.py derives for seg_head_finish:  |score - float64| <= d / 2 (d / 4 after two) + 1e-5 score.
 * a duplicated class's higher index never appears: its logit is bit-identical to the lower one's."""
import numpy as np
import pytest
import torch

import conv_edge_cases as EC
import conv_products_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1


def _mods():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    return _lib, E


def _guarded(t=None, shape=None, fill=0.0, dtype=torch.float32):
    """a device buffer with EC.GUARD elements of `fill` in front of and behind it -> (the buffer, the whole allocation)"""
    n = int(np.prod(shape if t is None else t.shape))
    whole = torch.full((n + 2 * EC.GUARD,), fill, dtype=dtype, device=DEV)
    view = whole[EC.GUARD:EC.GUARD + n].view(tuple(shape if t is None else t.shape))
    if t is not None:
        view.copy_(t)
    return view, whole


def _guards_intact(whole, fill):
    return bool((whole[:EC.GUARD] == fill).all() and (whole[-EC.GUARD:] == fill).all())


def _operands(name, nsplit):
    _, E = _mods()
    c = EC.unet_case(name)
    a, b, w, bias = EC.unet_inputs(name)
    da, _ = _guarded(a, fill=EC.NAN)
    db = _guarded(b, fill=EC.NAN)[0] if b is not None else None
    # (the layer only packs the weights: the kernel is called through the C ABI below)
    conv = E.Conv(w, bias, 1, 1, 1, E.ACT_NONE if c["head"] else E.ACT_RELU, device=DEV, precision=EC.PRECISION[nsplit])
    return c, da, db, conv


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", list(EC.UNET_CONV_CASES))
def test_unet_conv_against_its_own_products(name, nsplit):
    _lib, _ = _mods()
    c, da, db, conv = _operands(name, nsplit)
    M, Cout, yoff, ldy = c["M"], c["Cout"], c["yoff"], c["ldy"]
    y, whole = _guarded(shape=(M, ldy), fill=EC.Y_SENTINEL)
    _lib.call.ape_unet_conv3x3_bf16(_lib.dptr(da), c["lda"], c["C1"], _lib.dptr(db), c["ldb"], c["C2"], _lib.dptr(conv.wp), _lib.dptr(conv.bias),
                                    _lib.dptr(y), ldy, yoff, c["B"], c["H"], c["W"], Cout, c["ups"], nsplit, _lib.stream_ptr())
    torch.cuda.synchronize()
    whole = whole.cpu()
    y = whole[EC.GUARD:-EC.GUARD].view(M, ldy)
    got = y[:, yoff:yoff + Cout].double()
    assert not torch.isnan(whole).any()
    assert _guards_intact(whole, EC.Y_SENTINEL) and (y[:, :yoff] == EC.Y_SENTINEL).all() and (y[:, yoff + Cout:] == EC.Y_SENTINEL).all()
    want = EC.unet_expected(name, nsplit).clamp(min=0)
    plain = EC.unet_expected(name, 0).clamp(min=0)
    r = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
    r0 = float((got - plain).abs().max()) / max(1.0, float(plain.abs().max()))
    print("unet conv %s nsplit %d: %.3g of the output scale against its own products (%.0f %% of the bar), %.3g against the plain conv"
          % (name, nsplit, r, 100 * r / EC.BAR, r0))
    assert r <= EC.BAR, (name, nsplit, r)
    assert r0 <= EC.TOL[nsplit], (name, nsplit, r0)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", list(EC.UNET_HEAD_CASES))
def test_unet_head_against_float64(name, nsplit):
    _lib, _ = _mods()
    c, da, db, conv = _operands(name, nsplit)
    M, C = c["M"], c["Cout"]
    logits = EC.unet_expected(name, nsplit)
    higher = torch.tensor([d != k for k, d in enumerate(c["dup"] or range(C))])
    for dsm in (0, 1):
        label, lwhole = _guarded(shape=(M,), fill=EC.LABEL_SENTINEL, dtype=torch.uint8)
        score, swhole = _guarded(shape=(M,), fill=EC.SCORE_SENTINEL)
        _lib.call.ape_unet_conv3x3_seghead_bf16(_lib.dptr(da), c["lda"], c["C1"], _lib.dptr(db), c["ldb"], c["C2"], _lib.dptr(conv.wp),
                                                _lib.dptr(conv.bias), C, _lib.dptr(label), _lib.dptr(score), c["B"], c["H"], c["W"], c["ups"],
                                                nsplit, dsm, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert _guards_intact(lwhole, EC.LABEL_SENTINEL) and _guards_intact(swhole, EC.SCORE_SENTINEL)
        label, score = label.cpu().long(), score.cpu().double()
        assert not torch.isnan(score).any() and int(label.max()) < C
        want_label, want_score, p1 = R.head(logits, dsm)
        unsure = R.top2_gap(p1, c["dup"]) < EC.label_band(logits, C, dsm)
        assert int(unsure.sum()) <= EC.EXCLUDE_CAP * M, (name, nsplit, dsm)
        assert torch.equal(label[~unsure], want_label[~unsure]), (name, nsplit, dsm)
        assert not higher[label].any(), (name, nsplit, dsm)                    # a duplicated class's higher index never appears
        err = (score - want_score).abs()
        bound = EC.score_bound(logits, want_score, dsm)
        r = float((err / bound).max())
        print("unet head %s nsplit %d softmax x%d: score error %.3g = %.1f %% of the bound, %d of %d pixels left out of the label comparison"
              % (name, nsplit, 1 + dsm, float(err.max()), 100 * r, int(unsure.sum()), M))
        assert r <= 1.0, (name, nsplit, dsm, r)


def test_wide_operands_give_the_bits_of_narrow_ones():
    """lda > C1 and ldb > C2 change addresses only"""
    _lib, E = _mods()
    for name in ("nc4np4_ups_2x10x14_c16+16_o80", "nc2np8_full_3x13x17_c16+16_o32", "nc1np8_full_3x13x17_c48+16_o16"):
        c, da, db, conv = _operands(name, 3)
        y, _ = _guarded(shape=(c["B"], c["H"], c["W"], c["ldy"]), fill=EC.Y_SENTINEL)
        _lib.call.ape_unet_conv3x3_bf16(_lib.dptr(da), c["lda"], c["C1"], _lib.dptr(db), c["ldb"], c["C2"], _lib.dptr(conv.wp), _lib.dptr(conv.bias),
                                        _lib.dptr(y), c["ldy"], c["yoff"], c["B"], c["H"], c["W"], c["Cout"], c["ups"], 3, _lib.stream_ptr())
        narrow = E.unet_conv3x3(conv, da[..., :c["C1"]].contiguous(), db[..., :c["C2"]].contiguous(), ups=bool(c["ups"]))
        assert torch.equal(y[..., c["yoff"]:c["yoff"] + c["Cout"]], narrow), name


def test_engine_refuses_a_layer_whose_activation_the_kernel_would_ignore():
    """the conv epilogue is bias + ReLU, the head's is the bare bias: any other `act` of the layer would be silently dropped"""
    _, E = _mods()
    g = torch.Generator().manual_seed(0)
    a = torch.randn(1, 4, 6, 16, generator=g).to(DEV)
    w = torch.randn(16, 16, 3, 3, generator=g) / 12
    for act in (E.ACT_NONE, E.ACT_PRELU, E.ACT_SIGMOID):
        conv = E.Conv(w, torch.zeros(16), 1, 1, 1, act, alpha=0.25, device=DEV, precision="bf16x3")
        with pytest.raises(ValueError):
            E.unet_conv3x3(conv, a, None, ups=False)
    for act in (E.ACT_RELU, E.ACT_PRELU, E.ACT_SIGMOID):
        conv = E.Conv(w[:13], torch.zeros(13), 1, 1, 1, act, alpha=0.25, device=DEV, precision="bf16x3")
        with pytest.raises(ValueError):
            E.unet_conv3x3_seghead(conv, a, None, ups=False)
    relu = E.Conv(w, torch.zeros(16), 1, 1, 1, E.ACT_RELU, device=DEV, precision="bf16x3")
    none = E.Conv(w[:13], torch.zeros(13), 1, 1, 1, E.ACT_NONE, device=DEV, precision="bf16x3")
    assert E.unet_conv3x3(relu, a, None, ups=False).shape == (1, 4, 6, 16)
    assert E.unet_conv3x3_seghead(none, a, None, ups=False)[0].shape == (1, 4, 6)


def test_rejections():
    _lib, E = _mods()
    L, p, st = _lib.lib(), _lib.dptr, _lib.stream_ptr()
    f = torch.zeros(4096, device=DEV)
    u8 = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    wp = torch.zeros(1 << 16, dtype=torch.bfloat16, device=DEV)

    def conv(lda=16, C1=16, ldb=0, C2=0, ldy=16, yoff=0, H=4, W=4, Cout=16, ups=0, nsplit=3):
        return L.ape_unet_conv3x3_bf16(p(f), lda, C1, p(f), ldb, C2, p(wp), None, p(f), ldy, yoff, 1, H, W, Cout, ups, nsplit, st)

    assert conv() == 0
    assert conv(lda=12) == EINVAL and conv(lda=18) == EINVAL and conv(C1=24, lda=24) == EINVAL           # lda < C1, lda % 4, C1 % 16
    assert conv(C2=16, ldb=12) == EINVAL and conv(C2=8, ldb=8) == EINVAL
    assert conv(ldy=16, yoff=4) == EINVAL and conv(ldy=18) == EINVAL and conv(ldy=24, yoff=2) == EINVAL
    assert conv(Cout=24, ldy=24) == EINVAL and conv(nsplit=2) == EINVAL and conv(ups=2) == EINVAL
    assert conv(H=3, ups=1) == EINVAL and conv(W=5, ups=1) == EINVAL                                      # an up-sampled map has even sides
    for C in (0, 17):
        assert L.ape_unet_conv3x3_seghead_bf16(p(f), 16, 16, None, 0, 0, p(wp), None, C, p(u8), p(f), 1, 4, 4, 0, 3, 1, st) == EINVAL
    torch.cuda.synchronize()

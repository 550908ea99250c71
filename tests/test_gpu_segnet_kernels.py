"""GPU checks of csrc/segnet.hip: the 2x2 max-pool that records its winners, the unpool, the gather and the pixel-wise cross-entropy.

Pool / unpool / gather do no arithmetic, so every comparison is `torch.equal` against torch's CPU `F.max_pool2d(return_indices=True)` /
`F.max_unpool2d(output_size=...)`; torch's flat index is compared as (2 * oh + code // 2) * W + 2 * ow + code % 2.  The cross-entropy is held
to float64 `F.cross_entropy` with bars from fp32 arithmetic: the loss within 1e-6 * max(1, max|logit|), the gradient within 1e-6 / n_valid."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
EINVAL = -1

SHAPES = [(1, 2, 2, 4), (1, 1, 1, 4), (1, 5, 7, 4), (2, 3, 2, 8), (1, 2, 9, 12), (3, 30, 40, 512), (1, 15, 20, 64), (1, 64, 96, 64)]
KINDS = ["normal", "ties01", "zero", "negative", "signed_zero", "nan_one", "nan_many", "inf"]


def _mods():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    return _lib, E


def _values(kind, shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if kind == "ties01":
        x = (torch.rand(shape, generator=g) < 0.5).float()
    elif kind == "zero":
        x = torch.zeros(shape)
    elif kind == "negative":
        x = -x.abs() - 0.5
    elif kind == "signed_zero":
        x = torch.where(torch.rand(shape, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    elif kind == "nan_one":              # about one NaN per window
        x = torch.where(torch.rand(shape, generator=g) < 0.25, torch.tensor(float("nan")), x)
    elif kind == "nan_many":
        x = torch.where(torch.rand(shape, generator=g) < 0.7, torch.tensor(float("nan")), x)
    elif kind == "inf":
        r = torch.rand(shape, generator=g)
        x = torch.where(r < 0.4, torch.tensor(float("-inf")), torch.where(r > 0.8, torch.tensor(float("inf")), x))
    return x.contiguous()


def _same(a, b):
    """bit-equal, NaN positions included (NaN payloads are not compared: a NaN is copied, never made)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    za = torch.where(na, torch.zeros_like(a), a)
    zb = torch.where(nb, torch.zeros_like(b), b)
    return torch.equal(na, nb) and torch.equal(za, zb) and torch.equal(torch.signbit(za), torch.signbit(zb))


def _torch_pool(x):
    """x NHWC cpu -> (y NHWC, flat index NHWC) of torch's CPU pool (which refuses a map that pools to nothing: empty then)"""
    b, h, w, c = x.shape
    if h < 2 or w < 2:
        return torch.zeros(b, h // 2, w // 2, c), torch.zeros(b, h // 2, w // 2, c, dtype=torch.int64)
    y, idx = F.max_pool2d(x.permute(0, 3, 1, 2).contiguous(), 2, 2, return_indices=True)
    return y.permute(0, 2, 3, 1).contiguous(), idx.permute(0, 2, 3, 1).contiguous()


def _flat_index(code, w):
    b, ho, wo, c = code.shape
    oh = torch.arange(ho).view(1, ho, 1, 1)
    ow = torch.arange(wo).view(1, 1, wo, 1)
    k = code.long()
    return (2 * oh + k // 2) * w + 2 * ow + k % 2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_unpool_gather_equal_torch(shape):
    _, E = _mods()
    b, h, w, c = shape
    for n, kind in enumerate(KINDS):
        x = _values(kind, shape, 100 + n)
        want_y, want_idx = _torch_pool(x)
        y, code = E.maxpool2x2_idx(x.cuda())
        y2, code2 = E.maxpool2x2_idx(x.cuda())
        assert tuple(y.shape) == tuple(code.shape) == (b, h // 2, w // 2, c)
        assert _same(y.cpu(), want_y), (kind, "pool values")
        assert torch.equal(_flat_index(code.cpu(), w), want_idx), (kind, "pool indices")
        assert _same(y.cpu(), y2.cpu()) and torch.equal(code, code2), (kind, "two launches")

        # the unpool of other values at those positions: every element written (the buffer starts as a sentinel inside engine's
        # torch.empty only by luck, so write one here through the raw entry point)
        _lib, _ = _mods()
        v = _values("negative" if kind == "negative" else "normal", tuple(y.shape), 200 + n).cuda()
        out = torch.full(shape, 12345.0, device="cuda")
        rc = _lib.lib().ape_max_unpool2x2_nhwc_f32(_lib.dptr(v), _lib.dptr(code), _lib.dptr(out), b, h, w, c, None)
        assert rc == 0
        if y.numel():
            want_x = F.max_unpool2d(v.cpu().permute(0, 3, 1, 2).contiguous(), want_idx.permute(0, 3, 1, 2).contiguous(), 2, 2,
                                    output_size=(h, w)).permute(0, 2, 3, 1).contiguous()
        else:
            want_x = torch.zeros(shape)
        assert torch.equal(out.cpu(), want_x), (kind, "unpool")
        assert torch.equal(E.max_unpool2x2(v, code, h, w), out), (kind, "unpool, two launches")

        # the gather names the winner again, and picks any other tensor at the same places
        assert _same(E.gather2x2(x.cuda(), code).cpu(), want_y), (kind, "gather of x")
        z = _values("normal", shape, 300 + n)
        want_g = torch.gather(z.permute(0, 3, 1, 2).reshape(b, c, h * w), 2, want_idx.permute(0, 3, 1, 2).reshape(b, c, (h // 2) * (w // 2)))
        want_g = want_g.reshape(b, c, h // 2, w // 2).permute(0, 2, 3, 1)
        assert torch.equal(E.gather2x2(z.cuda(), code).cpu(), want_g), (kind, "gather")


def test_tie_nan_and_inf_rules_by_hand():
    _, E = _mods()
    nan, inf = float("nan"), float("inf")
    #          window (0,0) (0,1) (1,0) (1,1)      -> code
    cases = [([0.0, 0.0, 0.0, 0.0], 0), ([1.0, 2.0, 2.0, 1.0], 1), ([0.0, -0.0, 0.0, -0.0], 0), ([-0.0, 0.0, 0.0, 0.0], 0),
             ([-inf, -inf, -inf, -inf], 0), ([nan, 5.0, 1.0, 2.0], 0), ([5.0, nan, 9.0, 2.0], 1), ([1.0, nan, nan, 7.0], 2),
             ([1.0, 2.0, 3.0, nan], 3), ([inf, inf, 1.0, 2.0], 0), ([-3.0, -2.0, -1.0, -1.0], 2)]
    x = torch.zeros(1, 2, 2 * len(cases), 4)
    for i, (win, _) in enumerate(cases):
        x[0, :, 2 * i:2 * i + 2, :] = torch.tensor(win).view(2, 2, 1)
    _, code = E.maxpool2x2_idx(x.cuda())
    assert code.cpu()[0, 0, :, 0].tolist() == [k for _, k in cases]
    want_y, want_idx = _torch_pool(x)
    assert torch.equal(_flat_index(code.cpu(), x.shape[2]), want_idx)


@pytest.mark.parametrize("shape", [(1, 5, 7, 4), (2, 6, 4, 8), (1, 15, 20, 64)], ids=lambda s: "x".join(map(str, s)))
def test_tape_equals_torch_autograd(shape):
    """unpool(f(pool(x))) through the tape against torch's CPU autograd on the same graph: exact (the rules only move values)"""
    from autoposeestimation_amd import autograd as A
    b, h, w, c = shape
    x = _values("ties01", shape, 7) + 0.25 * _values("normal", shape, 8).round()
    scale = _values("normal", (b, h // 2, w // 2, c), 9)
    cot = _values("normal", shape, 10)

    xd = x.cuda().requires_grad_(True)
    sd = scale.cuda().requires_grad_(True)
    y, code = A.maxpool2x2_idx(xd)
    out = A.MaxUnpool2x2Fn.apply(y * sd, code, h, w)
    out.backward(cot.cuda())

    xc = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    sc = scale.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yc, idx = F.max_pool2d(xc, 2, 2, return_indices=True)
    outc = F.max_unpool2d(yc * sc, idx, 2, 2, output_size=(h, w))
    outc.backward(cot.permute(0, 3, 1, 2).contiguous())
    assert torch.equal(out.detach().cpu(), outc.detach().permute(0, 2, 3, 1))
    assert torch.equal(xd.grad.cpu(), xc.grad.permute(0, 2, 3, 1))
    assert torch.equal(sd.grad.cpu(), sc.grad.permute(0, 2, 3, 1))


def test_window_kernels_refuse_bad_arguments():
    _lib, _ = _mods()
    h = _lib.lib()
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    y = torch.zeros(1, 2, 2, 8, device="cuda")
    k = torch.zeros(1, 2, 2, 8, dtype=torch.uint8, device="cuda")
    p = _lib.dptr
    for fn, args in (("ape_maxpool2x2_idx_nhwc_f32", (p(x), p(y), p(k))), ("ape_max_unpool2x2_nhwc_f32", (p(y), p(k), p(x))),
                     ("ape_gather2x2_nhwc_f32", (p(x), p(k), p(y)))):
        f = getattr(h, fn)
        assert f(*args, 1, 4, 4, 8, None) == 0
        assert f(*args, 1, 4, 4, 6, None) == EINVAL          # C % 4
        assert f(*args, 1, 4, 4, 2, None) == EINVAL
        assert f(*args, -1, 4, 4, 8, None) == EINVAL
        assert f(*args, 1, -4, 4, 8, None) == EINVAL
        assert f(*args, 1 << 15, 1 << 10, 1 << 10, 8, None) == EINVAL      # 2^38 elements
        for i in range(3):
            bad = list(args)
            bad[i] = None
            assert f(*bad, 1, 4, 4, 8, None) == EINVAL       # null
        assert f(*args, 0, 4, 4, 8, None) == 0               # nothing to do
    with pytest.raises(_lib.ApeError):
        from autoposeestimation_amd import engine as E
        E.maxpool2x2_idx(torch.zeros(1, 4, 4, 6, device="cuda"))


# ---- cross-entropy ------------------------------------------------------------------------------------------------------------------------------
def _ce_case(P, C, pad, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, generator=g)
    if kind == "x80":
        x = 80.0 * x
    elif kind == "extremes":
        x = torch.where(torch.rand(P, C, generator=g) < 0.5, torch.tensor(1e4), torch.tensor(-1e4)) + x
    lab = torch.randint(0, C, (P,), generator=g).to(torch.uint8)
    if kind == "one_label":
        lab = torch.full((P,), C - 1, dtype=torch.uint8)
    buf = torch.full((P, C + pad), float("nan"))
    buf[:, :C] = x
    return x, lab, buf.contiguous()


def _check_ce(x, lab, buf, C, bad=()):
    _, E = _mods()
    P = x.shape[0]
    lab = lab.clone()
    for p in bad:
        lab[p] = C + (p % 3)
    keep = torch.ones(P, dtype=torch.bool)
    keep[list(bad)] = False
    n_valid = int(keep.sum())
    xr = x[keep].double().requires_grad_(True)
    want = F.cross_entropy(xr, lab[keep].long())
    want.backward()
    want_d = torch.zeros(P, buf.shape[1], dtype=torch.float64)
    want_d[keep, :C] = xr.grad * 0.5            # g = 0.5
    out, d = E.cross_entropy(buf.cuda(), lab.cuda(), C, g=0.5, want_grad=True)
    out2, d2 = E.cross_entropy(buf.cuda(), lab.cuda(), C, g=0.5, want_grad=True)
    out3, none = E.cross_entropy(buf.cuda(), lab.cuda(), C)
    assert none is None
    assert torch.equal(out, out2) and torch.equal(d, d2) and torch.equal(out, out3), "two launches differ"
    out, d = out.cpu(), d.cpu().double()
    assert out[1].item() == len(bad)
    err = abs(out[0].item() - want.item())
    derr = ((d - want_d).abs().max().item()) * n_valid / 0.5
    print("P %d C %d ld %d: loss err %.3g (bar %.3g), dlogits err * n %.3g" % (P, C, buf.shape[1], err,
                                                                                 1e-6 * max(1.0, x.abs().max().item()), derr))
    assert err <= 1e-6 * max(1.0, x.abs().max().item())
    assert derr <= 1e-6
    assert torch.equal(d[:, C:], torch.zeros(P, buf.shape[1] - C, dtype=torch.float64)), "pad lanes of the gradient"
    if bad:
        assert not d[list(bad)].any()


@pytest.mark.parametrize("P", [1, 257, 70001])
@pytest.mark.parametrize("C", [1, 2, 22, 64])
def test_cross_entropy_against_float64(P, C):
    for pad in (0, 2):
        for n, kind in enumerate(("normal", "x80", "extremes", "one_label")):
            x, lab, buf = _ce_case(P, C, pad, kind, 1000 * C + 10 * n + pad)
            _check_ce(x, lab, buf, C)


@pytest.mark.parametrize("P", [257, 70001])
def test_cross_entropy_skips_labels_outside_the_classes(P):
    x, lab, buf = _ce_case(P, 22, 2, "normal", 5)
    _check_ce(x, lab, buf, 22, bad=(0, P // 2, P - 1))


def test_cross_entropy_refusals():
    _lib, _ = _mods()
    h = _lib.lib()
    x = torch.zeros(8, 66, device="cuda")
    lab = torch.zeros(8, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.zeros(int(h.ape_cross_entropy_workspace_bytes(8)), dtype=torch.uint8, device="cuda")
    p = _lib.dptr
    call = lambda ld, C, n=ws.numel(), o=p(out), w=p(ws): h.ape_cross_entropy_f32(p(x), ld, C, p(lab), 8, ctypes.c_float(1.0), o, None, w, n, None)  # noqa: E731
    assert call(66, 64) == 0
    assert call(66, 65) == EINVAL
    assert call(20, 22) == EINVAL            # C > ld
    assert call(66, 0) == EINVAL
    assert call(66, 22, o=None) == EINVAL
    assert call(66, 22, w=None) == EINVAL
    assert call(66, 22, n=8) == -3           # APE_EWORKSPACE


def test_cross_entropy_tape():
    """CrossEntropyFn against torch autograd in float64, with a cotangent that is not 1"""
    from autoposeestimation_amd import autograd as A
    x, lab, _ = _ce_case(257, 22, 0, "normal", 11)
    xd = x.view(1, 257, 1, 22).cuda().requires_grad_(True)
    loss, bad = A.CrossEntropyFn.apply(xd, lab.cuda())
    (3.0 * loss).backward()
    xr = x.double().requires_grad_(True)
    want = F.cross_entropy(xr, lab.long())
    (3.0 * want).backward()
    assert abs(loss.item() - want.item()) <= 1e-6 * max(1.0, x.abs().max().item())
    assert (xd.grad.cpu().view(257, 22).double() - xr.grad).abs().max().item() * 257 / 3.0 <= 1e-6
    assert bad.item() == 0 and not bad.requires_grad

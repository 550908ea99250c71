"""The training step's backward, optimizer and metric kernels (csrc/backward.hip, segtrain.hip, adds.hip) against plain fp64 restatements
at the shapes, regimes and edges where such kernels go wrong.  Kernels are called through the C ABI (or their autograd.py wrapper) on
fixed-seed inputs.  Bounds are per element, |got - ref| <= c * u * sum|terms| (u = 2^-24, sum|terms| = the same fp64 sum over absolute
values); each case derives c from the fp32 roundings on its longest path: terms summed in fp32 plus split partials.  Single-rounding
kernels are compared bitwise.  The multi-workgroup regimes are restated from the host code and asserted.  Linear pairs are also checked
as adjoints, <fwd(x), dy> = <x, bwd(dy)> in fp64.  NaN propagation through max-pool is out of scope."""
import ctypes
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import densefusion_oracle as DO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
EINVAL, EWORKSPACE = -1, -3
NAN = float("nan")
_KEEP = []          # inline device tensors live until the test ends: a freed block is handed out again at once


@pytest.fixture(autouse=True)
def _release():
    yield
    _KEEP.clear()


def _L():
    from autoposeestimation_amd import _lib
    return _lib


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _d(t):
    _KEEP.append(t.to(DEV).contiguous())
    return _KEEP[-1]


def _call(name, *args):
    rc = getattr(_L().lib(), name)(*args, _L().stream_ptr())
    torch.cuda.synchronize()
    return rc


def _within(got, ref, bound, what):
    got, ref, bound = (t.detach().double().cpu() for t in (got, ref, bound))
    assert got.shape == ref.shape, what
    bad = ~((got - ref).abs() <= bound)                         # NaN fails too
    assert not bool(bad.any()), "%s: %d of %d out of bound, worst err/bound %.3g" % (
        what, int(bad.sum()), bad.numel(), float(((got - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(1e300).max()))


def _bitwise(got, ref, what):
    assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32)), what


def _adjoint(y, dy, x, dx, c, tot, what):
    lhs, rhs = float((y.cpu().double() * dy.double()).sum()), float((x.double() * dx.cpu().double()).sum())
    assert abs(lhs - rhs) <= c * U * tot, (what, lhs, rhs)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ==== conv weight gradient ===========================================================================================================
def _wgrad_splits(cout, ncols, npix):
    """wgrad_splits() of backward.hip: ~1024 workgroups, >= 64 pixels per split, at most 64 splits"""
    return max(min(-(-1024 // (-(-ncols // 64) * -(-cout // 64))), -(-npix // 64), 64), 1)


def _params(**kw):
    d = dict(B=1, H=1, W=1, Cin=4, ldx=4, xoff=0, Ho=1, Wo=1, Cout=1, ldy=1, yoff=0, KH=1, KW=1, stride=1, pad=0, dil=1, act=0, alpha=0.0,
             bias_bstride=0, ldr=0, roff=0, ups=0)
    d.update(kw)
    return _L().ConvParams(**d)


def _osz(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


WGRAD = [  # B, H, W, Cin, Cout, k, stride, pad, dil, ldx, xoff, ldy, yoff, cin_param, splits, name
    (1, 10, 10, 512, 1024, 3, 1, 1, 1, 512, 0, 1024, 0, 0, 1, "tiles>=1024"),
    (1, 8, 8, 4, 8, 3, 1, 1, 1, 4, 0, 8, 0, 0, 1, "npix<=64"),
    (2, 64, 64, 4, 16, 3, 1, 1, 1, 4, 0, 16, 0, 0, 64, "cap64"),
    (1, 63, 65, 4, 3, 3, 1, 1, 1, 4, 0, 3, 0, 0, 64, "npix%16"),
    (1, 17, 241, 4, 3, 1, 1, 0, 1, 4, 0, 3, 0, 0, 64, "trailing-empty"),
    (2, 19, 23, 4, 1, 3, 2, 1, 1, 4, 0, 1, 0, 0, None, "cout1-s2-odd"),
    (2, 13, 17, 4, 65, 3, 1, 2, 2, 4, 0, 65, 0, 0, None, "cout65-d2"),
    (1, 21, 19, 8, 3, 3, 2, 4, 4, 8, 0, 3, 0, 0, None, "cout3-d4-s2"),
    (2, 16, 16, 8, 16, 3, 2, 0, 1, 8, 0, 16, 0, 0, None, "pad0-s2"),
    (2, 11, 9, 4, 65, 3, 1, 1, 1, 12, 4, 70, 3, 0, None, "slices"),
    (2, 10, 12, 8, 7, 3, 1, 1, 1, 8, 0, 7, 0, 5, None, "param-cin5of8"),
    (1, 17, 241, 4, 3, 1, 1, 0, 1, 4, 0, 3, 0, 4, 64, "param-trailing-empty"),
]


@pytest.mark.parametrize("case", WGRAD, ids=[c[-1] for c in WGRAD])
def test_conv_wgrad(case):
    B, H, W, cin, cout, k, s, pad, dil, ldx, xoff, ldy, yoff, cinp, want, name = case
    ho, wo = _osz(H, k, s, pad, dil), _osz(W, k, s, pad, dil)
    g = _gen("wgrad", case)
    xb, dyb = torch.randn(B, H, W, ldx, generator=g), torch.randn(B, ho, wo, ldy, generator=g)
    p = _params(B=B, H=H, W=W, Cin=cin, ldx=ldx, xoff=xoff, Ho=ho, Wo=wo, Cout=cout, ldy=ldy, yoff=yoff, KH=k, KW=k, stride=s, pad=pad, dil=dil)
    ncols, npix = k * k * cin, B * ho * wo
    nb = _L().lib().ape_conv2d_wgrad_workspace_bytes(ctypes.byref(p))
    splits = (nb - 256) // (4 * cout * ncols)
    assert splits == _wgrad_splits(cout, ncols, npix) and (want is None or splits == want)
    pps = -(-(-(-npix // splits)) // 16) * 16                    # pixels per split, a multiple of 16
    assert "trailing" not in name or (splits - 1) * pps >= npix  # the last split is empty
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    dw = torch.full((cout, cinp, k, k) if cinp else (cout, k, k, cin), NAN, device=DEV)
    if cinp:
        rc = _call("ape_conv2d_wgrad_param_f32", _p(_d(xb)), _p(_d(dyb)), _p(dw), ctypes.byref(p), cinp, _p(ws), nb)
    else:
        rc = _call("ape_conv2d_wgrad_nhwc_f32", _p(_d(xb)), _p(_d(dyb)), _p(dw), ctypes.byref(p), _p(ws), nb)
    assert rc == 0
    x, dy = _nchw(xb[..., xoff:xoff + cin]).double(), _nchw(dyb[..., yoff:yoff + cout]).double()
    ref = torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dy, s, pad, dil)[:, :cinp or cin]
    mag = torch.nn.grad.conv2d_weight(x.abs(), (cout, cin, k, k), dy.abs(), s, pad, dil)[:, :cinp or cin]
    # c: pps pixels per split through the MFMA chain (<= 2 roundings each), then `splits` partials added in order
    _within(dw.cpu() if cinp else dw.cpu().permute(0, 3, 1, 2), ref, (2 * pps + splits + 2) * U * mag, name)


def test_conv_wgrad_empty_batch_and_refusals():
    big, ws = torch.zeros(1 << 20, device=DEV), torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)   # larger than any reading asks
    p0 = _params(B=0, H=5, W=6, Cin=8, ldx=8, Ho=5, Wo=6, Cout=3, ldy=3, KH=3, KW=3, pad=1)
    for cinp, shape in ((0, (3, 3, 3, 8)), (6, (3, 6, 3, 3))):
        dw = torch.full(shape, 7.5, device=DEV)
        rc = (_call("ape_conv2d_wgrad_param_f32", _p(big), _p(big), _p(dw), ctypes.byref(p0), cinp, _p(ws), ws.numel()) if cinp else
              _call("ape_conv2d_wgrad_nhwc_f32", _p(big), _p(big), _p(dw), ctypes.byref(p0), _p(ws), ws.numel()))
        assert rc == 0 and bool((dw == 0).all())             # B = 0 zero-fills

    def run(cinp=0, short=0, **kw):
        p = _params(**dict(dict(B=1, H=6, W=7, Cin=8, ldx=8, Ho=6, Wo=7, Cout=5, ldy=5, KH=3, KW=3, pad=1), **kw))
        nb = _L().lib().ape_conv2d_wgrad_workspace_bytes(ctypes.byref(p)) - short
        if cinp:
            return _call("ape_conv2d_wgrad_param_f32", _p(big), _p(big), _p(big), ctypes.byref(p), cinp, _p(ws), nb)
        return _call("ape_conv2d_wgrad_nhwc_f32", _p(big), _p(big), _p(big), ctypes.byref(p), _p(ws), nb)

    assert run() == 0 and run(cinp=8) == 0
    assert run(Cin=6) == run(Cin=4, ldx=10) == run(Cin=4, ldx=12, xoff=2) == run(Ho=7) == run(Wo=6) == EINVAL
    assert run(short=1) == EWORKSPACE
    assert run(cinp=9) == EINVAL                              # cin_param > Cin


@pytest.mark.parametrize("cin,cout,k,h,w", [(8, 12, 3, 15, 17), (12, 5, 3, 16, 16), (4, 6, 1, 13, 11), (8, 3, 1, 9, 1)])
def test_convfn_input_gradient_stride2_pad0(cin, cout, k, h, w):
    from autoposeestimation_amd import autograd as A, engine as E
    g = _gen("convfn", cin, cout, k, h, w)
    x, wt = torch.randn(2, cin, h, w, generator=g), torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    gy = torch.randn(2, cout, _osz(h, k, 2, 0, 1), _osz(w, k, 2, 0, 1), generator=g)
    xd, wd = _d(_nhwc(x)).requires_grad_(), _d(wt).requires_grad_()
    yd = A.conv(xd, wd, None, None, 2, 0, 1, E.ACT_NONE)
    yd.backward(_d(_nhwc(gy)))
    y, dx = _nchw(yd.detach().cpu()), _nchw(xd.grad.cpu())
    ymag = F.conv2d(x.double().abs(), wt.double().abs(), None, 2)
    # c: Cin k k (forward) / Cout k k (input gradient) products summed in fp32, plus up to 64 split-K partials
    _within(y, F.conv2d(x.double(), wt.double(), None, 2), (cin * k * k + 66) * U * ymag, "forward")
    _within(dx, torch.nn.grad.conv2d_input(x.shape, wt.double(), gy.double(), 2),
            (cout * k * k + 66) * U * torch.nn.grad.conv2d_input(x.shape, wt.double().abs(), gy.double().abs(), 2), "input gradient")
    _adjoint(y, gy, x, dx, (cin + cout) * k * k + 140, float((ymag * gy.double().abs()).sum()), "ConvFn")


# ==== activations, PReLU, column sums ================================================================================================
def test_act_bwd():
    L, n, g = _L(), 4099, _gen("act")
    dy, y = torch.randn(n, generator=g), F.relu(torch.randn(n, generator=g))
    y[:64] = 0.0
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 3)
    x[0], x[1] = 0.0, -0.0                                   # x = +-0 takes the alpha branch
    sg = torch.sigmoid(torch.randn(n, generator=g) * 4)
    sg[:8], sg[8:16] = 0.0, 1.0
    out = torch.full((n,), NAN, device=DEV)

    def run(act, ref, a=0.0):
        assert _call("ape_act_bwd_f32", _p(_d(dy)), _p(None if ref is None else _d(ref)), _p(out), n, act, a) == 0
        return out.cpu().clone()

    _bitwise(run(L.ACT_NONE, None), dy, "none")
    _bitwise(run(L.ACT_RELU, y), torch.ops.aten.threshold_backward(dy, y, 0.0), "relu")
    for a in (0.25, -0.3):
        _bitwise(run(L.ACT_PRELU, x, a), torch.where(x > 0, dy, torch.tensor(a) * dy), "prelu")
    ref = dy.double() * sg.double() * (1.0 - sg.double())
    _within(run(L.ACT_SIGMOID, sg), ref, 3 * U * ref.abs(), "sigmoid")   # c = 3: g * y, 1 - y, the product
    assert _call("ape_act_bwd_f32", _p(out), _p(None), _p(out), n, L.ACT_RELU, 0.0) == EINVAL


@pytest.mark.parametrize("n", [0, 1, 255, 257, 1024 * 256 + 4099])
@pytest.mark.parametrize("signs", ["mixed", "one-signed"])
def test_prelu_and_dalpha(n, signs):
    g = _gen("prelu", n, signs)
    x = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 6 - 3)
    dy = torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 4 - 2)
    if signs == "one-signed":
        x, dy = -x.abs(), dy.abs()                           # every term of the sum has one sign
    xd, dyd = (_d(x), _d(dy)) if n else (_d(torch.zeros(1)), _d(torch.zeros(1)))
    y = torch.full((max(n, 1),), 9.0, device=DEV)
    assert _call("ape_prelu_f32", _p(xd), _p(y), n, 0.2) == 0
    _bitwise(y.cpu()[:n], torch.where(x > 0, x, torch.tensor(0.2) * x), "prelu")
    blocks = min(max(-(-n // 256), 1), 1024)                 # ape_prelu_dalpha_f32's grid
    assert n <= 1024 * 256 or blocks == 1024                 # the block cap and the grid-stride loop both run
    da = torch.full((1,), NAN, device=DEV)
    assert _call("ape_prelu_dalpha_f32", _p(dyd), _p(xd), _p(da), n, _p(torch.full((1024,), NAN, device=DEV))) == 0
    t = dy.double() * x.double() * (x <= 0).double()
    # c: the product, ceil(n / 256 blocks) terms per thread, 6 shuffle levels, 3 wave adds, `blocks` partials in order
    _within(da.cpu()[0], t.sum(), (1 + -(-n // (256 * blocks)) + 9 + blocks) * U * t.abs().sum(), "dalpha")


@pytest.mark.parametrize("rows", [0, 1, 255, 256, 257, 64 * 256 + 1000, 100003])
@pytest.mark.parametrize("C,off,ld", [(1, 0, 1), (63, 2, 70), (65, 3, 69)])
def test_colsum(rows, C, off, ld):
    g = _gen("colsum", rows, C)
    x = torch.randn(rows, ld, generator=g) * torch.pow(10.0, torch.rand(rows, ld, generator=g) * 2 - 1)
    groups = min(max(-(-rows // 256), 1), 64)                # ape_colsum_f32's row groups
    rpg = -(-rows // groups)
    assert rows <= 64 * 256 or groups == 64
    out = torch.full((C,), NAN, device=DEV)
    xd = _d(x) if rows else _d(torch.zeros(ld))
    assert _call("ape_colsum_f32", _p(xd), _p(out), rows, C, ld, off, _p(torch.full((64 * C,), NAN, device=DEV))) == 0
    sl = x[:, off:off + C].double()
    # c: ceil(rpg / 4) rows per lane, 3 lane adds, `groups` partials in order
    _within(out.cpu(), sl.sum(0), (-(-rpg // 4) + 3 + groups) * U * sl.abs().sum(0), "colsum")
    assert _call("ape_colsum_f32", _p(xd), _p(out), rows, C, C + off - 1, off, _p(out)) == EINVAL     # off + C > ld


# ==== max-pool 3x3 s2 backward =======================================================================================================
@pytest.mark.parametrize("H", [1, 2, 3, 4, 5])
def test_maxpool_bwd(H):
    from autoposeestimation_amd import engine as E
    for W in range(1, 6):
        g, B, C = _gen("maxpool", H, W), 2, 4
        x = torch.randint(0, 3, (B, H, W, C), generator=g).float()     # ties everywhere
        x[..., 1], x[..., 2] = 1.0, float("-inf")                        # a plane of equal values; all -inf windows
        x[0, 1::2, 1::2, 3] = 5.0                                        # maxima shared by four windows
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dy = torch.randn(B, Ho, Wo, C, generator=g)
        xd = _d(x)
        y = _nchw(E.maxpool3x3s2(xd).cpu())
        assert torch.equal(y.double(), F.max_pool2d(_nchw(x).double(), 3, 2, 1))
        dx = torch.full_like(xd, NAN)
        assert _call("ape_maxpool3x3s2_bwd_nhwc_f32", _p(xd), _p(_d(dy)), _p(dx), B, H, W, C) == 0
        dx = _nchw(dx.cpu())
        xr, xm = _nchw(x).double().requires_grad_(), _nchw(x).double().requires_grad_()
        F.max_pool2d(xr, 3, 2, 1).backward(_nchw(dy).double())          # ATen's first maximum
        F.max_pool2d(xm, 3, 2, 1).backward(_nchw(dy).double().abs())
        _within(dx, xr.grad, 3 * U * xm.grad, "vs F.max_pool2d %dx%d" % (H, W))   # c = 3: <= 4 windows summed
        # the forward kernel's maxima: each window sends dy to its first (row-major) pixel equal to the forward's value
        win = F.unfold(F.pad(_nchw(x).double(), (1, 1, 1, 1), value=NAN), 3, stride=2).view(B, C, 9, -1)
        pix = F.unfold(F.pad(torch.arange(H * W, dtype=torch.float64).view(1, 1, H, W), (1, 1, 1, 1), value=-1), 3, stride=2).view(9, -1)
        first = (win == y.double().reshape(B, C, 1, -1)).double().argmax(2)          # torch.argmax: the first maximum
        src = pix.t()[torch.arange(Ho * Wo), first].long()
        gyf = _nchw(dy).double().reshape(B, C, -1)
        ref = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, src, gyf).view(B, C, H, W)
        mag = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, src, gyf.abs()).view(B, C, H, W)
        _within(dx, ref, 3 * U * mag, "vs the forward's first maximum %dx%d" % (H, W))


# ==== adaptive average pool, bilinear ================================================================================================
def _adaptive(B, H, W, C, S, key):
    from autoposeestimation_amd import engine as E
    g = _gen("adaptive", key)
    x, dy = torch.randn(B, H, W, C, generator=g), torch.randn(B, S, S, C, generator=g)
    xd = _d(x)
    y = _nchw(E.adaptive_avgpool(xd, S).cpu())
    dx = torch.full_like(xd, NAN)
    assert _call("ape_adaptive_avgpool_bwd_nhwc_f32", _p(_d(dy)), _p(dx), B, H, W, C, S) == 0
    dx = _nchw(dx.cpu())
    xr, xm = _nchw(x).double().requires_grad_(), _nchw(x).double().requires_grad_()
    F.adaptive_avg_pool2d(xr, (S, S)).backward(_nchw(dy).double())
    F.adaptive_avg_pool2d(xm, (S, S)).backward(_nchw(dy).double().abs())
    ymag = F.adaptive_avg_pool2d(_nchw(x).double().abs(), (S, S))
    # forward c: a bin's <= (H // S + 2)(W // S + 2) pixels summed, one scaling; backward c: <= (S // H + 2)(S // W + 2) bins, one division each
    cf, cb = (H // S + 2) * (W // S + 2) + 2, (S // H + 2) * (S // W + 2) + 1
    errs = []
    for f in (lambda: _within(y, F.adaptive_avg_pool2d(_nchw(x).double(), (S, S)), cf * U * ymag, "forward H=%d W=%d S=%d" % (H, W, S)),
              lambda: _within(dx, xr.grad, cb * U * xm.grad, "backward H=%d W=%d S=%d" % (H, W, S)),
              lambda: _adjoint(y, _nchw(dy), _nchw(x), dx, cf + cb + 2, float((ymag * _nchw(dy).double().abs()).sum()), (H, W, S))):
        try:
            f()
        except AssertionError as e:
            errs.append(str(e))
    return errs


@pytest.mark.parametrize("S", [1, 2, 3, 6])
@pytest.mark.parametrize("H", list(range(1, 14)))
def test_adaptive_avgpool_every_small_size(H, S):
    errs = sum((_adaptive(2, H, W, 4, S, (H, W, S)) for W in range(1, 14)), [])
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("S", [1, 2, 3, 6])
def test_adaptive_avgpool_large_map(S):
    errs = _adaptive(2, 61, 97, 8, S, ("large", S))
    assert not errs, "\n".join(errs)


def _taps(n_out, n_in, ac):
    """the kernel's fp32 source coordinates (numpy float32: one rounding per operation) -> weights A[o][i] and tap counts N[o][i]"""
    f = np.float32
    scale = (f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)) if ac else f(n_in) / f(n_out)
    d = np.arange(n_out, dtype=np.float32)
    s = scale * d if ac else np.maximum(scale * (d + f(0.5)) - f(0.5), f(0)).astype(np.float32)
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (s - i0.astype(np.float32)).astype(np.float32)
    A, N, o = np.zeros((n_out, n_in)), np.zeros((n_out, n_in)), np.arange(n_out)
    np.add.at(A, (o, i0), (f(1) - l1).astype(np.float64))
    np.add.at(A, (o, i1), l1.astype(np.float64))
    np.add.at(N, (o, i0), 1.0)
    np.add.at(N, (o, i1), 1.0)
    return torch.from_numpy(A), torch.from_numpy(N)


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("H,W,Ho,Wo", [(5, 7, 1, 1), (1, 1, 6, 9), (1, 6, 4, 11), (7, 1, 3, 5), (13, 17, 4, 6), (3, 2, 97, 61),
                                       (96, 80, 5, 3), (20, 24, 40, 48)])
def test_bilinear_bwd(H, W, Ho, Wo, ac):
    from autoposeestimation_amd import engine as E
    g, B, C = _gen("bilinear", H, W, Ho, Wo, ac), 2, 4
    x, dy = torch.randn(B, H, W, C, generator=g), torch.randn(B, Ho, Wo, C, generator=g)
    xd = _d(x)
    dx = torch.full_like(xd, NAN)
    assert _call("ape_bilinear_bwd_nhwc_f32", _p(_d(dy)), _p(dx), B, H, W, C, Ho, Wo, int(ac)) == 0
    y = E.bilinear(xd, Ho, Wo, ac).cpu()
    (Ay, Ny), (Ax, Nx) = _taps(Ho, H, ac), _taps(Wo, W, ac)
    bwd = lambda A1, t, A2: torch.einsum("oh,bopc,pw->bhwc", A1, t, A2)   # noqa: E731
    k = int((Ny.sum(0)[:, None] * Nx.sum(0)[None, :]).max())              # contributions per input pixel
    # c: g * ly * lx (2 roundings), then k float atomics in any order
    _within(dx.cpu(), bwd(Ay, dy.double(), Ax), (k + 2) * U * bwd(Ay, dy.double().abs(), Ax), "bilinear backward")
    # the restatement is torch's operator: fp64 coordinates differ from the fp32 ones by <= u * size per weight
    xr = _nchw(x).double().requires_grad_()
    F.interpolate(xr, size=(Ho, Wo), mode="bilinear", align_corners=ac).backward(_nchw(dy.double()))
    _within(xr.grad, _nchw(bwd(Ay, dy.double(), Ax)), 8 * max(H, W, Ho, Wo) * U * _nchw(bwd(Ny, dy.double().abs(), Nx)), "vs F.interpolate")
    ymag = torch.einsum("oh,bhwc,pw->bopc", Ay, x.double().abs(), Ax)
    _adjoint(y, dy, x, dx, 2 * k + 12, float((ymag * dy.double().abs()).sum()), "bilinear")


# ==== log-softmax, gather / scatter, mean ============================================================================================
@pytest.mark.parametrize("C", [1, 2, 21, 1000])
def test_log_softmax_bwd(C):
    g, rows = _gen("lsm", C), 37
    x = torch.randn(rows, C, generator=g) * 4
    if C > 1:
        x[3, : C // 2], x[5, 1:] = float("-inf"), float("-inf")     # y = -inf in part of a row / all but one
    y, dy = torch.log_softmax(x, 1), torch.randn(rows, C, generator=g)
    dx = torch.full((rows, C), NAN, device=DEV)
    assert _call("ape_log_softmax_bwd_rows_f32", _p(_d(dy)), _p(_d(y)), _p(dx), rows, C) == 0
    e = torch.exp(y.double())
    ref = dy.double() - e * dy.double().sum(1, keepdim=True)
    # c: C - 1 adds for sum(dy), expf (<= 2 ulp), the product, the difference
    _within(dx.cpu(), ref, 2 * U * ref.abs() + e * (C + 6) * U * dy.double().abs().sum(1, keepdim=True), "log-softmax backward")


@pytest.mark.parametrize("mode", ["random", "one-row", "out-of-range"])
@pytest.mark.parametrize("B,rows,n", [(3, 7, 11), (2, 50, 1), (4, 1, 9)])
def test_scatter_add_rows_is_gathers_adjoint(mode, B, rows, n):
    from autoposeestimation_amd import engine as E
    g, C = _gen("scatter", mode, B, rows, n), 8
    idx = {"random": lambda: torch.randint(0, rows, (B, n), generator=g), "one-row": lambda: torch.full((B, n), rows // 2),
           "out-of-range": lambda: torch.randint(-3, rows + 3, (B, n), generator=g)}[mode]()
    if mode == "out-of-range":
        idx[0, 0], idx[-1, -1] = -(1 << 40), 1 << 40
    dy, x = torch.randn(B, n, C, generator=g), torch.randn(B, rows, C, generator=g)
    idxd, dx = _d(idx), torch.full((B, rows, C), NAN, device=DEV)
    assert _call("ape_scatter_add_rows_f32", _p(_d(dy)), _p(idxd), _p(dx), B, rows, n, C) == 0
    cl = idx.clamp(0, rows - 1)                              # gather_rows clamps a bad index
    y = E.gather_rows(_d(x), idxd).cpu()
    assert torch.equal(y, torch.stack([x[b][cl[b]] for b in range(B)]))
    ref, mag = torch.zeros(B, rows, C, dtype=torch.float64), torch.zeros(B, rows, C, dtype=torch.float64)
    for b in range(B):
        ref[b].index_add_(0, cl[b], dy[b].double())
        mag[b].index_add_(0, cl[b], dy[b].double().abs())
    _within(dx.cpu(), ref, n * U * mag, mode)               # c = n: <= n float atomics per row, any order
    _adjoint(y, dy, x, dx, n + 2, float((x.double().abs() * mag).sum()), "gather/scatter " + mode)
    dx0 = torch.full((B, rows, C), 4.25, device=DEV)
    assert _call("ape_scatter_add_rows_f32", _p(dx0), _p(idxd), _p(dx0), B, rows, 0, C) == 0 and bool((dx0 == 0).all())   # n = 0


@pytest.mark.parametrize("B,n,C", [(3, 7, 8), (2, 1, 4), (4, 1000, 12), (1, 65, 3)])
def test_mean_rows_bwd(B, n, C):
    from autoposeestimation_amd import engine as E
    g = _gen("mean", B, n, C)
    dy, x = torch.randn(B, C, generator=g), torch.randn(B, n, C, generator=g)
    dx = torch.full((B, n, C), NAN, device=DEV)
    assert _call("ape_mean_rows_bwd_f32", _p(_d(dy)), _p(dx), B, n, C) == 0
    _bitwise(dx.cpu(), (dy / n)[:, None, :].expand(B, n, C).contiguous(), "mean backward")
    y = E.mean_rows(_d(x)).cpu()
    _within(y, x.double().mean(1), (n + 2) * U * x.double().abs().mean(1), "mean forward")   # c: n - 1 adds, the scaling
    _adjoint(y, dy, x, dx, n + 4, float((x.double().abs().mean(1) * dy.double().abs()).sum()), "mean")


# ==== BatchNorm (train mode) =========================================================================================================
def _bn_groups(rows, C):
    """rows_per() of segtrain.hip: one group per 256 rows, at most 2048 / channel tiles and at most 1024"""
    return max(1, min(-(-rows // 256), 2048 // -(-C // 64), 1024))


BN = [(1, 1, 1, 2, 0, False, None), (3, 1, 2, 1, 1, True, None), (65, 1, 1, 2, 0, True, None), (130, 2, 1, 1, 1, False, None),
      (3, 2, 9, 13, 1, True, None), (1, 1, 300, 1000, 0, False, 1024), (65, 2, 150, 1000, 0, False, 1024), (130, 1, 175, 1000, 0, False, 682)]


@pytest.mark.parametrize("case", BN, ids=["C%d-rows%d-relu%d" % (c[0], c[1] * c[2] * c[3], c[4]) for c in BN])
def test_batchnorm_train(case):
    from autoposeestimation_amd import autograd as A
    C, B, H, W, relu, has_res, cap = case
    rows = B * H * W
    assert cap is None or _bn_groups(rows, C) == cap       # 1024 cap; 2048 / 2 = 1024; 2048 / 3
    g = _gen("bn", case)
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g)
    rmd, rvd, nbt = _d(torch.zeros(C)), _d(torch.ones(C)), torch.zeros((), dtype=torch.int64, device=DEV)
    rm, rv, brm, brv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64), 0.0, 0.0
    steps = 3 if rows < 10000 else 1                          # running buffers over three steps at the small shapes
    for step in range(steps):
        x = torch.randn(B, C, H, W, generator=g) * 2 + 0.5
        x[:, 0] = 1e3 + 1e-2 * torch.randn(B, H, W, generator=g)        # mean 1e3, std 1e-2
        res = torch.randn(B, C, H, W, generator=g) if has_res else None
        dy = torch.randn(B, C, H, W, generator=g)
        xd, gd, bd = _d(_nhwc(x)).requires_grad_(), _d(gamma).requires_grad_(), _d(beta).requires_grad_()
        resd = _d(_nhwc(res)).requires_grad_() if has_res else None
        y = A.BatchNormFn.apply(xd, gd, bd, resd, rmd, rvd, nbt, relu, 1e-5, 0.1)
        y.backward(_d(_nhwc(dy)))
        y = _nchw(y.detach().cpu())
        x64, g64, b64 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
        mu, var = x.double().mean((0, 2, 3)), x.double().var((0, 2, 3), unbiased=False)
        cv = lambda t: t[None, :, None, None]                 # noqa: E731
        xh = (x.double() - cv(mu)) / cv(torch.sqrt(var + 1e-5))
        z = F.batch_norm(x64, None, None, g64, b64, training=True, eps=1e-5) + (res.double() if has_res else 0.0)
        zmag = (xh * cv(gamma.double())).abs() + cv(beta.double().abs()) + (res.double().abs() if has_res else 0.0)
        # forward c = 8: x - hi, - lo, * invstd (and its own rounding), * gamma, + beta, + residual
        _within(y, F.relu(z) if relu else z, 8 * U * zmag, "forward %d" % step)
        gm = torch.where(y > 0, dy.double(), 0.0) if relu else dy.double()   # the device's own ReLU mask
        z.backward(gm)
        gs, gx = gm.sum((0, 2, 3)), (gm * xh).abs().sum((0, 2, 3))
        dxmag = cv(gamma.double().abs() / torch.sqrt(var + 1e-5)) * (gm.abs() + cv(gs.abs() / rows) + xh.abs() * cv(2 * gx / rows))
        # dx c = 12: the two coefficients, x_hat (4), three element operations, gamma * invstd (2); dgamma: fp64 sum of fp32 products
        # whose x_hat carries <= 4 roundings; dbeta: fp64 sum of fp32 values
        _within(_nchw(xd.grad.cpu()), x64.grad, 12 * U * dxmag, "dx %d" % step)
        _within(gd.grad.cpu(), g64.grad, 5 * U * gx + 1e-300, "dgamma %d" % step)
        _within(bd.grad.cpu(), b64.grad, 2 * U * gm.abs().sum((0, 2, 3)) + 1e-300, "dbeta %d" % step)
        if has_res:
            _bitwise(resd.grad.cpu(), _nhwc(gm.float()), "residual gradient")
        # running buffers (momentum 0.1, unbiased variance): 6 roundings per step, earlier error damped by 0.9
        vu = var * rows / (rows - 1)
        brm, brv = 0.9 * brm + 6 * U * (0.9 * rm.abs() + 0.1 * mu.abs()), 0.9 * brv + 6 * U * (0.9 * rv.abs() + 0.1 * vu)
        rm, rv = 0.9 * rm + 0.1 * mu, 0.9 * rv + 0.1 * vu
        _within(rmd.cpu(), rm, brm, "running_mean %d" % step)
        _within(rvd.cpu(), rv, brv, "running_var %d" % step)
    assert int(nbt) == steps


# ==== nearest x2 backward, softmax ===================================================================================================
@pytest.mark.parametrize("B,h,w,C,ld,off", [(2, 3, 5, 6, 20, 7), (1, 1, 1, 1, 3, 2), (2, 4, 3, 8, 24, 8), (3, 2, 7, 13, 13, 0)])
def test_upsample_nearest2x_bwd(B, h, w, C, ld, off):
    from autoposeestimation_amd import engine as E
    g = _gen("ups", B, h, w, C, ld, off)
    dyb = torch.randn(B, 2 * h, 2 * w, ld, generator=g)
    dx = torch.full((B, h, w, C), NAN, device=DEV)
    assert _call("ape_upsample_nearest2x_bwd_f32", _p(_d(dyb)), ld, off, _p(dx), B, h, w, C) == 0
    d = dyb[..., off:off + C]
    _bitwise(dx.cpu(), (d[:, 0::2, 0::2] + d[:, 0::2, 1::2]) + (d[:, 1::2, 0::2] + d[:, 1::2, 1::2]), "nearest x2 backward")
    if C % 4 == 0 and off % 4 == 0 and ld % 4 == 0:           # the forward's channel-window constraints
        x, out = torch.randn(B, h, w, C, generator=g), torch.zeros(B, 2 * h, 2 * w, ld, device=DEV)
        up = E.nearest_up2(_d(x), out, off).cpu()[..., off:off + C]
        _adjoint(up, d, x, dx, 6, float((up.double().abs() * d.double().abs()).sum()), "nearest x2")
    assert _call("ape_upsample_nearest2x_bwd_f32", _p(dx), C, 1, _p(dx), 1, 1, 1, C) == EINVAL      # off + C > ld


@pytest.mark.parametrize("C", [1, 2, 32, 100])
def test_softmax_rows_and_bwd(C):
    g, rows = _gen("softmax", C), 40
    x = torch.randn(rows, C, generator=g) * 3 + torch.tensor([0.0, 80.0, -80.0, 1e4, -1e4]).repeat(8)[:, None]
    y = torch.full((rows, C), NAN, device=DEV)
    assert _call("ape_softmax_rows_f32", _p(_d(x)), _p(y), rows, C) == 0
    ref = torch.softmax(x.double(), 1)
    _within(y.cpu(), ref, (C + 8) * U * ref, "softmax")      # c: x - max (exact), expf (<= 2 ulp), C - 1 adds, reciprocal, product
    dy = torch.randn(rows, C, generator=g)
    dx = torch.full((rows, C), NAN, device=DEV)
    assert _call("ape_softmax_rows_bwd_f32", _p(_d(dy)), _p(y), _p(dx), rows, C) == 0
    y64, dy64 = y.cpu().double(), dy.double()
    dref = y64 * (dy64 - (dy64 * y64).sum(1, keepdim=True))
    # c: C products and C - 1 adds for sum(dy y), then the difference and the product
    _within(dx.cpu(), dref, 2 * U * dref.abs() + y64 * (C + 2) * U * ((dy64 * y64).abs().sum(1, keepdim=True) + dy64.abs()), "softmax bwd")


# ==== SGD ============================================================================================================================
SGD = [(0.1, 0.0, 0.0, 0.0, False), (0.1, 0.0, 0.0, 1e-2, False), (0.05, 0.9, 0.3, 0.0, False), (0.05, 0.9, 0.1, 1e-2, False),
       (0.05, 0.9, 0.0, 1e-2, True), (0.05, 0.8, 0.0, 0.0, True)]


@pytest.mark.parametrize("cfg", SGD, ids=["lr%g-m%g-d%g-wd%g-nest%d" % c for c in SGD])
def test_sgd_multi_vs_torch(cfg):
    L = _L()
    lr, mom, damp, wd = (float(np.float32(v)) for v in cfg[:4])   # the fp32 values the kernel receives
    nest, g = cfg[4], _gen("sgd", cfg)
    sizes = [int(v) for v in torch.randint(1, 3000, (70,), generator=g)]
    sizes[5], sizes[40] = 0, 70000                       # an empty buffer; one past the 256-block cap; 70 buffers = two launches of 64
    params = [_d(torch.randn(max(n, 1), generator=g)) for n in sizes]       # an empty job still passes valid pointers
    bufs = [torch.full((max(n, 1),), NAN, device=DEV) for n in sizes]
    for step in range(3):                                # the first step's buffer is d, not (1 - dampening) d
        grads = [_d(torch.randn(max(n, 1), generator=g) * 0.5) for n in sizes]
        p0 = [p.cpu().double()[:n] for p, n in zip(params, sizes)]
        b0 = [b.cpu().double()[:n] for b, n in zip(bufs, sizes)]
        jobs = (L.SgdJob * 70)(*[L.SgdJob(param=p.data_ptr(), grad=gr.data_ptr(), momentum_buffer=b.data_ptr() if mom else None, n=n,
                                          first=int(step == 0), reserved=0) for p, gr, b, n in zip(params, grads, bufs, sizes)])
        assert _call("ape_sgd_step_multi_f32", 70, jobs, lr, mom, damp, wd, int(nest)) == 0
        ref = [p.clone().requires_grad_() for p in p0]   # fp64 torch.optim.SGD from the device's state before the step
        for r, gr in zip(ref, grads):
            r.grad = gr.cpu().double()[:r.numel()]
        opt = torch.optim.SGD(ref, lr=lr, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nest)
        for r, b in zip(ref, b0):
            if step and mom:
                opt.state[r]["momentum_buffer"] = b.clone()
        opt.step()
        for i, n in enumerate(sizes):
            dmag = grads[i].cpu().double()[:n].abs() + wd * p0[i].abs()
            bmag = dmag if step == 0 else mom * b0[i].abs() + abs(1 - damp) * dmag
            if mom:       # buffer c = 5: wd * p, + g, momentum * buf, (1 - dampening) * d, +
                _within(bufs[i].cpu()[:n], opt.state[ref[i]]["momentum_buffer"], 5 * U * bmag, "buffer %d step %d" % (i, step))
            dirmag = (dmag + mom * bmag if nest else bmag) if mom else dmag
            # parameter c = 10: the buffer's 5, the Nesterov product and add, lr * d, the update
            _within(params[i].cpu()[:n], ref[i].detach(), 10 * U * (p0[i].abs() + lr * dirmag), "param %d step %d" % (i, step))


def test_sgd_refusals():
    L, b = _L(), torch.zeros(16, device=DEV)

    def run(mom=0.9, damp=0.0, nest=0, lr=0.1, n=16, buf=True):
        job = (L.SgdJob * 1)(L.SgdJob(param=b.data_ptr(), grad=b.data_ptr(), momentum_buffer=b.data_ptr() if buf else None, n=n, first=1))
        return _call("ape_sgd_step_multi_f32", 1, job, lr, mom, damp, 0.0, nest)

    assert run() == run(mom=0.0, buf=False) == run(nest=1) == run(n=0) == 0
    assert run(nest=1, damp=0.1) == run(nest=1, mom=0.0) == run(buf=False) == run(n=-1) == run(lr=-0.1) == run(lr=NAN) == run(mom=-0.5) == EINVAL


# ==== confusion matrix, Jaccard class limits =========================================================================================
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_confusion_argmax_ties_and_nan(layout):
    K, B, H, W, g = 64, 2, 9, 13, _gen("conf", layout)
    s = torch.randint(0, 3, (B, K, H, W), generator=g).float()      # exact ties everywhere
    s[torch.rand(B, K, H, W, generator=g) < 0.01] = NAN
    s[0, :, 0, 0], s[0, :, 0, 1], s[0, K - 1, 0, 1] = NAN, 2.0, NAN  # NaN everywhere; a NaN in the last channel only
    tgt = torch.randint(0, K, (B, H, W), generator=g)
    tgt[1, 2, 3] = K                                                 # out of range: flagged, not counted
    dev = _d(s.permute(0, 2, 3, 1)).permute(0, 3, 1, 2) if layout == "nhwc" else _d(s)
    conf, bad = torch.zeros(K * K, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    st, lab = (ctypes.c_long * 4)(*dev.stride()), _d(tgt.reshape(-1))
    assert _call("ape_confusion_add", _p(dev), st, None, None, None, _p(lab), B, H, W, K, _p(conf), _p(bad)) == 0
    pred, ok = np.argmax(s.numpy(), axis=1), tgt.numpy() < K         # numpy: the first maximum; a NaN counts as the maximum
    want = np.zeros((K, K), np.int64)
    np.add.at(want, (tgt.numpy()[ok], pred[ok]), 1)
    assert int(bad.cpu()) == 1 and np.array_equal(conf.cpu().view(K, K).numpy(), want)
    assert _call("ape_confusion_add", _p(dev), st, None, None, None, _p(lab), B, H, W, K + 1, _p(conf), _p(bad)) == EINVAL


@pytest.mark.parametrize("C", [32, 33])
def test_jaccard_class_limit(C):
    L, B, H, W = _L(), 2, 8, 8
    logits, labd = _d(torch.randn(B, C, H, W, generator=_gen("jac", C))), _d(torch.arange(B * H * W).remainder(C))
    st = (ctypes.c_long * 4)(*logits.stride())
    nb = max(int(L.lib().ape_jaccard_workspace_bytes(32, 1)), 256)
    ws, loss, gs = torch.zeros(nb, dtype=torch.uint8, device=DEV), torch.full((1,), NAN, device=DEV), torch.ones(1, device=DEV)
    dl, want = torch.empty_like(logits), 0 if C <= 32 else EINVAL
    assert _call("ape_jaccard_fwd_f32", _p(logits), st, _p(labd), B, C, H, W, 1, 1e-7, _p(loss), _p(ws), nb) == want
    assert _call("ape_jaccard_bwd_f32", _p(logits), st, _p(labd), B, C, H, W, 1, _p(gs), _p(dl), st, _p(ws), nb) == want
    assert want or 0.0 < float(loss) < 1.0


# ==== ADD(-S) loss gradient ==========================================================================================================
def _adds_check(r, t, pts, model, target, c, sym, full, w=0.015, gsc=0.7):
    """fp64 autograd through oracle/densefusion_oracle.py's Loss (full) or Loss_refine's dis against ape_adds_grad_f32"""
    N, M = r.shape[0], model.shape[0]
    rd, td, md, tgd, ptd, cd = _d(r), _d(t), _d(model), _d(target), _d(pts) if full else None, _d(c) if full else None
    dis, std = torch.empty(N, device=DEV), torch.empty(N, device=DEV) if full else None
    assert _call("ape_adds_dis_f32", _p(rd), _p(td), _p(ptd), _p(md), _p(tgd), N, M, int(sym), None, _p(dis), _p(std)) == 0
    d_r, d_t = torch.full((N, 4), NAN, device=DEV), torch.full((N, 3), NAN, device=DEV)
    d_c = torch.full((N,), NAN, device=DEV) if full else None
    assert _call("ape_adds_grad_f32", _p(rd), _p(td), _p(ptd), _p(md), _p(tgd), _p(cd), _p(dis), _p(std), _p(_d(torch.tensor([gsc]))), N, M,
                 int(sym), int(full), w, _p(d_r), _p(d_t), _p(d_c)) == 0
    r64, t64, idx, syms = r.double().requires_grad_(), t.double().requires_grad_(), torch.tensor([[0]]), [0] if sym else []
    if full:
        c64 = c.double().requires_grad_()
        loss = DO.loss_forward(r64[None], t64[None], c64.view(1, N, 1), target.double()[None], model.double()[None], idx, pts.double()[None],
                               w, False, M, syms)[0]
        loss.backward(torch.tensor(gsc, dtype=torch.float64))
    else:
        DO.loss_refine_forward(r64, t64, target.double()[None], model.double()[None], idx, torch.zeros(1, 1, 3, dtype=torch.float64), M,
                               syms)[0].backward(torch.full((1,), gsc, dtype=torch.float64))
    # A[n, m] bounds |dL / d pred_nm| times the conditioning of the unit vector (pred - tgt) / |.|; d_t sums A, d_r sums A |model|
    with torch.no_grad():
        qn = r.double() / r.double().norm(dim=1, keepdim=True)
        T = t.double() + (pts.double() if full else 0.0)
        pred = torch.einsum("mi,nji->nmj", model.double(), DO.quat_to_base(qn)) + T[:, None, :]
        tg = (target.double()[((target.double()[None, None] - pred[:, :, None]) ** 2).sum(-1).argmin(-1)] if sym else
              target.double()[None].expand(N, M, 3))
        nrm = (pred - tg).norm(dim=-1)
        dis, sd = nrm.mean(1), nrm.std(1) if M > 1 else None
        wgt = (abs(gsc) * c.double()[:, None] / N * (1.0 / M + 2 * (nrm + dis[:, None]) / ((M - 1) * sd[:, None])) if full else
               torch.full_like(nrm, abs(gsc) / M))
        A = wgt * (1 + 4 * (model.double().abs().sum(1)[None] + T.abs().sum(1)[:, None] + tg.abs().sum(-1)) / nrm)
        cc = -(-M // 256) + 40        # c: ceil(M / 256) points per thread, 8 block-sum levels, ~24 roundings per point term and chain
        _within(d_t.cpu(), t64.grad, (cc * U * A.sum(1))[:, None].expand(N, 3), "d_t")
        SR = (A * model.double().abs().sum(1)[None]).sum(1)
        _within(d_r.cpu(), r64.grad, (cc * U * 60 * qn.abs().sum(1) * SR / r.double().norm(dim=1))[:, None].expand(N, 4), "d_r")
        if full:
            _within(d_c.cpu(), c64.grad, (cc + 8) * U * abs(gsc) * (dis + 2 * sd + w / c.double()) / N, "d_c")


def _pose(N, M, key):
    g = _gen("adds", N, M, key)
    r = torch.randn(N, 4, generator=g) * torch.pow(10.0, torch.rand(N, 1, generator=g) * 1.4 - 0.7)    # |q| from 0.2 to 5
    return (r, torch.randn(N, 3, generator=g) * 0.1, torch.randn(N, 3, generator=g) * 0.1, torch.randn(M, 3, generator=g) * 0.05,
            torch.randn(M, 3, generator=g) * 0.05 + 0.02, torch.rand(N, generator=g) * 0.9 + 0.05)


@pytest.mark.parametrize("N,M,sym", [(500, 300, False), (1, 300, False), (5, 300, True), (1, 2, False), (3, 7900, False), (4, 257, True)])
def test_adds_grad_full(N, M, sym):
    _adds_check(*_pose(N, M, ("full", sym)), sym, True)     # M = 7900: most of the LDS target buffer


@pytest.mark.parametrize("M,sym", [(300, False), (300, True), (7900, False), (1, False)])
def test_adds_grad_refine(M, sym):
    r, t, _, model, target, _ = _pose(1, M, ("refine", sym))
    _adds_check(r, t, None, model, target, None, sym, False)


@pytest.mark.parametrize("full", [True, False])
def test_adds_grad_symmetric_ties_follow_lowest_index(full):
    """identity rotation, zero translation, model points on an even integer grid, each target at +(1, 0, dz) of a model point (dz = layer
    parity): every fp32 distance is exact, most model points have two nearest targets (x +- 1) at different indices, and distances are 1 or
    sqrt(2) so std > 0.  The gradient must follow the lowest index, as adds_dis and the k-NN oracle do."""
    model = torch.tensor([(2 * a, 2 * b, 4 * z) for a in range(6) for b in range(4) for z in range(3)], dtype=torch.float32)
    tg = model + torch.tensor([1.0, 0.0, 0.0])
    tg[:, 2] += (model[:, 2] / 4).remainder(2)
    target = tg[torch.randperm(len(model), generator=_gen("tiegrid", full))]
    d2 = ((target[None] - model[:, None]) ** 2).sum(-1)
    assert int(((d2 == d2.min(1, keepdim=True).values).sum(1) >= 2).sum()) >= len(model) // 2     # the ties are real
    N = 2 if full else 1
    r = torch.tensor([[1.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0]][:N])                           # |q| = 2: the same rotation
    _adds_check(r, torch.zeros(N, 3), torch.zeros(N, 3) if full else None, model, target, torch.tensor([0.6, 0.3][:N]) if full else None,
                True, full)

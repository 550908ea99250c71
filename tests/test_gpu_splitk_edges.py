"""GPU checks of the split-K form of csrc/conv_gemm.hip (ape_conv_gemm_bf16_splitk: conv_gemm_splitk_kernel<{1, 3}, {pure, not}> and
splitk_finish_kernel) at its edge shapes, against the float64 sum of the kernel's own products (tests/conv_products_reference.py) on the
inputs of tests/conv_edge_cases.py -- whose guards and branch-reached claims tests/test_conv_edges_host.py proves on the CPU.

|got - restatement| <= 2e-6 max(1, max|restatement|) for both precisions: the restatement holds the kernel's very products, so only the
float32 accumulation order remains (the project's bar for "same products, other summation order"); the plain float64 convolution of the
unsplit operands is held at test_gpu_conv.py's TOL.  Operands are channel slices of wider tensors whose unread channels are NaN; the
output window, the buffer around it and the workspace carry sentinels and guards.  Then the contract (workspace size, the two refusals,
run-to-run bits, the one-pass kernel) and the routing of engine.Conv(..., splitk=True) inside and outside engine.low_latency()."""
import ctypes

import numpy as np
import pytest
import torch

import conv_edge_cases as EC
import conv_products_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EWORKSPACE = -1, -3


def _mods():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    return _lib, E


def _guarded(t=None, shape=None, fill=0.0, dtype=torch.float32):
    n = int(np.prod(shape if t is None else t.shape))
    whole = torch.full((n + 2 * EC.GUARD,), fill, dtype=dtype, device=DEV)
    view = whole[EC.GUARD:EC.GUARD + n].view(tuple(shape if t is None else t.shape))
    if t is not None:
        view.copy_(t)
    return view, whole


def _guards_intact(whole, fill):
    return bool((whole[:EC.GUARD] == fill).all() and (whole[-EC.GUARD:] == fill).all())


class _Case:
    """the device operands of one split-K case and the two raw entry points on them"""

    def __init__(self, name, nsplit):
        self.lib, E = _mods()
        self.name, self.nsplit = name, nsplit
        g, x, w, bias, res = EC.splitk_inputs(name)
        self.g, self.M = g, g["B"] * g["Ho"] * g["Wo"]
        self.p = self.lib.ConvParams(**g)
        self.x = _guarded(x, fill=EC.NAN)[0]
        self.bias = None if bias is None else _guarded(bias, fill=EC.NAN)[0]
        self.res = None if res is None else _guarded(res, fill=EC.NAN)[0]
        self.conv = E.Conv(w, None, g["stride"], g["pad"], g["dil"], g["act"], alpha=g["alpha"], device=DEV, precision=EC.PRECISION[nsplit])
        self.need = int(self.lib.lib().ape_conv_gemm_splitk_workspace_bytes(ctypes.byref(self.p)))

    def new_y(self):
        return _guarded(shape=(self.M, self.g["ldy"]), fill=EC.Y_SENTINEL)

    def splitk(self, y, ws, ws_bytes):
        d = self.lib.dptr
        return self.lib.lib().ape_conv_gemm_bf16_splitk(d(self.x), d(self.conv.wp), d(self.bias), d(self.res), d(y), ctypes.byref(self.p), self.nsplit,
                                                        d(ws), ws_bytes, self.lib.stream_ptr())

    def one_pass(self, y):
        d = self.lib.dptr
        return self.lib.lib().ape_conv_gemm_bf16(d(self.x), d(self.conv.wp), d(self.bias), d(self.res), d(y), ctypes.byref(self.p), self.nsplit, 0,
                                                 self.lib.stream_ptr())


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", list(EC.SPLITK_CASES))
def test_splitk_against_its_own_products_and_its_contract(name, nsplit):
    c = _Case(name, nsplit)
    g, M, Cout, yoff = c.g, c.M, c.g["Cout"], c.g["yoff"]
    nk, nk_per, launched = EC.splitk_plan(g)
    assert c.need > 0                                                     # a case the library would not split tests nothing
    assert c.need == launched * M * Cout * 4
    ws, ws_whole = _guarded(shape=(c.need // 4,), fill=EC.WS_SENTINEL)
    # one byte less: refused, y untouched
    y, whole = c.new_y()
    assert c.splitk(y, ws, c.need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert (whole == EC.Y_SENTINEL).all() and (ws_whole == EC.WS_SENTINEL).all()
    assert c.splitk(y, ws, c.need) == 0
    y2, whole2 = c.new_y()
    assert c.splitk(y2, ws, c.need) == 0
    y1p, _ = c.new_y()
    assert c.one_pass(y1p) == 0
    torch.cuda.synchronize()
    assert _guards_intact(ws_whole, EC.WS_SENTINEL) and not torch.isnan(ws).any()
    assert torch.equal(whole, whole2)                                     # two calls: the same bits (fixed-order second pass)
    whole = whole.cpu()
    yc = whole[EC.GUARD:-EC.GUARD].view(M, g["ldy"])
    assert not torch.isnan(whole).any()
    assert _guards_intact(whole, EC.Y_SENTINEL) and (yc[:, :yoff] == EC.Y_SENTINEL).all() and (yc[:, yoff + Cout:] == EC.Y_SENTINEL).all()
    got = yc[:, yoff:yoff + Cout].double()
    want, plain = EC.splitk_expected(name, nsplit), EC.splitk_expected(name, 0)
    scale = max(1.0, float(want.abs().max()))
    r = float((got - want).abs().max()) / scale
    r0 = float((got - plain).abs().max()) / max(1.0, float(plain.abs().max()))
    one = y1p.cpu()[:, yoff:yoff + Cout].double()
    r1 = float((got - one).abs().max()) / scale
    print("split-K %s nsplit %d: %.3g of the output scale against its own products (%.0f %% of the bar), %.3g against the one-pass kernel, "
          "%.3g against the plain conv" % (name, nsplit, r, 100 * r / EC.BAR, r1, r0))
    assert r <= EC.BAR, (name, nsplit, r)
    assert r1 <= EC.BAR, (name, nsplit, r1)
    assert r0 <= EC.TOL[nsplit], (name, nsplit, r0)


def test_a_shape_that_does_not_split_is_refused():
    _lib, E = _mods()
    c = _Case("pure_cin672_last_split_one_ktile", 3)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    y, whole = c.new_y()
    for change in (dict(Cout=64, ldy=68), dict(Cin=224, ldx=232)):        # Cout <= 64; fewer than 8 k-tiles
        p = _lib.ConvParams(**dict(c.g, **change))
        assert _lib.lib().ape_conv_gemm_splitk_workspace_bytes(ctypes.byref(p)) == 0
        d = _lib.dptr
        assert _lib.lib().ape_conv_gemm_bf16_splitk(d(c.x), d(c.conv.wp), None, None, d(y), ctypes.byref(p), 3, d(ws), ws.numel(),
                                                    _lib.stream_ptr()) == EINVAL
    p = _lib.ConvParams(**R.conv_geometry(64, 20, 20, 256, 512))          # a chip-filling batch: 100 x 4 tiles
    assert _lib.lib().ape_conv_gemm_splitk_workspace_bytes(ctypes.byref(p)) == 0
    torch.cuda.synchronize()
    assert (whole == EC.Y_SENTINEL).all()


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_low_latency_routes_only_the_layers_built_for_it(precision):
    """Conv(..., splitk=True) inside engine.low_latency() == conv(x, splitk=True) bit for bit; outside the block, and for a layer built
    without the keyword inside it, the one-pass bits; at K = 1056 the two summation orders differ"""
    _, E = _mods()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 20, 1, 1056, generator=g).to(DEV)
    w = torch.randn(66, 1056, generator=g) / 1056 ** 0.5
    b = torch.randn(66, generator=g)
    pose = E.Conv(w, b, act=E.ACT_RELU, device=DEV, precision=precision, splitk=True)
    seg = E.Conv(w, b, act=E.ACT_RELU, device=DEV, precision=precision)
    one_pass = seg(x)
    explicit = pose(x, splitk=True)
    assert torch.equal(seg(x, splitk=True), explicit)
    assert torch.equal(pose(x), one_pass)
    with E.low_latency():
        assert torch.equal(pose(x), explicit)
        assert torch.equal(seg(x), one_pass)
        with E.low_latency(False):
            assert torch.equal(pose(x), one_pass)
    assert torch.equal(pose(x), one_pass)
    assert not torch.equal(explicit, one_pass)
    assert float((explicit - one_pass).abs().max()) <= EC.BAR * max(1.0, float(one_pass.abs().max()))

"""GPU checks of the LDS-halo 3x3 kernels at their edge shapes, through their raw entry points: ape_conv3x3_halo_bf16 (csrc/conv3x3_halo.hip:
every (dilation, block width) pair, the fused x2 up-sampling) and ape_conv3x3_halo_s32 (csrc/conv3x3_halo_s32.hip: ping-pong and lockstep
schedules, ragged rpw rows, the persistent tile walk, both S32 stores), against the float64 sum of the kernels' own products
(tests/conv_products_reference.py) on the inputs of tests/conv_edge_cases.py -- whose guards, branch-reached claims and mutations
tests/test_halo_edges_host.py proves on the CPU.

|got - restatement| <= 2e-6 max(1, max|restatement|) (EC.BAR: same products, other float32 summation order); the plain float64
convolution is held at test_gpu_conv.py's TOL.  halo_s32's sigmoid goes through the fast exponential and is held to EC.BAR + 1e-5
(EC.score_bound's figure for the fast exponentials and reciprocals).  Operands are channel slices of wider tensors whose unread channels
are NaN (S32: every bf16 of an unread group), per-image bias rows have NaN between them, outputs are windows of sentinel-filled buffers
with guards in front and behind.  An S32 output must be split() of the fp32 output of the same call, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import conv_edge_cases as EC
import conv_products_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
FMT = {"f32": 0, "s32": 1}
NAN_BF16_PAIR = 0x7FC07FC0                 # two bf16 NaN patterns (as float32 bits: a NaN too)
S32_SENTINEL_PAIR = 0xC342C342 - (1 << 32)  # two bf16 of EC.S32_SENTINEL (-194.0 = 0xC342), as an int32
S32_FAST_SIGMOID = 1e-5


def _mods():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    return _lib, E


def _guarded(t=None, shape=None, fill=0.0, bits=None):
    """a float32 device view with EC.GUARD elements in front and behind; bits: fill with this int32 pattern instead of the value `fill`"""
    n = int(np.prod(shape if t is None else t.shape))
    whole = torch.empty(n + 2 * EC.GUARD, dtype=torch.float32, device=DEV)
    if bits is None:
        whole.fill_(fill)
    else:
        whole.view(torch.int32).fill_(bits)
    view = whole[EC.GUARD:EC.GUARD + n].view(tuple(shape if t is None else t.shape))
    if t is not None:
        view.copy_(t)
    return view, whole


def _guards_hold(whole, pristine):
    return bool(torch.equal(whole[:EC.GUARD].view(torch.int32), pristine[:EC.GUARD].view(torch.int32))
                and torch.equal(whole[-EC.GUARD:].view(torch.int32), pristine[-EC.GUARD:].view(torch.int32)))


def _ratios(got, want, plain):
    return (float((got - want).abs().max()) / max(1.0, float(want.abs().max())),
            float((got - plain).abs().max()) / max(1.0, float(plain.abs().max())))


# ---- ape_conv3x3_halo_bf16 ------------------------------------------------------------------------------------------------------------------------
class _Halo:
    def __init__(self, name, nsplit):
        self.lib, E = _mods()
        self.nsplit = nsplit
        g, x, w, bias, res = EC.halo_inputs(name)
        self.g, self.M = g, g["B"] * g["H"] * g["W"]
        self.x = _guarded(x, fill=EC.NAN)[0]
        self.bias = None if bias is None else _guarded(bias, fill=EC.NAN)[0]
        self.res = None if res is None else _guarded(res, fill=EC.NAN)[0]
        self.conv = E.Conv(w, None, 1, g["dil"], g["dil"], g["act"], alpha=g["alpha"], device=DEV, precision=EC.PRECISION[nsplit])

    def new_y(self):
        return _guarded(shape=(self.M, self.g["ldy"]), fill=EC.Y_SENTINEL)

    def run(self, y, nsplit=None, null=(), **change):
        """null: the pointer arguments ("x", "w", "y", "params") passed as NULL"""
        d = self.lib.dptr
        p = self.lib.ConvParams(**dict(self.g, **change))
        return self.lib.lib().ape_conv3x3_halo_bf16(d(None if "x" in null else self.x), d(None if "w" in null else self.conv.wp), d(self.bias),
                                                    d(self.res), d(None if "y" in null else y), None if "params" in null else ctypes.byref(p),
                                                    self.nsplit if nsplit is None else nsplit, self.lib.stream_ptr())


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", list(EC.HALO_CASES))
def test_halo_against_its_own_products(name, nsplit):
    c = _Halo(name, nsplit)
    g, M, Cout, yoff = c.g, c.M, c.g["Cout"], c.g["yoff"]
    if g["ups"]:
        # the restatement's up-sampling is the library's, bit for bit: otherwise the restatement is wrong, not the fused kernel
        _, E = _mods()
        xs = EC.halo_inputs(name)[1][..., g["xoff"]:g["xoff"] + g["Cin"]].contiguous()
        assert torch.equal(E.bilinear(xs.to(DEV), g["H"], g["W"], True).cpu(), R.ups2x_f32(xs)), name
    y, whole = c.new_y()
    pristine = whole.clone()
    assert c.run(y) == 0
    y2, whole2 = c.new_y()
    assert c.run(y2) == 0
    torch.cuda.synchronize()
    assert torch.equal(whole, whole2)                                     # two calls: the same bits
    assert _guards_hold(whole, pristine)
    yc = y.cpu()
    assert not torch.isnan(yc).any()
    assert (yc[:, :yoff] == EC.Y_SENTINEL).all() and (yc[:, yoff + Cout:] == EC.Y_SENTINEL).all()
    got = yc[:, yoff:yoff + Cout].double()
    assert (got != EC.Y_SENTINEL).all()                                   # every element of the window was written
    r, r0 = _ratios(got, EC.halo_expected(name, nsplit), EC.halo_expected(name, 0))
    print("halo %s nsplit %d: %.3g of the output scale against its own products (%.0f %% of the bar), %.3g against the plain conv"
          % (name, nsplit, r, 100 * r / EC.BAR, r0))
    assert r <= EC.BAR, (name, nsplit, r)
    assert r0 <= EC.TOL[nsplit], (name, nsplit, r0)


def test_halo_refusals_leave_y_untouched():
    c = _Halo("d1_n128_1x16x16_one_full_tile_cin96_cout128_vector_residual_slice", 3)
    y, whole = c.new_y()
    refused = [dict(ldx=106), dict(xoff=6), dict(ldx=100), dict(ldy=132), dict(ldr=128), dict(act=4), dict(act=-1), dict(dil=3, pad=3), dict(pad=2),
               dict(stride=2), dict(KH=1, KW=1), dict(Cin=48), dict(Cin=0), dict(Ho=15), dict(Wo=15), dict(H=0, Ho=0), dict(W=0, Wo=0), dict(Cout=0), dict(B=-1), dict(ups=2),
               dict(ups=1, H=15, Ho=15), dict(ups=1, W=15, Wo=15), dict(ups=1, dil=2, pad=2)]
    g = c.g
    assert (g["ldx"], g["xoff"], g["Cin"], g["ldy"], g["yoff"], g["Cout"], g["ldr"], g["roff"]) == (104, 8, 96, 140, 8, 128, 136, 4)      # what the changes rest on
    for change in refused:
        assert c.run(y, **change) == EINVAL, change
    assert c.run(y, nsplit=2) == EINVAL and c.run(y, nsplit=0) == EINVAL
    for null in ("x", "w", "y", "params"):
        assert c.run(y, null=(null,)) == EINVAL, null
    # (the two 2^31 clauses -- B H W ldx and Cout Kp -- have no geometry here: were one of them not refused, the call would run out of its buffers)
    assert c.run(y, B=0) == 0                                            # an empty batch: nothing to do
    torch.cuda.synchronize()
    assert (whole == EC.Y_SENTINEL).all()


def test_halo_seghead_refusals_leave_its_outputs_untouched():
    _lib, E = _mods()
    gen = torch.Generator().manual_seed(9)
    conv = E.Conv(torch.randn(64, 32, 3, 3, generator=gen) / 17.0, None, 1, 1, 1, E.ACT_RELU, device=DEV, precision="bf16x3")
    x = torch.randn(1, 4, 6, 32, generator=gen).to(DEV)
    hw, hb = torch.randn(5, 64, generator=gen).to(DEV), torch.randn(5, generator=gen).to(DEV)
    label = torch.full((24,), EC.LABEL_SENTINEL, dtype=torch.uint8, device=DEV)
    score = torch.full((24,), EC.SCORE_SENTINEL, device=DEV)
    g = R.halo_geometry(1, 4, 6, 32, 64, 1)

    def run(C=5, nsplit=3, null=(), **change):
        p = _lib.ConvParams(**dict(g, **change))
        a = dict(x=x, w=conv.wp, head_w=hw, label=label, score=score)
        a = {k: _lib.dptr(None if k in null else v) for k, v in a.items()}
        return _lib.lib().ape_conv3x3_halo_seghead_bf16(a["x"], a["w"], None, None if "params" in null else ctypes.byref(p), nsplit, a["head_w"],
                                                        _lib.dptr(hb), C, a["label"], a["score"], 1, _lib.stream_ptr())

    for change in (dict(Cout=128, ldy=128), dict(dil=2, pad=2), dict(ldx=34), dict(xoff=4), dict(act=4), dict(ups=2), dict(ups=1, H=3, Ho=3),
                   dict(ups=1, W=5, Wo=5), dict(B=-1), dict(Cin=16), dict(Cin=48), dict(H=0, Ho=0), dict(W=0, Wo=0), dict(Ho=3), dict(Wo=5), dict(stride=2),
                   dict(pad=2), dict(KH=1, KW=1), dict(act=-1)):
        assert run(**change) == EINVAL, change
    for null in ("x", "w", "params", "head_w", "label", "score"):
        assert run(null=(null,)) == EINVAL, null
    assert run(C=0) == EINVAL and run(C=17) == EINVAL and run(nsplit=2) == EINVAL
    assert run(B=0) == 0
    torch.cuda.synchronize()
    assert (label == EC.LABEL_SENTINEL).all() and (score == EC.SCORE_SENTINEL).all()
    assert run() == 0
    torch.cuda.synchronize()
    assert (score != EC.SCORE_SENTINEL).all()


# ---- ape_conv3x3_halo_s32 ---------------------------------------------------------------------------------------------------------------------------
def _ncu():
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert ncu % 16 == 0, ncu
    return ncu


class _HaloS32:
    def __init__(self, name, ncu):
        self.lib, E = _mods()
        g, x, w, bias, res, out = EC.halo_s32_inputs(name, ncu)
        self.g, self.M, self.out = g, g["B"] * g["H"] * g["W"], out
        self.x = _guarded(R.s32_pack(*x), bits=NAN_BF16_PAIR)[0]
        self.bias = None if bias is None else _guarded(bias, fill=EC.NAN)[0]
        self.res, self.res_fmt = None, FMT["f32"]
        if isinstance(res, tuple):
            self.res, self.res_fmt = _guarded(R.s32_pack(*res), bits=NAN_BF16_PAIR)[0], FMT["s32"]
        elif res is not None:
            self.res = _guarded(res, fill=EC.NAN)[0]
        self.conv = E.Conv(w, None, 1, g["dil"], g["dil"], g["act"], alpha=g["alpha"], device=DEV, precision="bf16x3")
        self.ws = self.conv.s32k()

    def new_y(self, out):
        if out == "s32":
            return _guarded(shape=(self.M, self.g["ldy"]), bits=S32_SENTINEL_PAIR)
        return _guarded(shape=(self.M, self.g["ldy"]), fill=EC.Y_SENTINEL)

    def run(self, y, out, null=(), res_fmt=None, out_fmt=None, **change):
        """null: the pointer arguments ("x", "w", "y", "params") passed as NULL"""
        d = self.lib.dptr
        p = self.lib.ConvParams(**dict(self.g, **change))
        return self.lib.lib().ape_conv3x3_halo_s32(d(None if "x" in null else self.x), d(None if "w" in null else self.ws), d(self.bias), d(self.res),
                                                   self.res_fmt if res_fmt is None else res_fmt, d(None if "y" in null else y),
                                                   FMT[out] if out_fmt is None else out_fmt, None if "params" in null else ctypes.byref(p),
                                                   self.lib.stream_ptr())


@pytest.mark.parametrize("name", EC.HALO_S32_NAMES)
def test_halo_s32_against_its_own_products_under_both_schedules(name):
    ncu = _ncu()
    c = _HaloS32(name, ncu)
    g, M, Cout, yoff, out = c.g, c.M, c.g["Cout"], c.g["yoff"], c.out
    outs = ["f32"] + (["s32"] if out == "s32" else [])
    ys = {o: [c.new_y(o) for _ in range(3)] for o in outs}
    pristine = {o: ys[o][0][1].clone() for o in outs}
    lib = c.lib.lib()
    try:
        for o in outs:
            assert c.run(ys[o][0][0], o) == 0 and c.run(ys[o][1][0], o) == 0          # the product (ping-pong) schedule, twice
        lib.ape_conv3x3_halo_s32_debug(4096)
        for o in outs:
            assert c.run(ys[o][2][0], o) == 0                                          # the lockstep schedule
    finally:
        lib.ape_conv3x3_halo_s32_debug(0)
    torch.cuda.synchronize()
    for o in outs:
        w0, w1, w2 = (ys[o][k][1].view(torch.int32) for k in range(3))
        assert torch.equal(w0, w1), (name, o)                                          # two calls: the same bits
        assert torch.equal(w0, w2), (name, o)                                          # both schedules: the same bits
        assert _guards_hold(ys[o][0][1], pristine[o])
    yc = ys["f32"][0][0].cpu()
    assert not torch.isnan(yc).any()
    assert (yc[:, :yoff] == EC.Y_SENTINEL).all() and (yc[:, yoff + Cout:] == EC.Y_SENTINEL).all()
    got32 = yc[:, yoff:yoff + Cout]
    assert (got32 != EC.Y_SENTINEL).all()                                              # every element of the window was written
    if out == "s32":
        hi, lo = R.s32_unpack(ys["s32"][0][0].cpu())
        assert not torch.isnan(hi).any() and not torch.isnan(lo).any()
        for plane in (hi, lo):                                                         # the unwritten channels keep their sentinel pattern
            assert (plane[:, :yoff] == EC.S32_SENTINEL).all() and (plane[:, yoff + Cout:] == EC.S32_SENTINEL).all()
        wh, wl = R.split(got32)
        assert torch.equal(hi[:, yoff:yoff + Cout].view(torch.int32), wh.view(torch.int32)), name        # == split(fp32 output), bit for bit
        assert torch.equal(lo[:, yoff:yoff + Cout].view(torch.int32), wl.view(torch.int32)), name
    r, r0 = _ratios(got32.double(), EC.halo_s32_expected(name, 3, ncu), EC.halo_s32_expected(name, 0, ncu))
    bar = EC.BAR + (S32_FAST_SIGMOID if g["act"] == R.ACT_SIGMOID else 0.0)
    print("halo_s32 %s: %.3g of the output scale against its own products (%.0f %% of the bar%s), %.3g against the plain conv"
          % (name, r, 100 * r / bar, ", fast sigmoid: ratio to 2e-6 + 1e-5 = %.3f" % (r / bar) if g["act"] == R.ACT_SIGMOID else "", r0))
    assert r <= bar, (name, r)
    assert r0 <= EC.TOL[3], (name, r0)


def test_halo_s32_refusals_leave_y_untouched():
    c = _HaloS32("d2_1x17x9_last_tile_row_rpw1_f32_residual_per_image_bias", 256)
    y, whole = c.new_y("f32")
    S = FMT["s32"]
    refused = [dict(ldx=68), dict(xoff=16, ldx=96), dict(xoff=32), dict(Cout=124), dict(Cout=130), dict(ldy=128), dict(ldy=142), dict(yoff=2),
               dict(out_fmt=S), dict(ldr=128), dict(ldr=138), dict(roff=2), dict(res_fmt=S), dict(out_fmt=2), dict(res_fmt=2), dict(act=4), dict(act=-1),
               dict(ups=1), dict(dil=3, pad=3), dict(pad=1), dict(stride=2), dict(KH=1, KW=1), dict(Cin=16), dict(Cin=48), dict(Ho=16), dict(Wo=8),
               dict(H=0, Ho=0), dict(W=0, Wo=0), dict(B=-1)]
    g = c.g
    assert (g["W"], g["ldx"], g["xoff"], g["Cin"], g["ldy"], g["yoff"], g["Cout"], g["ldr"], g["roff"]) == (9, 64, 0, 64, 140, 4, 128, 140, 4)     # what the changes rest on
    assert c.res is not None and c.res_fmt == FMT["f32"]
    for change in refused:
        assert c.run(y, "f32", **change) == EINVAL, change
    for null in ("x", "w", "y", "params"):
        assert c.run(y, "f32", null=(null,)) == EINVAL, null
    # (the two 2^31 clauses have no geometry here either: a call that slipped through would run out of its buffers)
    assert c.run(y, "f32", B=0) == 0                                      # an empty batch: nothing to do
    torch.cuda.synchronize()
    assert (whole == EC.Y_SENTINEL).all()

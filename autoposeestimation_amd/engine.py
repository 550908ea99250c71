"""Thin host layer over the C ABI (include/ape_hip.h): weight repacking into the device layout and one Python
function per kernel.  Tensors are torch CUDA(HIP) tensors used purely as device buffers; every function enqueues on
torch's current stream and returns without synchronising.  No function here has a CPU path.

Device layout (DESIGN.md "Data layout in HBM"): activations NHWC fp32 `[B,H,W,C]` (points are `[B,N,1,C]`),
weights `[Cout][KH][KW][Cin4]` with Cin zero-padded to a multiple of 4.
"""
import contextlib
import contextvars
import ctypes
import os

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_PRELU, ACT_RELU, ACT_SIGMOID, ConvParams  # noqa: F401


def _st():
    return _lib.stream_ptr()


class LaunchProfile:
    """Optional per-launch HIP-event timing of the heavy kernels on torch's current stream (bench.py's roofline leg).
    Events are recorded on the very stream the kernel is enqueued on; durations are read after the final sync.
    A record = (kernel label as rocprofv3 spells it, shape string, algorithmic flop, algorithmic bytes, start, end): the flop are
    2 * M * Cout * KH * KW * Cin of the convolution the launch evaluates, the bytes its activations in + weights + residual +
    output, each counted once (what a perfect kernel would move)."""

    def __init__(self, only=None):
        self.records = []
        self.only = only        # None: time every profiled launch; else a set of labels (the others run un-timed, without
                                # the two event packets per launch that cost ~4 us of dispatch gap each)

    def wants(self, label):
        return self.only is None or label in self.only

    def begin(self, label):
        """-> a start event, or None when this label is not being timed"""
        if not self.wants(label):
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    def end(self, e0, label, shape, flop, nbytes):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.append((label, shape, float(flop), float(nbytes), e0, e1))

    def summary(self, by_shape=False):
        out = {}
        for name, shape, flop, nbytes, e0, e1 in self.records:
            key = (name, shape) if by_shape else name
            d = out.setdefault(key, {"launches": 0, "flop": 0.0, "bytes": 0.0, "ms": 0.0})
            d["launches"] += 1
            d["flop"] += flop
            d["bytes"] += nbytes
            d["ms"] += e0.elapsed_time(e1)
        return out


def _prof_begin(label):
    prof = PROFILE
    return None if prof is None else prof.begin(label)


def _prof_end(e0, label, shape, flop, nbytes):
    if e0 is not None and PROFILE is not None:
        PROFILE.end(e0, label, shape, flop, nbytes)


def _conv_cost(conv, b, h_in, w_in, ho, wo, residual):
    """(algorithmic flop, algorithmic bytes) of one conv launch: see LaunchProfile"""
    flop = 2.0 * b * ho * wo * conv.cout * conv.kh * conv.kw * conv.cin_real
    nbytes = 4.0 * (b * h_in * w_in * conv.cin_real + conv.cout * conv.kh * conv.kw * conv.cin_real + b * ho * wo * conv.cout * (2 if residual else 1))
    return flop, nbytes


PROFILE = None   # set to a LaunchProfile() to time conv launches

# operand precision of the dense contractions (accumulation is always fp32):
#   "f32"    exact fp32 MFMA (v_mfma_f32_32x32x2_f32)                 157 TFLOP/s peak
#   "bf16x3" split-bf16, 3 products per term, ~2^-16 operand error      833 TFLOP/s effective peak
#   "bf16"   plain bf16 operands (2^-8)                                 2.5 PFLOP/s peak
PRECISIONS = ("f32", "bf16x3", "bf16")
USE_HALO_KERNEL = True    # route eligible 3x3 convs of the bf16 paths to the LDS-halo kernel (conv3x3_halo.hip)
USE_GEMM_KERNEL = os.environ.get("APE_USE_GEMM_KERNEL", "1") != "0"    # route Cin % 32 == 0 layers the halo kernel does not take to conv_gemm.hip (else conv_bf16.hip)
USE_CONV_MULTI = os.environ.get("APE_USE_CONV_MULTI", "1") != "0"     # the PSP stage convolutions in one launch (conv1x1_multi); 0: one launch each (A/B)
GEMM_VARIANT = int(os.environ.get("APE_GEMM_VARIANT", "0"))          # 0 = chosen from the shape; 1..4 force a block shape (tools/microbench_generic.py)
USE_GEMM_ROWS = os.environ.get("APE_USE_GEMM_ROWS", "1") != "0"      # pure 1x1 layers of at most GEMM_ROWS_MAX_M rows take conv_rows_kernel (conv_gemm.hip variant 7); 0: the block shapes only (A/B)
GEMM_ROWS_MAX_M = 128                                                # = ROWS_MAX_M of conv_gemm.hip
USE_POINT_FEAT = os.environ.get("APE_USE_POINT_FEAT", "1") != "0"    # the point-feature front of the pose networks in one launch (point_feat.hip); 0: its five launches (A/B)


FMT_F32, FMT_S32 = 0, 1
USE_S32 = os.environ.get("APE_USE_S32", "1") != "0"    # pre-split activations between the segmentor's bf16x3 layers (conv_gemm_s32.hip)


class S32:
    """A pre-split activation tensor (include/ape_hip.h "S32"): per pixel and 32-channel group 128 bytes [hi 32 x bf16 | lo 32 x bf16].
    Same bytes per channel as fp32, so it lives in a float32 torch tensor `t` of the logical shape [B,H,W,C]; only kernels that
    declare S32 operands may read it (the element values of `t` are NOT the activations)."""
    __slots__ = ("t",)

    def __init__(self, t):
        if t.dtype != torch.float32 or t.shape[-1] % 32:
            raise ValueError("S32 needs a float32 buffer with a multiple of 32 channels")
        self.t = t

    @property
    def shape(self):
        return self.t.shape

    @property
    def device(self):
        return self.t.device

    def __getitem__(self, idx):          # batch slicing only
        return S32(self.t[idx])

    def to_f32(self):
        y = torch.empty_like(self.t)
        c = self.t.shape[-1]
        _lib.call.ape_convert_s32(_lib.dptr(self.t, torch.float32), _lib.dptr(y), self.t.numel() // c, c, 0, _st())
        return y

    @staticmethod
    def from_f32(x):
        y = torch.empty_like(x)
        c = x.shape[-1]
        _lib.call.ape_convert_s32(_lib.dptr(x, torch.float32), _lib.dptr(y), x.numel() // c, c, 1, _st())
        return S32(y)


PF_X, PF_EMB = 1, 2                    # APE_POINT_FEAT_X / _EMB: the halves of the point-feature front
POINT_FEAT_LABEL = "point_feat_kernel"


def point_feat(x4, emb, conv1, e_conv1, conv2, e_conv2, pf=None, pf_s32=None, parts=PF_X | PF_EMB):
    """The front of PoseNetFeat / PoseRefineNetFeat in one launch (ape_point_feat_bf16): x4[..,4], emb[..,32] -> the rows
    [conv1 64 | e_conv1 64 | conv2 128 | e_conv2 128] into pf ([..,384] f32) and / or pf_s32 (an `S32` of the same shape), whichever is
    given; `parts` selects the x half, the emb half or both (the other half's columns are left as they are).  The layers are the `Conv`
    objects of the five-launch route, in 'bf16x3'; every value is bit for bit what that route gives."""
    layers = (conv1, e_conv1, conv2, e_conv2)
    want = ((64, 4), (64, 32), (128, 64), (128, 64))
    for c, (cout, cin) in zip(layers, want):
        if (c.nsplit != 3 or (c.cout, c.cin, c.kh, c.kw) != (cout, cin, 1, 1) or c.stride != 1 or c.pad != 0 or c.act != ACT_RELU
                or c.bias is None):
            raise ValueError("point_feat needs the bf16x3 1x1 ReLU layers 4->64, 32->64, 64->128, 64->128 with biases")
    if pf is None and pf_s32 is None:
        raise ValueError("point_feat needs an output buffer")
    m = x4.numel() // 4
    if x4.shape[-1] != 4 or emb.shape[-1] != 32 or emb.numel() != m * 32:
        raise ValueError("point_feat takes x4[..,4] and emb[..,32] of the same rows")
    for t in (pf, None if pf_s32 is None else pf_s32.t):
        if t is not None and (t.shape[-1] != 384 or t.numel() != m * 384):
            raise ValueError("point_feat output buffer %s does not hold %d rows of 384" % (tuple(t.shape), m))
    e0 = _prof_begin(POINT_FEAT_LABEL)
    _lib.call.ape_point_feat_bf16(_lib.dptr(x4, torch.float32), _lib.dptr(emb, torch.float32),
                                  _lib.dptr(conv1.wp), _lib.dptr(conv1.bias), _lib.dptr(e_conv1.wp), _lib.dptr(e_conv1.bias),
                                  _lib.dptr(conv2.wp), _lib.dptr(conv2.bias), _lib.dptr(e_conv2.wp), _lib.dptr(e_conv2.bias),
                                  _lib.dptr(pf, torch.float32), _lib.dptr(None if pf_s32 is None else pf_s32.t, torch.float32),
                                  m, parts, 3, _st())
    if e0 is not None:
        cols = (192 if parts & PF_X else 0) + (192 if parts & PF_EMB else 0)
        k = (4 * 64 + 64 * 128 if parts & PF_X else 0) + (32 * 64 + 64 * 128 if parts & PF_EMB else 0)
        nout = (pf is not None) + (pf_s32 is not None)
        _prof_end(e0, POINT_FEAT_LABEL, "%dx%d parts%d out%d" % (m, cols, parts, nout), 2.0 * m * k,
                  4.0 * m * ((4 if parts & PF_X else 0) + (32 if parts & PF_EMB else 0) + cols * nout) + 4.0 * k)
    return pf, pf_s32


def pack_conv_weight(w, device):
    """[Cout,Cin,KH,KW] | [Cout,Cin,1] | [Cout,Cin]  ->  contiguous f32 [Cout,KH,KW,Cin4] on `device`."""
    w = w.detach()
    if w.dim() == 2:
        w = w[:, :, None, None]
    elif w.dim() == 3:
        w = w[:, :, :, None]
    cout, cin, kh, kw = w.shape
    cin4 = (cin + 3) // 4 * 4
    out = torch.zeros(cout, kh, kw, cin4, dtype=torch.float32, device=device)
    out[..., :cin] = w.to(device=device, dtype=torch.float32).permute(0, 2, 3, 1)
    return out.contiguous()


# 3x3 layers on S32 inputs with these input channel counts take the half-pass kernel (fp16 main product + block-scaled e2m3 cross terms,
# conv3x3_halo_mx.hip) instead of halo_s32's three bf16 products.  Off unless asked for: not bit-identical to bf16x3.
USE_MX6 = os.environ.get("APE_USE_MX6", "0") != "0"
MX6_CIN = tuple(int(v) for v in os.environ.get("APE_MX6_CIN", "512").split(","))


_POSE_STAGE = contextvars.ContextVar("ape_low_latency_pose_stage", default=False)


@contextlib.contextmanager
def low_latency(on=True):
    """Inside this block (of this thread / context only) the layers built with `Conv(..., splitk=True)` take the split-K form at small M:
    the batch-1 pose stage of FramePipeline(low_latency=True).  Layers built without the keyword -- the segmentor's -- never do."""
    token = _POSE_STAGE.set(bool(on))
    try:
        yield
    finally:
        _POSE_STAGE.reset(token)


def _tf(v):
    return "true" if v else "false"


def tiles16_mostly_full(h, w):
    """the LDS-halo kernels tile an h x w map in 16x16 pixels: worth it only when those tiles are mostly full (crop feature maps of
    20x20 / 40x40 would waste 30..60 % of the MFMAs; the flattened-M kernels have no such edge effect)"""
    return h * w >= 0.8 * (-(-h // 16) * -(-w // 16) * 256)


# ---- profiling labels: the kernel names as rocprofv3 spells them (bench.py finds a kernel's HBM traffic in profiles/*_pmc_traffic.json by
# them), one function per kernel family, and the shape string of a conv launch
def halo_label(nsplit, dil, cout, ups, head=False):
    return "conv3x3_halo_kernel<%d,%d,%d,%s,%s>" % (nsplit, dil, 64 if cout <= 64 else 128, _tf(ups), _tf(head))


def halo_s32_label(dil):
    return "halo_s32_kernel<%d, true>" % dil          # <dilation, ping-pong schedule>


def halo_mx_label(dil):
    return "halo_mx_kernel<%d>" % dil


def gemm_s32_label(cout, residual=False):
    bn = 128 if cout <= 128 else 192 if (-(-cout // 192) * 192 - cout) < (-(-cout // 256) * 256 - cout) else 256
    return ("gemm_s32_res_kernel<%d, false>" if residual else "gemm_s32_kernel<%d, false>") % bn


def conv_shape(conv, b, ho, wo, ups=False):
    return "%dx%dx%d %d->%d k%d s%d d%d%s" % (b, ho, wo, conv.cin_real, conv.cout, conv.kh, conv.stride, conv.dil, " ups" if ups else "")


def conv_params(conv, b, h, w, ldx, ldy, xoff=0, yoff=0, act=None, bias_bstride=0, ldr=0, roff=0, ups=False):
    """the `ape_conv_params` of `conv` on a [b,h,w,ldx] input (h, w: of the up-sampled map when `ups`) writing a map of ldy channels;
    ldr / roff: the residual's channels per pixel (0: none) and offset; act: None = the layer's own"""
    ho, wo = conv.out_hw(h, w)
    return ConvParams(B=b, H=h, W=w, Cin=conv.cin, ldx=ldx, xoff=xoff, Ho=ho, Wo=wo, Cout=conv.cout, ldy=ldy, yoff=yoff, KH=conv.kh, KW=conv.kw,
                      stride=conv.stride, pad=conv.pad, dil=conv.dil, act=conv.act if act is None else act, alpha=conv.alpha,
                      bias_bstride=bias_bstride, ldr=ldr, roff=roff, ups=int(bool(ups)))


def _nsplit(precision):
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s" % (PRECISIONS,))
    return {"f32": 0, "bf16x3": 3, "bf16": 1}[precision]


# argument layouts of the conv entry points (Conv._make_plan picks one with the entry point, Conv.__call__ passes the operands accordingly)
_ARGS_F32, _ARGS_BF16, _ARGS_GEMM, _ARGS_SPLITK, _ARGS_S32, _ARGS_MX = range(6)


class Conv:
    """One conv / 1x1 / Linear layer bound to ape_conv2d_nhwc_f32 or, in the bf16 precisions, to the kernel of its family that takes the
    call's geometry.  splitk: the layer may take the split-K form at small M inside `low_latency()` (the pose networks' layers)."""

    def __init__(self, weight, bias=None, stride=1, pad=0, dil=1, act=ACT_NONE, alpha=0.0, device="cuda", precision="f32", splitk=False):
        nsplit = _nsplit(precision)          # (refuses an unknown precision before anything is packed)
        w, wp = pack_conv_weight(weight, device), None
        if nsplit:
            cout, kh, kw, cin = w.shape
            wp = torch.empty(_lib.lib().ape_packed_weights_bf16_elems(cout, kh * kw * cin), dtype=torch.bfloat16, device=device)
            _lib.call.ape_pack_weights_bf16(_lib.dptr(w), _lib.dptr(wp), cout, kh * kw * cin, _st())
        self._bind(w, wp, weight.shape[1], stride, pad, dil, act, alpha, precision, splitk)
        self.bias = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()

    @classmethod
    def from_packed(cls, w, wp, cin_real, stride=1, pad=0, dil=1, act=ACT_NONE, alpha=0.0, precision="f32", splitk=False):
        """a layer over operands that are ALREADY packed (w: f32 [Cout,KH,KW,Cin4]; wp: the split-bf16 planes of the same weights, needed
        unless precision == 'f32'): the training tape keeps them per parameter and re-packs them after each optimizer step
        (autograd.WeightBank), instead of packing per call"""
        self = cls.__new__(cls)
        self._bind(w, wp, cin_real, stride, pad, dil, act, alpha, precision, splitk)
        self.bias = None
        return self

    def _bind(self, w, wp, cin_real, stride, pad, dil, act, alpha, precision, splitk):
        """geometry, precision and kernel variant names of a layer over the packed operands (w, wp); its caches start empty"""
        self.nsplit = _nsplit(precision)
        self.precision = precision
        self.w = w
        self.cout, self.kh, self.kw, self.cin = w.shape
        self.cin_real = cin_real
        if self.nsplit:
            if wp is None:
                raise ValueError("precision %s needs the packed bf16 planes" % precision)
            self.wp = wp
            self.variant = "conv_bf16_kernel<%d,%s>" % (self.nsplit, "128,128,2,2,64,false" if self.cout > 64 else "128,64,4,1,32,true")
        else:
            self.variant = "conv_f32_kernel<%s>" % ("128,2,2" if self.cout > 64 else "64,4,1" if self.cout > 32 else "32,4,1")
        self.stride, self.pad, self.dil, self.act, self.alpha = stride, pad, dil, act, float(alpha)
        self.splitk = bool(splitk)
        self._plans, self._ws32, self._wmx6 = {}, None, None

    def s32k(self):
        """the weights in the S32K grouping ([Cout][K/32][hi 32 | lo 32] bf16) for the S32 consumers; built on first use"""
        if self._ws32 is None:
            k = self.kh * self.kw * self.cin
            ws = torch.empty(self.cout * k * 2, dtype=torch.bfloat16, device=self.w.device)
            _lib.call.ape_pack_weights_s32k(_lib.dptr(self.w), _lib.dptr(ws), self.cout, k, _st())
            self._ws32 = ws
        return self._ws32

    def mx6k(self):
        """the weights as F16M6 lines ([Cout][9 * Cin / 32][128 B], mx6.pack_conv_weights) for ape_conv3x3_halo_mx; built on first use"""
        if self._wmx6 is None:
            from . import mx6
            w = self.w.detach().float().cpu().numpy().reshape(self.cout, self.kh, self.kw, self.cin)       # (the unpacked layout: [Cout][kh][kw][Cin])
            lines = mx6.pack_lines(w.reshape(self.cout, self.kh * self.kw * (self.cin // 32), 32))
            self._wmx6 = torch.from_numpy(lines).to(self.w.device)
        return self._wmx6

    def _generic_variant(self, m):
        """name of the template instantiation ape_conv2d_nhwc_* dispatches to (mirrors the C++ rule; profiling label only)"""
        if self.nsplit and self.cout >= 256 and ((-(-self.cout // 256)) * 256 - self.cout) * 8 <= self.cout and m >= 65536:
            return "conv_bf16_kernel<%d,256,256,4,2,32,true>" % self.nsplit
        return self.variant

    def _gemm_variant(self, m, residual=False, out_fmt=FMT_F32):
        """name of the conv_gemm.hip instantiation ape_conv_gemm_bf16_fmt dispatches to (mirrors the C++ rule; profiling label only)"""
        pure = "true" if (self.kh == 1 and self.kw == 1 and self.stride == 1 and self.pad == 0) else "false"
        v = GEMM_VARIANT & 15
        if v == 0:
            k = self.kh * self.kw * self.cin
            if (m <= GEMM_ROWS_MAX_M and USE_GEMM_ROWS and not (GEMM_VARIANT & 0x100) and pure == "true" and not residual
                    and out_fmt == FMT_F32):
                v = 7
            elif self.cout <= 64:
                v = 3
            elif (self.cout >= 256 and ((-(-self.cout // 256)) * 256 - self.cout) * 8 <= self.cout and k >= 256
                  and -(-m // 256) * -(-self.cout // 256) >= 192):
                v = 1
            elif (self.cout >= 192 and ((-(-self.cout // 192)) * 192 - self.cout) * 8 <= self.cout and k >= 256
                  and -(-m // 256) * -(-self.cout // 192) >= 192):
                v = 4
            else:
                v = 2
        if v == 7:
            return "conv_rows_kernel<%d>" % self.nsplit
        # the same spelling as rocprofv3's kernel name (template arguments NSPLIT, BM, BN, WM, WN, PURE, PP), so that bench.py finds
        # this kernel's HBM traffic in profiles/*_pmc_traffic.json
        return "conv_gemm_kernel<%d,%s,%s,%s>" % (self.nsplit, {1: "256,256,2,4", 2: "128,128,2,2", 3: "256,64,4,1", 4: "256,192,2,4",
                                                               5: "256,256,2,4", 6: "128,192,2,2"}[v], pure, "true" if v == 5 else "false")

    def out_hw(self, h, w):
        ho = (h + 2 * self.pad - self.dil * (self.kh - 1) - 1) // self.stride + 1
        wo = (w + 2 * self.pad - self.dil * (self.kw - 1) - 1) // self.stride + 1
        return ho, wo

    def _make_plan(self, key):
        """The launch of one call signature (`key`: see __call__): the parameter block, the kernel family that takes it -- f32 generic, bf16
        generic, LDS-halo, conv_gemm plain / _fmt / split-K for fp32 inputs; halo_mx, halo_s32, gemm_s32 for S32 inputs -- as (argument
        layout, checked entry point), the launch's profiling label and shape string and its algorithmic cost.  Depends on shapes and on the
        module switches in the key only: kept per signature (the training tape calls every layer with the same shapes step after step;
        building the ctypes struct and asking the library twice cost ~15 us per call)."""
        b, h, w, ldx, xoff, ldy, yoff, act, bias_bstride, ldr, roff, ups, splitk, in_fmt, out_fmt = key[:15]
        p = conv_params(self, b, h, w, ldx, ldy, xoff, yoff, act, bias_bstride, ldr, roff, ups)
        pref, L, m = ctypes.byref(p), _lib.lib(), b * p.Ho * p.Wo
        sk_bytes = 0
        if in_fmt == FMT_S32:
            if self.kh != 3:
                if not L.ape_conv_gemm_s32_supported(pref):
                    raise ValueError("no S32 kernel for this layer geometry (%dx%d, stride %d, Cin %d, Cout %d)" % (self.kh, self.kw, self.stride, self.cin, self.cout))
                args, entry, label = _ARGS_S32, "ape_conv_gemm_s32", gemm_s32_label(self.cout, ldr != 0)
            elif (USE_MX6 and self.cin in MX6_CIN and self.cout >= 128 and self.stride == 1 and xoff == 0 and ldx == self.cin
                  and L.ape_conv3x3_halo_mx_supported(pref)):
                # half the matrix passes (conv3x3_halo_mx.hip): the S32 input is re-expressed once as F16M6 lines
                args, entry, label = _ARGS_MX, "ape_conv3x3_halo_mx", halo_mx_label(self.dil)
            else:
                if not L.ape_conv3x3_halo_s32_supported(pref):
                    raise ValueError("no S32 kernel for this layer geometry (3x3, stride %d, dil %d, Cin %d, Cout %d)" % (self.stride, self.dil, self.cin, self.cout))
                args, entry, label = _ARGS_S32, "ape_conv3x3_halo_s32", halo_s32_label(self.dil)
        else:
            halo = bool(self.nsplit and USE_HALO_KERNEL and (ups or tiles16_mostly_full(h, w)) and L.ape_conv3x3_halo_supported(pref))
            gemm = bool(not halo and self.nsplit and USE_GEMM_KERNEL and L.ape_conv_gemm_supported(pref))
            if out_fmt == FMT_S32 and not gemm:
                raise ValueError("an S32 output from an fp32 input exists only on the conv_gemm kernel (Cin % 32 == 0, not a halo layer)")
            if halo:
                args, entry, label = _ARGS_BF16, "ape_conv3x3_halo_bf16", halo_label(self.nsplit, self.dil, self.cout, ups)
            elif gemm:
                # k-tiles dealt to several workgroups per output tile where the library finds it worth it (fewer than 96 tiles and >= 8 k-tiles)
                sk_bytes = int(L.ape_conv_gemm_splitk_workspace_bytes(pref)) if splitk and out_fmt == FMT_F32 else 0
                args, entry = (_ARGS_SPLITK, "ape_conv_gemm_bf16_splitk") if sk_bytes else (_ARGS_GEMM, "ape_conv_gemm_bf16_fmt")
                label = self._gemm_variant(m, ldr != 0, out_fmt)
            else:
                args, entry = (_ARGS_BF16, "ape_conv2d_nhwc_bf16") if self.nsplit else (_ARGS_F32, "ape_conv2d_nhwc_f32")
                label = self._generic_variant(m)
        hin, win = (h // 2, w // 2) if ups else (h, w)
        if len(self._plans) > 64:
            self._plans.clear()
        plan = self._plans[key] = (p, pref, args, getattr(_lib.call, entry), sk_bytes, label, conv_shape(self, b, p.Ho, p.Wo, ups),
                                   *_conv_cost(self, b, hin, win, p.Ho, p.Wo, ldr != 0))
        return plan

    def __call__(self, x, out=None, xoff=0, yoff=0, residual=None, roff=0, bias=None, bias_bstride=0, act=None, upsample2x=False,
                 out_fmt=FMT_F32, splitk=False):
        """x[B,H,W,ldx] (reads channels xoff..xoff+cin) -> out[B,Ho,Wo,ldy] (writes yoff..yoff+cout).
        upsample2x: the conv runs on the bilinear x2 (align_corners=True) up-sampling of x, fused into the LDS-halo kernel
        when it applies, otherwise materialised by ape_bilinear_nhwc_f32 first.
        x / residual may be `S32` (pre-split) tensors and out_fmt=FMT_S32 returns one: only on the split-bf16 kernels that
        declare S32 operands (this never converts silently -- an unsupported combination raises).
        splitk: take the split-K form if the library finds the shape worth it (the training tape); layers built with splitk=True also do
        inside `low_latency()`."""
        in_fmt = FMT_S32 if isinstance(x, S32) else FMT_F32
        if in_fmt == FMT_S32 or isinstance(residual, S32):
            if self.nsplit != 3:
                raise ValueError("S32 operands exist only in the split-bf16 ('bf16x3') precision")
            if in_fmt != FMT_S32:
                raise ValueError("S32 output / residual needs an S32 input on this path")
            if upsample2x:
                raise ValueError("no S32 kernel up-samples its input")
            x = x.t
        if upsample2x:
            can_fuse = (self.nsplit and USE_HALO_KERNEL and self.kh == 3 and self.kw == 3 and self.stride == 1 and self.pad == 1
                        and self.dil == 1 and self.cin % 32 == 0 and x.shape[3] == self.cin and xoff == 0)
            if not can_fuse:
                return self(bilinear(x, 2 * x.shape[1], 2 * x.shape[2], True), out, 0, yoff, residual, roff, bias, bias_bstride, act)
        b, h, w, ldx = x.shape
        if upsample2x:
            h, w = 2 * h, 2 * w
        ho, wo = self.out_hw(h, w)
        if out is None:
            out = torch.empty(b, ho, wo, self.cout, dtype=torch.float32, device=x.device)
        elif isinstance(out, S32):
            out = out.t
        if tuple(out.shape[:3]) != (b, ho, wo):
            raise ValueError("conv output buffer %s does not match %s" % (tuple(out.shape), (b, ho, wo)))
        res_fmt = FMT_F32
        if residual is not None:
            if isinstance(residual, S32):
                residual, res_fmt = residual.t, FMT_S32
            if tuple(residual.shape[:3]) != (b, ho, wo):
                raise ValueError("residual shape mismatch")
        bias = self.bias if bias is None else bias
        # small-M layers of the POSE networks (one crop's 20 x 20 maps: 4..16 output tiles walking K = 4608 alone on a 256-CU chip) take the split-K
        # form inside `low_latency()` -- the batch-1 live loop of main.py:517-553; batches that fill the chip (the bench's 64 crops: 200+ tiles per
        # layer) never do.  Opt-in per layer (the `splitk` keyword of the constructor, passed by PoseNet / PoseRefineNet for their plans): the split
        # changes the fp32 summation order, and the SEGMENTOR's class maps must stay bit-identical between a frame run alone and the same
        # frame inside a batch (tests/test_gpu_bench_parity.py)
        splitk = bool(splitk or (self.splitk and _POSE_STAGE.get()))
        # the call signature: geometry and formats, then the module switches that take part in routing
        key = (b, h, w, ldx, xoff, out.shape[3], yoff, self.act if act is None else act, bias_bstride, 0 if residual is None else residual.shape[3], roff,
               bool(upsample2x), splitk, in_fmt, out_fmt, USE_HALO_KERNEL, USE_GEMM_KERNEL, GEMM_VARIANT, USE_MX6, MX6_CIN, USE_GEMM_ROWS)
        plan = self._plans.get(key) or self._make_plan(key)
        p, pref, args, fn, sk_bytes, label, shape, flop, nbytes = plan
        if p.alpha != self.alpha:
            p.alpha = self.alpha
        if args == _ARGS_MX:
            xq = torch.empty_like(x)
            _lib.call.ape_s32_to_f16m6(_lib.dptr(x, torch.float32), _lib.dptr(xq, torch.float32), b * h * w, ldx, _st())
            x = xq
        e0 = None if PROFILE is None else PROFILE.begin(label)
        xp, bp, rp, yp = _lib.dptr(x, torch.float32), _lib.dptr(bias), _lib.dptr(residual), _lib.dptr(out, torch.float32)
        if args == _ARGS_GEMM:
            fn(xp, _lib.dptr(self.wp), bp, rp, yp, out_fmt, pref, self.nsplit, GEMM_VARIANT if USE_GEMM_ROWS else GEMM_VARIANT | 0x100, _st())
        elif args == _ARGS_BF16:
            fn(xp, _lib.dptr(self.wp), bp, rp, yp, pref, self.nsplit, _st())
        elif args == _ARGS_S32:
            fn(xp, _lib.dptr(self.s32k()), bp, rp, res_fmt, yp, out_fmt, pref, _st())
        elif args == _ARGS_SPLITK:
            ws = torch.empty(sk_bytes, dtype=torch.uint8, device=x.device)
            fn(xp, _lib.dptr(self.wp), bp, rp, yp, pref, self.nsplit, _lib.dptr(ws), sk_bytes, _st())
        elif args == _ARGS_MX:
            fn(xp, _lib.dptr(self.mx6k()), bp, rp, res_fmt, yp, out_fmt, pref, _st())
        else:
            fn(xp, _lib.dptr(self.w), bp, rp, yp, pref, _st())
        if e0 is not None:
            _prof_end(e0, label, shape, flop, nbytes)
        return S32(out) if out_fmt == FMT_S32 else out


def conv_seg_head(conv, x, head_w, head_b, double_softmax=True, upsample2x=False):
    """`seg_head(conv(x))` for a 64-channel 3x3 layer: fused into the LDS-halo kernel's epilogue when that kernel applies
    (split-bf16 / bf16 precision, Cin % 32 == 0), otherwise the two calls.  -> label[B,H,W] u8, score[B,H,W] f32"""
    b, h, w, ldx = x.shape
    if upsample2x:
        h, w = 2 * h, 2 * w
    c = head_w.shape[0]
    fusable = (conv.nsplit and USE_HALO_KERNEL and conv.cout == 64 and conv.kh == 3 and conv.kw == 3 and conv.stride == 1
               and conv.pad == 1 and conv.dil == 1 and conv.cin % 32 == 0 and ldx == conv.cin and c <= 16
               and (upsample2x or tiles16_mostly_full(h, w)))
    if not fusable:
        return seg_head(conv(x, upsample2x=upsample2x), head_w, head_b, double_softmax)
    p = conv_params(conv, b, h, w, ldx, conv.cout, ups=upsample2x)
    label = torch.empty(b, h, w, dtype=torch.uint8, device=x.device)
    score = torch.empty(b, h, w, dtype=torch.float32, device=x.device)
    hlabel = halo_label(conv.nsplit, conv.dil, conv.cout, upsample2x, head=True)
    e0 = _prof_begin(hlabel)
    _lib.call.ape_conv3x3_halo_seghead_bf16(_lib.dptr(x, torch.float32), _lib.dptr(conv.wp), _lib.dptr(conv.bias), ctypes.byref(p),
                                            conv.nsplit, _lib.dptr(head_w, torch.float32), _lib.dptr(head_b), c, _lib.dptr(label),
                                            _lib.dptr(score), int(bool(double_softmax)), _st())
    if e0 is not None:
        hin, win = (h // 2, w // 2) if upsample2x else (h, w)
        # the 64-channel activation is never written: out = label (1 B) + score (4 B) per pixel
        _prof_end(e0, hlabel, conv_shape(conv, b, h, w, upsample2x) + " +head",
                  2.0 * b * h * w * conv.cout * 9 * conv.cin_real,
                  4.0 * (b * hin * win * conv.cin_real + conv.cout * 9 * conv.cin_real) + 5.0 * b * h * w)
    return label, score



# ---- smp Unet decoder (csrc/unet.hip) -------------------------------------------------------------------------------------------
def bn_fold(weight, gamma, beta, mean, var, eps=1e-5):
    """conv (no bias) followed by eval-mode BatchNorm2d  ->  (w', b') of one conv with bias: w' = w * g / sqrt(var + eps),
    b' = beta - mean * g / sqrt(var + eps), formed in fp64 on the host.  Returns fp64 CPU tensors (the caller casts)."""
    s = gamma.detach().double().cpu() / torch.sqrt(var.detach().double().cpu() + eps)
    w = weight.detach().double().cpu() * s.view(-1, *([1] * (weight.dim() - 1)))
    b = beta.detach().double().cpu() - mean.detach().double().cpu() * s
    return w, b


def unet_conv3x3_supported(c1, c2, cout, ups):
    return bool(_lib.lib().ape_unet_conv3x3_supported(int(c1), int(c2), int(cout), int(bool(ups))))


def _unet_operands(conv, a, b, ups):
    """(B, H, W, C1, C2, ldb) of a decoder conv over cat([nearest_up2(a) | a, b]); checks the channel split against the layer"""
    if conv.kh != 3 or conv.kw != 3 or conv.stride != 1 or conv.pad != 1 or conv.dil != 1 or not conv.nsplit:
        raise ValueError("the Unet decoder kernel takes 3x3 / stride 1 / pad 1 layers in the bf16 precisions")
    bb, ha, wa, lda = a.shape
    h, w = (2 * ha, 2 * wa) if ups else (ha, wa)
    c2 = 0 if b is None else b.shape[3]
    c1 = conv.cin_real - c2
    if c1 != lda:          # (a wider `a` would be read in part: the kernel takes channels 0..C1-1 of it)
        raise ValueError("input channels %d + %d do not match the layer's %d" % (lda, c2, conv.cin_real))
    if b is not None and tuple(b.shape[:3]) != (bb, h, w):
        raise ValueError("skip %s does not match the output %s" % (tuple(b.shape[:3]), (bb, h, w)))
    return bb, h, w, c1, c2, (0 if b is None else b.shape[3])


def unet_conv3x3(conv, a, b=None, ups=True, out=None, yoff=0):
    """relu(conv(cat([nearest_up2(a), b])) + bias) (ups=False: a at full resolution) -> out[B,H,W,ldy] channels yoff..yoff+Cout;
    conv: an engine.Conv (3x3 p1, the BN folded into weight and bias, precision bf16x3 | bf16) whose input channels are [a's | b's]"""
    bb, h, w, c1, c2, ldb = _unet_operands(conv, a, b, ups)
    if conv.act != ACT_RELU:          # (the kernel's epilogue is bias + ReLU: another activation would be dropped without a word)
        raise ValueError("the Unet decoder kernel's epilogue is ReLU; the layer's activation is %d" % conv.act)
    if not unet_conv3x3_supported(c1, c2, conv.cout, ups):
        raise ValueError("no Unet decoder kernel for C1 %d, C2 %d, Cout %d" % (c1, c2, conv.cout))
    if out is None:
        out = torch.empty(bb, h, w, conv.cout, dtype=torch.float32, device=a.device)
    if tuple(out.shape[:3]) != (bb, h, w):
        raise ValueError("output buffer %s does not match %s" % (tuple(out.shape), (bb, h, w)))
    nc = 4 if conv.cout >= 64 else 2 if conv.cout in (32, 48) else 1
    label = "unet_conv3x3_kernel<%d,%s,%d,%d,false>" % (conv.nsplit, "true" if ups else "false", nc, 4 if nc == 4 else 8)
    e0 = _prof_begin(label)
    _lib.call.ape_unet_conv3x3_bf16(_lib.dptr(a, torch.float32), a.shape[3], c1, _lib.dptr(b, torch.float32), ldb, c2,
                                    _lib.dptr(conv.wp), _lib.dptr(conv.bias), _lib.dptr(out, torch.float32), out.shape[3], yoff,
                                    bb, h, w, conv.cout, int(bool(ups)), conv.nsplit, _st())
    if e0 is not None:
        m = bb * h * w
        lo = (bb * a.shape[1] * a.shape[2] * c1 + m * c2)
        _prof_end(e0, label, "%dx%dx%d %d+%d->%d%s" % (bb, h, w, c1, c2, conv.cout, " ups" if ups else ""),
                  2.0 * m * conv.cout * 9 * conv.cin_real, 4.0 * (lo + conv.cout * 9 * conv.cin_real + m * conv.cout))
    return out


def unet_conv3x3_seghead(conv, a, b=None, ups=False, double_softmax=True):
    """the segmentation head: conv(cat([a (up-sampled when ups), b])) + bias (conv.cout = classes <= 16) -> softmax (+ softmax) -> arg-max,
    -> (label u8[B,H,W], score f32[B,H,W]); the logits are never stored"""
    bb, h, w, c1, c2, ldb = _unet_operands(conv, a, b, ups)
    if conv.cout > 16:
        raise ValueError("the fused head takes at most 16 classes")
    if conv.act != ACT_NONE:          # (the softmax runs on conv + bias)
        raise ValueError("the fused head applies no activation before the softmax; the layer's activation is %d" % conv.act)
    label = torch.empty(bb, h, w, dtype=torch.uint8, device=a.device)
    score = torch.empty(bb, h, w, dtype=torch.float32, device=a.device)
    klabel = "unet_conv3x3_kernel<%d,%s,1,8,true>" % (conv.nsplit, "true" if ups else "false")
    e0 = _prof_begin(klabel)
    _lib.call.ape_unet_conv3x3_seghead_bf16(_lib.dptr(a, torch.float32), a.shape[3], c1, _lib.dptr(b, torch.float32),
                                            ldb, c2, _lib.dptr(conv.wp), _lib.dptr(conv.bias), conv.cout, _lib.dptr(label), _lib.dptr(score),
                                            bb, h, w, int(bool(ups)), conv.nsplit, int(bool(double_softmax)), _st())
    if e0 is not None:
        m = bb * h * w
        _prof_end(e0, klabel, "%dx%dx%d %d+%d->%d%s +head" % (bb, h, w, c1, c2, conv.cout, " ups" if ups else ""),
                  2.0 * m * conv.cout * 9 * conv.cin_real,
                  4.0 * (bb * a.shape[1] * a.shape[2] * c1 + m * c2 + conv.cout * 9 * conv.cin_real) + 5.0 * m)
    return label, score


def nearest_up2(x, out=None, yoff=0, scale=2):
    """x[B,h,w,C] -> out[B,2h,2w,ldy] channels yoff..yoff+C = F.interpolate(scale_factor=2, mode='nearest') (scale=1: a copy).  The materialised
    form of the Unet decoder's first step: the up-sample and the skip are written into their channel windows of one concatenation buffer"""
    b, h, w, c = x.shape
    if out is None:
        out = torch.empty(b, scale * h, scale * w, c, dtype=torch.float32, device=x.device)
    if tuple(out.shape[:3]) != (b, scale * h, scale * w):
        raise ValueError("nearest_up2 output buffer mismatch")
    _lib.call.ape_nearest_upsample_nhwc_f32(_lib.dptr(x, torch.float32), _lib.dptr(out, torch.float32), b, h, w, c, scale, out.shape[3], yoff, _st())
    return out


USE_FUSED_STEM = os.environ.get("APE_USE_FUSED_STEM", "1") != "0"
USE_U8_STEM = os.environ.get("APE_USE_U8_STEM", "1") != "0"      # the stem reads the uint8 frames itself (ToTensor / Normalize fused into its patch load)


class U8Frames:
    """The network input `ToTensor + Normalize` of uint8 frames or crops (pipeline/utils.py:421-427, 556-560), NOT yet materialised:
    crop o = the hc x wc window of frame rects[o,0] at (rects[o,1], rects[o,2]) of rgb[F,H,W,3] u8.  `stem_pool` consumes it directly (the
    fp32 NHWC4 image -- 16 bytes per pixel -- is then never written); `materialise()` gives the tensor `preprocess_u8` would."""
    __slots__ = ("rgb", "rects", "hc", "wc", "div255", "_x4")

    def __init__(self, rgb, rects, hc, wc, div255):
        self.rgb, self.rects, self.hc, self.wc, self.div255, self._x4 = rgb, rects, int(hc), int(wc), bool(div255), None

    @property
    def shape(self):
        return (self.rects.shape[0], self.hc, self.wc, 4)

    @property
    def is_cuda(self):
        return self.rgb.is_cuda

    @property
    def device(self):
        return self.rgb.device

    def __getitem__(self, idx):          # batch slicing only
        return U8Frames(self.rgb, self.rects[idx].contiguous(), self.hc, self.wc, self.div255)

    def materialise(self):
        if self._x4 is None:
            self._x4 = preprocess_u8(self.rgb, self.rects, self.hc, self.wc, self.div255)
        return self._x4


def stem_pool(conv, x):
    """maxpool3x3s2(conv(x)) for the ResNet stem (7x7 / stride 2 / pad 3, 4 -> 64 channels, ReLU): one fused kernel on the bf16
    paths (the half-resolution activation is never stored), the two calls otherwise.  x: the normalised image [B,H,W,4], or `U8Frames`."""
    if isinstance(x, U8Frames):
        fus = (USE_U8_STEM and USE_FUSED_STEM and conv.nsplit and conv.cout == 64 and conv.cin == 4 and conv.kh == 7 and conv.kw == 7
               and conv.stride == 2 and conv.pad == 3 and conv.dil == 1 and conv.act == ACT_RELU)
        if not fus:
            return stem_pool(conv, x.materialise())
        n, h, w, _ = x.shape
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        y = torch.empty(n, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1, 64, dtype=torch.float32, device=x.device)
        _lib.call.ape_stem_conv_pool_u8(_lib.dptr(x.rgb, torch.uint8), x.rgb.shape[0], _lib.dptr(x.rects, torch.int32), _lib.dptr(conv.w, torch.float32),
                                        _lib.dptr(conv.bias), _lib.dptr(y), n, x.rgb.shape[1], x.rgb.shape[2], h, w, int(x.div255), conv.nsplit, _st())
        return y
    b, h, w, ldx = x.shape
    fusable = (USE_FUSED_STEM and conv.nsplit and conv.cout == 64 and conv.cin == 4 and ldx == 4 and conv.kh == 7 and conv.kw == 7
               and conv.stride == 2 and conv.pad == 3 and conv.dil == 1 and conv.act == ACT_RELU)
    if not fusable:
        return maxpool3x3s2(conv(x))
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty(b, (ho - 1) // 2 + 1, (wo - 1) // 2 + 1, 64, dtype=torch.float32, device=x.device)
    _lib.call.ape_stem_conv_pool_bf16(_lib.dptr(x, torch.float32), _lib.dptr(conv.w, torch.float32), _lib.dptr(conv.bias),
                                      _lib.dptr(y), b, h, w, conv.nsplit, _st())
    return y


def maxpool3x3s2(x):
    b, h, w, c = x.shape
    y = torch.empty(b, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c, dtype=torch.float32, device=x.device)
    _lib.call.ape_maxpool3x3s2_nhwc_f32(_lib.dptr(x, torch.float32), _lib.dptr(y), b, h, w, c, _st())
    return y


# ---- SegNet glue (csrc/segnet.hip) ----------------------------------------------------------------------------------------------------
def maxpool2x2_idx(x):
    """F.max_pool2d(x, 2, 2, return_indices=True) on x[B,H,W,C]: -> y[B,H//2,W//2,C] f32, code[B,H//2,W//2,C] u8 = 2 * dy + dx of each
    window's winner (torch's CPU tie / NaN rule)"""
    b, h, w, c = x.shape
    y = torch.empty(b, h // 2, w // 2, c, dtype=torch.float32, device=x.device)
    code = torch.empty(b, h // 2, w // 2, c, dtype=torch.uint8, device=x.device)
    _lib.call.ape_maxpool2x2_idx_nhwc_f32(_lib.dptr(x, torch.float32), _lib.dptr(y), _lib.dptr(code), b, h, w, c, _st())
    return y, code


def max_unpool2x2(y, code, h, w):
    """F.max_unpool2d(y, idx, 2, 2, output_size=(h, w)) for the codes of `maxpool2x2_idx`: y[B,h//2,w//2,C] -> x[B,h,w,C], every element
    written (zeros off the coded positions and in an odd last row / column)"""
    b, ho, wo, c = y.shape
    if (ho, wo) != (h // 2, w // 2) or tuple(code.shape) != tuple(y.shape):
        raise ValueError("max_unpool2x2: y %s / code %s do not pool a %d x %d map" % (tuple(y.shape), tuple(code.shape), h, w))
    x = torch.empty(b, h, w, c, dtype=torch.float32, device=y.device)
    _lib.call.ape_max_unpool2x2_nhwc_f32(_lib.dptr(y, torch.float32), _lib.dptr(code, torch.uint8), _lib.dptr(x), b, h, w, c, _st())
    return x


def gather2x2(x, code):
    """y[B,H//2,W//2,C] = the element of each 2 x 2 window of x[B,H,W,C] that `code` names (the unpool's backward)"""
    b, h, w, c = x.shape
    if tuple(code.shape) != (b, h // 2, w // 2, c):
        raise ValueError("gather2x2: code %s does not pool %s" % (tuple(code.shape), tuple(x.shape)))
    y = torch.empty(b, h // 2, w // 2, c, dtype=torch.float32, device=x.device)
    _lib.call.ape_gather2x2_nhwc_f32(_lib.dptr(x, torch.float32), _lib.dptr(code, torch.uint8), _lib.dptr(y), b, h, w, c, _st())
    return y


def cross_entropy(logits, labels, n_classes=None, g=1.0, want_grad=False):
    """nn.CrossEntropyLoss() over the pixels of logits[..., ld] (classes = the first n_classes channels) and labels u8 of the leading shape.
    -> out f64[2] on the device (the mean over the valid pixels; the number of labels >= n_classes, which the caller must treat as an
    error when it reads the loss) and, with want_grad, dlogits = g * (softmax - onehot) / n_valid in the layout of `logits`."""
    ld = logits.shape[-1]
    c = ld if n_classes is None else int(n_classes)
    p = logits.numel() // ld
    if labels.numel() != p:
        raise ValueError("cross_entropy: %d labels for %d pixels" % (labels.numel(), p))
    out = torch.empty(2, dtype=torch.float64, device=logits.device)
    dlogits = torch.empty_like(logits) if want_grad else None
    nbytes = _lib.lib().ape_cross_entropy_workspace_bytes(p)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=logits.device)
    _lib.call.ape_cross_entropy_f32(_lib.dptr(logits, torch.float32), ld, c, _lib.dptr(labels, torch.uint8), p, float(g), _lib.dptr(out),
                                    _lib.dptr(dlogits), _lib.dptr(ws), nbytes, _st())
    return out, dlogits


def adaptive_avgpool(x, s):
    b, h, w, c = x.shape
    y = torch.empty(b, s, s, c, dtype=torch.float32, device=x.device)
    _lib.call.ape_adaptive_avgpool_nhwc_f32(_lib.dptr(x, torch.float32), _lib.dptr(y), b, h, w, c, s, _st())
    return y


POOL_ATOM_ROWS = False   # adaptive_avgpool_multi's first pass with one workgroup per atom ROW (the former kernel; A/B, same bits)


def adaptive_avgpool_multi(x, sizes, channels=None):
    """{s: AdaptiveAvgPool2d((s, s))(x[..., :channels])} for several sizes in one pass over x[B,H,W,C]; per-size launches when the bin edges
    of the sizes cut an axis into more than 12 atoms.  `channels` (default: all) pools the leading channels only and gives [B,s,s,channels]."""
    fmt = FMT_S32 if isinstance(x, S32) else FMT_F32
    xt = x.t if fmt == FMT_S32 else x
    b, h, w, ld = xt.shape
    c = ld if channels is None else int(channels)
    sizes = list(sizes)
    ys = [torch.empty(b, s, s, c, dtype=torch.float32, device=xt.device) for s in sizes]
    ws = _workspace(_lib.lib().ape_adaptive_avgpool_multi_workspace_bytes(b, c), xt.device)
    ptrs = (ctypes.c_void_p * len(sizes))(*[y.data_ptr() for y in ys])
    szs = (ctypes.c_int * len(sizes))(*sizes)
    try:
        _lib.call.ape_adaptive_avgpool_multi_nhwc_ld(_lib.dptr(xt, torch.float32), fmt | (0x100 if POOL_ATOM_ROWS else 0), ptrs, szs, len(sizes), b, h, w, c, ld, _lib.dptr(ws),
                                                     ws.numel() * ws.element_size(), _st())
    except _lib.ApeError as e:
        if e.code != -1:
            raise
        xf = x.to_f32() if fmt == FMT_S32 else x      # APE_EINVAL: too many atoms for this geometry
        xf = xf if c == ld else xf[..., :c].contiguous()
        return {s: adaptive_avgpool(xf, s) for s in sizes}
    return dict(zip(sizes, ys))


def conv1x1_multi(convs, xs):
    """[conv(x) for conv, x in zip(convs, xs)] for up to four independent 1x1 / stride-1 convolutions of fp32 maps in ONE launch
    (ape_conv_gemm_bf16_multi): the PSP module's stage convolutions (pspnet.py:15-18, 22), problems of 1 .. 18 tiles each whose separate
    launches ran one after the other with the chip idle.  Bit for bit what the separate calls give; they are what runs where the
    launch does not apply (more than four problems, other precisions, geometries the GEMM kernel does not take)."""
    convs, xs = list(convs), list(xs)
    n = len(convs)
    ok = (1 <= n <= 4 and USE_CONV_MULTI and USE_GEMM_KERNEL and not (GEMM_VARIANT & 15) and
          all(c.nsplit and c.nsplit == convs[0].nsplit and c.kh == 1 and c.kw == 1 and c.stride == 1 and c.pad == 0 and not isinstance(x, S32)
              and x.shape[3] == c.cin and x.is_contiguous() for c, x in zip(convs, xs)))
    if ok:
        outs = [torch.empty(x.shape[0], x.shape[1], x.shape[2], c.cout, dtype=torch.float32, device=x.device) for c, x in zip(convs, xs)]
        ps = (ConvParams * n)(*[conv_params(c, x.shape[0], x.shape[1], x.shape[2], x.shape[3], c.cout) for c, x in zip(convs, xs)])
        ok = all(_lib.lib().ape_conv_gemm_supported(ctypes.byref(ps[i])) for i in range(n))
    if not ok:
        return [c(x) for c, x in zip(convs, xs)]
    arr = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    _lib.call.ape_conv_gemm_bf16_multi(n, arr(xs), arr([c.wp for c in convs]), arr([c.bias for c in convs]), arr(outs), ps, convs[0].nsplit, _st())
    return outs


def bilinear(x, ho, wo, align_corners, out=None, yoff=0, accumulate=False):
    b, h, w, c = x.shape
    if out is None:
        out = torch.empty(b, ho, wo, c, dtype=torch.float32, device=x.device)
    if tuple(out.shape[:3]) != (b, ho, wo):
        raise ValueError("bilinear output buffer mismatch")
    _lib.call.ape_bilinear_nhwc_f32(_lib.dptr(x, torch.float32), _lib.dptr(out, torch.float32), b, h, w, c, c, ho, wo,
                                    out.shape[3], yoff, int(bool(align_corners)), int(bool(accumulate)), _st())
    return out


def psp_prior_sum(zs, h, w):
    """zs = [z1[B,1,1,C], z2[B,2,2,C], z3[B,3,3,C], z6[B,6,6,C]] -> sum of their bilinear (align_corners=False) resizes [B,h,w,C]"""
    b, c = zs[0].shape[0], zs[0].shape[3]
    out = torch.empty(b, h, w, c, dtype=torch.float32, device=zs[0].device)
    _lib.call.ape_psp_prior_sum_f32(*[_lib.dptr(z, torch.float32) for z in zs], _lib.dptr(out), b, h, w, c, _st())
    return out


USE_PSP_FOLD = os.environ.get("APE_USE_PSP_FOLD", "1") != "0"    # the PSP prior sum as 64 more K-columns of the bottleneck's contraction (S32 graph)
PSP_FOLD_K = 64


def psp_bottleneck_folded(conv, x576, zs, out_fmt=FMT_S32):
    """relu(W_f . f + sum_s upsample(z_s) + bias) (pspnet.py:22-24 with the prior sum of :12-17 folded in) as ONE contraction over
    K = Cin + 64: `x576` is the S32 map f[B,h,w,Cin + 64] whose last 64 channels this call fills with the pixels' bilinear coefficients,
    `zs` = [z1[B,1,1,C], z2[B,2,2,C], z3[B,3,3,C], z6[B,6,6,C]] fp32 (the merged prior convs of the pooled maps), `conv` the bottleneck's
    feats columns (Cin -> C, bias, ReLU).  No [B,h,w,C] prior-sum tensor is written or read (include/ape_hip.h ape_psp_fold_operands)."""
    xt = x576.t
    b, h, w, ld = xt.shape
    if conv.nsplit != 3 or (conv.kh, conv.kw, conv.stride, conv.pad) != (1, 1, 1, 0) or ld != conv.cin + PSP_FOLD_K or [tuple(z.shape) for z in zs] != [(b, s, s, conv.cout) for s in (1, 2, 3, 6)]:
        raise ValueError("psp_bottleneck_folded: a split-bf16 1x1 layer, an S32 map of Cin + 64 channels and the four prior maps [B,s,s,Cout]")
    groups = conv.cin // 32 + 2
    wimg = torch.empty(b, conv.cout, groups * 64, dtype=torch.bfloat16, device=xt.device)
    _lib.call.ape_psp_fold_operands(_lib.dptr(conv.s32k()), *[_lib.dptr(z, torch.float32) for z in zs], _lib.dptr(wimg),
                                    _lib.dptr(xt, torch.float32), b, h, w, ld, conv.cin, conv.cout, _st())
    out = torch.empty(b, h, w, conv.cout, dtype=torch.float32, device=xt.device)
    p = conv_params(conv, b, h, w, ld, conv.cout)
    p.Cin = ld                  # the contraction runs over K = Cin + 64
    label = gemm_s32_label(conv.cout)
    e0 = _prof_begin(label)
    _lib.call.ape_conv_gemm_s32_per_image(_lib.dptr(xt, torch.float32), _lib.dptr(wimg), conv.cout * groups * 128, _lib.dptr(conv.bias),
                                          _lib.dptr(out), out_fmt, ctypes.byref(p), _st())
    if e0 is not None:      # algorithmic: the layer's own contraction (K = Cin) + the prior sum's 50 coefficient columns; bytes: f in, out, per-frame weights
        _prof_end(e0, label, "%dx%dx%d %d+%d->%d k1 s1 d1 psp-fold" % (b, h, w, conv.cin, PSP_FOLD_K, conv.cout), 2.0 * b * h * w * conv.cout * ld,
                  4.0 * (b * h * w * ld + b * conv.cout * ld + b * h * w * conv.cout))
    return S32(out) if out_fmt == FMT_S32 else out


USE_UPFUSE = os.environ.get("APE_USE_UPFUSE", "1") != "0"    # 64-channel PSPUpsample layers on S32 inputs as ONE kernel (upconv_fused.hip)


class UpConv:
    """PSPUpsample (pspnet.py:27-37) as  1x1 conv at low resolution (9*Cout channels) + ape_upconv3x3_gather_f32 -- or, for a 64 -> 64
    layer on an S32 input (up_3), as the ONE kernel of upconv_fused.hip that keeps the 9*Cout-channel tensor on the chip (bit-identical
    to the two calls).  fma: both interpolation steps as chained fused multiply-adds instead of separately rounded products."""

    def __init__(self, weight, bias, alpha, device="cuda", precision="f32", fma=False, splitk=False):
        cout, cin, kh, kw = weight.shape
        assert (kh, kw) == (3, 3)
        w9 = weight.detach().permute(2, 3, 0, 1).reshape(9 * cout, cin)            # row = (ky*3+kx)*Cout + co
        self.mix = Conv(w9, None, device=device, precision=precision, splitk=splitk)
        self.bias = bias.detach().to(device=device, dtype=torch.float32).contiguous()
        self.alpha, self.cout, self.cin, self.fma = float(alpha), cout, cin, bool(fma)

    def fusable(self, x):
        """the one-kernel form applies: split-bf16 operands, an S32 input, and a geometry upconv_fused.hip serves"""
        return bool(USE_UPFUSE and isinstance(x, S32) and self.mix.nsplit == 3 and x.shape[3] == self.cin
                    and _lib.lib().ape_upconv3x3_fused_supported(x.shape[1], x.shape[2], self.cin, self.cout))

    def _gather(self, z, out_fmt):
        b, h, w, _ = z.shape
        out = torch.empty(b, 2 * h, 2 * w, self.cout, dtype=torch.float32, device=z.device)
        strip = self.cout % 64 == 0 and _lib.lib().ape_upconv3x3_gather_strip_rows(-1) > 0      # the library's own routing rule
        glabel = "upconv_gather_%skernel<%s,%s>" % ("strip_" if strip else "", "true" if out_fmt == FMT_S32 else "false", "true" if self.fma else "false")
        e0 = _prof_begin(glabel)
        _lib.call.ape_upconv3x3_gather_ex(_lib.dptr(z, torch.float32), _lib.dptr(self.bias), _lib.dptr(out), out_fmt, b, h, w,
                                          self.cout, ACT_PRELU, self.alpha, int(self.fma), _st())
        if e0 is not None:      # HBM-bound: z read once (9 * Cout channels at low resolution) + the output written once
            _prof_end(e0, glabel, "%dx%dx%d C%d" % (b, 2 * h, 2 * w, self.cout), 0.0, 4.0 * (b * h * w * 9 * self.cout + b * 4 * h * w * self.cout))
        return S32(out) if out_fmt == FMT_S32 else out

    def __call__(self, x, out_fmt=FMT_F32, fused=None):
        """x fp32 or S32 -> [B,2h,2w,Cout] in `out_fmt` (two-call form: the 9*Cout-channel intermediate z stays fp32, the gather is
        VALU work).  fused: None = the one-kernel form whenever it applies, False = never, True = required."""
        if fused is None:
            fused = self.fusable(x)
        if not fused:
            return self._gather(self.mix(x), out_fmt)
        if not self.fusable(x):
            raise ValueError("no fused PSPUpsample kernel for this layer / input (needs split-bf16 operands, an S32 input, 64 -> 64 channels)")
        b, h, w, _ = x.shape
        out = torch.empty(b, 2 * h, 2 * w, self.cout, dtype=torch.float32, device=x.device)
        label = "upconv_fused_kernel<%d,false,%s>" % (self.cin // 32, "true" if self.fma else "false")
        e0 = _prof_begin(label)
        _lib.call.ape_upconv3x3_fused_s32(_lib.dptr(x.t, torch.float32), _lib.dptr(self.mix.s32k()), _lib.dptr(self.bias), _lib.dptr(out),
                                          out_fmt, b, h, w, self.cin, ACT_PRELU, self.alpha, int(self.fma), _st())
        if e0 is not None:
            _prof_end(e0, label, "%dx%dx%d %d->%d up (executed flop; direct form x4)" % (b, 2 * h, 2 * w, self.cin, self.cout), *self._fused_cost(b, h, w, 4.0 * self.cout))
        return S32(out) if out_fmt == FMT_S32 else out

    def _fused_cost(self, b, h, w, out_bytes_per_pixel):
        """(flop, algorithmic bytes) of the one-kernel form.  The flop are the ones the kernel EXECUTES on the matrix cores -- the channel
        mixing at LOW resolution, 2 * B * h * w * (9 * Cout) * Cin -- a quarter of the reference's convolution at high resolution
        (pspnet.py:30-33: 2 * B * 4 h w * Cout * 9 * Cin): pricing the layer's direct form against the matrix peak would overstate the
        matrix-core throughput four times over (the kernel is bound by vector-instruction issue, not by the matrix pipe).  Bytes: the input
        read + the output written once."""
        return (2.0 * b * h * w * 9 * self.cout * self.cin,
                4.0 * (b * h * w * self.cin + 9 * self.cout * self.cin) + out_bytes_per_pixel * b * 4 * h * w)

    def seg_head(self, x, head_w, head_b, double_softmax=True, fused=None):
        """`seg_head(self(x))`: label[B,2h,2w] u8, score f32 -- in the one-kernel form the 64-channel activation is never stored"""
        if fused is None:
            fused = self.fusable(x) and head_w.shape[0] <= 16 and self.cout == 64
        if not fused:
            return seg_head(self(x, fused=False), head_w, head_b, double_softmax)
        b, h, w, _ = x.shape
        c = head_w.shape[0]
        label = torch.empty(b, 2 * h, 2 * w, dtype=torch.uint8, device=x.device)
        score = torch.empty(b, 2 * h, 2 * w, dtype=torch.float32, device=x.device)
        klabel = "upconv_fused_kernel<%d,true,%s>" % (self.cin // 32, "true" if self.fma else "false")
        e0 = _prof_begin(klabel)
        _lib.call.ape_upconv3x3_fused_seghead_s32(_lib.dptr(x.t, torch.float32), _lib.dptr(self.mix.s32k()), _lib.dptr(self.bias), b, h, w,
                                                  self.cin, ACT_PRELU, self.alpha, int(self.fma), _lib.dptr(head_w, torch.float32),
                                                  _lib.dptr(head_b), c, _lib.dptr(label), _lib.dptr(score), int(bool(double_softmax)), _st())
        if e0 is not None:
            _prof_end(e0, klabel, "%dx%dx%d %d->%d up +head (executed flop; direct form x4)" % (b, 2 * h, 2 * w, self.cin, self.cout), *self._fused_cost(b, h, w, 5.0))
        return label, score


def gather_rows(x, index):
    """x[B,R,C], index[B,n] i64 -> [B,n,C]"""
    b, r, c = x.shape
    n = index.shape[1]
    y = torch.empty(b, n, c, dtype=torch.float32, device=x.device)
    _lib.call.ape_gather_rows_f32(_lib.dptr(x, torch.float32), _lib.dptr(index, torch.int64), _lib.dptr(y), b, r, n, c, _st())
    return y


def ups_patch_gather(x, index):
    """x[B,h,w,C], index[B,n] i64 (pixel of the x2 up-sampled image) -> [B*n, 1, 1, 9*C] patches of the up-sampled image"""
    b, h, w, c = x.shape
    n = index.shape[1]
    out = torch.empty(b * n, 1, 1, 9 * c, dtype=torch.float32, device=x.device)
    _lib.call.ape_ups_patch_gather_f32(_lib.dptr(x, torch.float32), _lib.dptr(index, torch.int64), _lib.dptr(out), b, h, w, c, n, _st())
    return out


def conv3x3_as_matrix(conv):
    """A 3x3 Conv viewed as the 1x1 contraction over its 9*Cin patch columns: a layer of its own (plan cache, lazily packed S32K / MX6
    operands) over the 3x3 layer's weight storage (already [Cout][KH][KW][Cin]), bf16 planes and bias."""
    assert conv.kh == 3 and conv.kw == 3 and conv.cin == conv.cin_real
    m = Conv.from_packed(conv.w.view(conv.cout, 1, 1, 9 * conv.cin), conv.wp if conv.nsplit else None, 9 * conv.cin, act=conv.act, alpha=conv.alpha,
                         precision=conv.precision, splitk=conv.splitk)
    m.bias = conv.bias
    return m


def log_softmax_rows(x):
    c = x.shape[-1]
    rows = x.numel() // c
    y = torch.empty_like(x)
    _lib.call.ape_log_softmax_rows_f32(_lib.dptr(x, torch.float32), _lib.dptr(y), rows, c, _st())
    return y


def mean_rows(x):
    """x[B,n,C] -> [B,C]"""
    b, n, c = x.shape
    y = torch.empty(b, c, dtype=torch.float32, device=x.device)
    _lib.call.ape_mean_rows_f32(_lib.dptr(x, torch.float32), _lib.dptr(y), b, n, c, _st())
    return y


def pad3to4(x):
    """x[...,3] -> [...,4]"""
    rows = x.numel() // 3
    y = torch.empty(*x.shape[:-1], 4, dtype=torch.float32, device=x.device)
    _lib.call.ape_pad3to4_f32(_lib.dptr(x, torch.float32), _lib.dptr(y), rows, _st())
    return y


def head_select(h, off_r, off_t, off_c, wr, br, wt, bt, wc, bc, obj, b, n, k):
    """h[B*n, ldh] -> out[B,n,8]"""
    out = torch.empty(b, n, 8, dtype=torch.float32, device=h.device)
    _lib.call.ape_head_select_f32(_lib.dptr(h, torch.float32), h.shape[-1], off_r, off_t, off_c, _lib.dptr(wr),
                                  _lib.dptr(br), _lib.dptr(wt), _lib.dptr(bt), _lib.dptr(wc), _lib.dptr(bc),
                                  _lib.dptr(obj, torch.int64), _lib.dptr(out), b, n, k, _st())
    return out


def pose_select(heads, points4, want_new_points=True):
    """heads[B,n,8], points4[B,n,4] -> pose[B,7] f64, which[B] i32, new_points4[B,n,4] | None"""
    b, n, _ = heads.shape
    pose = torch.empty(b, 7, dtype=torch.float64, device=heads.device)
    which = torch.empty(b, dtype=torch.int32, device=heads.device)
    newp = torch.empty(b, n, 4, dtype=torch.float32, device=heads.device) if want_new_points else None
    _lib.call.ape_pose_select_f32(_lib.dptr(heads, torch.float32), _lib.dptr(points4, torch.float32), _lib.dptr(pose),
                                  _lib.dptr(which), _lib.dptr(newp), b, n, _st())
    return pose, which, newp


def head_conf_argmax(h3c, off_c, wc, bc, obj, b, n, k, pf=None):
    """h3c[B*n, ldh] (the confidence head's input at off_c), pf[B*n, ld] | None -> which[B] i32 (first maximum of sigmoid(c) over the crop's
    rows), conf[B], pf_row[B, ld] | None (pf at the selected rows)"""
    which = torch.empty(b, dtype=torch.int32, device=h3c.device)
    conf = torch.empty(b, dtype=torch.float32, device=h3c.device)
    row = None if pf is None else torch.empty(b, pf.shape[-1], dtype=torch.float32, device=h3c.device)
    _lib.call.ape_head_conf_argmax_f32(_lib.dptr(h3c, torch.float32), h3c.shape[-1], off_c, _lib.dptr(wc), _lib.dptr(bc),
                                       _lib.dptr(obj, torch.int64), _lib.dptr(which), _lib.dptr(conf), _lib.dptr(pf, torch.float32),
                                       0 if pf is None else pf.shape[-1], _lib.dptr(row), b, n, k, _st())
    return which, conf, row


def pose_from_row(h3rt, off_r, off_t, wr, br, wt, bt, obj, which, points4, k, want_new_points=True):
    """h3rt[B, ldh] (the r / t heads' inputs of each crop's selected row), which[B] i32, points4[B,n,4]
    -> pose[B,7] f64, new_points4[B,n,4] | None: what pose_select gives from the full heads"""
    b, n, _ = points4.shape
    pose = torch.empty(b, 7, dtype=torch.float64, device=h3rt.device)
    newp = torch.empty(b, n, 4, dtype=torch.float32, device=h3rt.device) if want_new_points else None
    _lib.call.ape_pose_from_row_f32(_lib.dptr(h3rt, torch.float32), h3rt.shape[-1], off_r, off_t, _lib.dptr(wr), _lib.dptr(br),
                                    _lib.dptr(wt), _lib.dptr(bt), _lib.dptr(obj, torch.int64), _lib.dptr(which, torch.int32),
                                    _lib.dptr(points4, torch.float32), _lib.dptr(pose), _lib.dptr(newp), b, n, k, _st())
    return pose, newp


def pose_compose(pose, ref_r, ref_t):
    """in-place: pose[B,7] f64 <- pose o (ref_r[B,>=4], ref_t[B,>=3]) ; ref_* are (possibly strided) row views"""
    b = pose.shape[0]
    _lib.call.ape_pose_compose_f64(_lib.dptr(pose, torch.float64), ctypes.c_void_p(ref_r.data_ptr()), ref_r.stride(0),
                                   ctypes.c_void_p(ref_t.data_ptr()), ref_t.stride(0), b, _st())
    return pose


def pose_recentre(points4, pose):
    b, n, _ = points4.shape
    out = torch.empty_like(points4)
    _lib.call.ape_pose_recentre_f32(_lib.dptr(points4, torch.float32), _lib.dptr(pose, torch.float64), _lib.dptr(out), b, n, _st())
    return out


# ---- segmentation post-processing / selection --------------------------------------------------------------------
def preprocess_u8(rgb, rects, hc, wc, div255):
    """rgb[B,H,W,3] u8, rects[n,3] i32 (frame,row0,col0) -> [n,hc,wc,4] f32"""
    b, h, w, _ = rgb.shape
    n = rects.shape[0]
    out = torch.empty(n, hc, wc, 4, dtype=torch.float32, device=rgb.device)
    _lib.call.ape_preprocess_u8_nhwc4(_lib.dptr(rgb, torch.uint8), _lib.dptr(rects, torch.int32), _lib.dptr(out), n, h, w,
                                      hc, wc, int(bool(div255)), _st())
    return out


def seg_argmax(logits, n_classes, double_softmax=True):
    """logits[B,H,W,ld] -> label[B,H,W] u8, score[B,H,W] f32"""
    b, h, w, ld = logits.shape
    label = torch.empty(b, h, w, dtype=torch.uint8, device=logits.device)
    score = torch.empty(b, h, w, dtype=torch.float32, device=logits.device)
    _lib.call.ape_seg_argmax_f32(_lib.dptr(logits, torch.float32), ld, n_classes, _lib.dptr(label), _lib.dptr(score),
                                 b * h * w, int(bool(double_softmax)), _st())
    return label, score


def seg_head(feat, w, bias, double_softmax=True):
    """feat[B,H,W,64], w[C,64], bias[C] -> label[B,H,W] u8, score[B,H,W] f32 (fused final conv + softmax^2 + argmax)"""
    b, h, wd, c = feat.shape
    if c != 64:
        raise ValueError("seg_head expects the 64-channel up_3 activation")
    label = torch.empty(b, h, wd, dtype=torch.uint8, device=feat.device)
    score = torch.empty(b, h, wd, dtype=torch.float32, device=feat.device)
    _lib.call.ape_seg_head_f32(_lib.dptr(feat, torch.float32), _lib.dptr(w, torch.float32), _lib.dptr(bias), w.shape[0],
                               _lib.dptr(label), _lib.dptr(score), b * h * wd, int(bool(double_softmax)), _st())
    return label, score


_ws_cache = {}
CAPTURING = False       # set while a HIP graph is being captured (pipeline.FramePipeline pose graphs): workspaces then come from the graph's own pool


def _workspace(nbytes, device):
    if CAPTURING:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    key = (str(device), "seg", torch.cuda.current_stream().cuda_stream)   # one workspace per stream: sub-batches may overlap
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


SEG_SCORE_MEAN, SEG_SCORE_SUM = 0, 1


def seg_components(label, score, n_classes, min_pixels=100, score_mode=SEG_SCORE_MEAN):
    """-> objmap[B,H,W] u8, det[B,C,5] i32 (valid,rmin,rmax,cmin,cmax); score_mode: best component by mean (full_prediction)
    or summed (do_cca) probability"""
    b, h, w = label.shape
    objmap = torch.empty_like(label)
    det = torch.empty(b, n_classes, 5, dtype=torch.int32, device=label.device)
    nbytes = _lib.lib().ape_seg_components_workspace_bytes(b, h, w, n_classes)
    ws = _workspace(nbytes, label.device)
    _lib.call.ape_seg_components_scored(_lib.dptr(label, torch.uint8), _lib.dptr(score, torch.float32), _lib.dptr(objmap),
                                        _lib.dptr(det), b, h, w, n_classes, min_pixels, score_mode, _lib.dptr(ws),
                                        ws.numel(), _st())
    return objmap, det


def bgsub_features(f_rgb, b_rgb, f_depth, b_depth, gate, mean, std, want_diff=False):
    """f_rgb/b_rgb[B,H,W,3] u8, f_depth/b_depth[B,H,W] u16, gate[B,2] f64 (min,max) -> x8[B,H,W,8] f32 (7 normalised difference
    channels + a zero), optionally the uint8 channels diff[B,H,W,7]."""
    import ctypes
    b, h, w, _ = f_rgb.shape
    out = torch.empty(b, h, w, 8, dtype=torch.float32, device=f_rgb.device)
    diff = torch.empty(b, h, w, 7, dtype=torch.uint8, device=f_rgb.device) if want_diff else None
    m = (ctypes.c_float * 7)(*[float(v) for v in mean])
    s = (ctypes.c_float * 7)(*[float(v) for v in std])
    _lib.call.ape_bgsub_features_f32(_lib.dptr(f_rgb, torch.uint8), _lib.dptr(b_rgb, torch.uint8),
                                     _lib.dptr(f_depth, torch.uint16), _lib.dptr(b_depth, torch.uint16),
                                     _lib.dptr(gate, torch.float64), ctypes.cast(m, ctypes.c_void_p),
                                     ctypes.cast(s, ctypes.c_void_p), _lib.dptr(out),
                                     _lib.dptr(diff) if want_diff else None, b, h, w, _st())
    return (out, diff) if want_diff else out


def choose_points(objmap, depth, objects, n_points, seed=0):
    """objects[n,6] i32 (frame,cls,rmin,rmax,cmin,cmax) -> choose[n,N] i64, n_cand[n] i32.  `seed`: an int, or a device tensor (int32[1]) that the
    kernel reads when it runs -- the form a captured launch needs to follow a seed that changes between replays"""
    b, h, w = objmap.shape
    n = objects.shape[0]
    choose = torch.zeros(n, n_points, dtype=torch.int64, device=objmap.device)
    n_cand = torch.zeros(n, dtype=torch.int32, device=objmap.device)
    stride = h * w
    cand = torch.empty(n, stride, dtype=torch.int32, device=objmap.device)
    if isinstance(seed, torch.Tensor):
        _lib.call.ape_choose_points_dseed(_lib.dptr(objmap, torch.uint8), _lib.dptr(depth, torch.uint16), _lib.dptr(objects, torch.int32),
                                          n, h, w, n_points, _lib.dptr(seed, torch.int32), _lib.dptr(cand), stride, _lib.dptr(choose),
                                          _lib.dptr(n_cand), _st())
    else:
        _lib.call.ape_choose_points(_lib.dptr(objmap, torch.uint8), _lib.dptr(depth, torch.uint16), _lib.dptr(objects, torch.int32),
                                    n, h, w, n_points, seed & 0xFFFFFFFF, _lib.dptr(cand), stride, _lib.dptr(choose),
                                    _lib.dptr(n_cand), _st())
    return choose, n_cand


def backproject(depth, objects, choose, intr, depth_scale):
    b, h, w = depth.shape
    n, npts = choose.shape
    pts = torch.empty(n, npts, 4, dtype=torch.float32, device=depth.device)
    _lib.call.ape_backproject_f32(_lib.dptr(depth, torch.uint16), _lib.dptr(objects, torch.int32), _lib.dptr(choose, torch.int64),
                                  _lib.dptr(pts), n, h, w, npts, float(intr["fx"]), float(intr["fy"]), float(intr["ppx"]),
                                  float(intr["ppy"]), float(depth_scale), _st())
    return pts


ICP_ESTIMATIONS = ("point_to_point", "point_to_plane")


def icp_polish(points4, n_cand, obj_class, models, pose, max_correspondence_distance, criteria, min_fitness=0.0, estimation="point_to_point"):
    """Depth ICP polish of a batch of objects in ONE launch (csrc/icp_polish.hip): points4[n,N,4] f32 as `backproject` leaves
    them, n_cand[n] i32, obj_class[n] (row of `models` per object: an int32 device tensor, or a host sequence that is checked against the
    table and uploaded), models = pipeline.polish.ModelSet, pose[n,7] f64 (w,x,y,z,tx,ty,tz), criteria with relative_fitness /
    relative_rmse / max_iteration -> (pose_out[n,7] f64, stats[n,4] f64 = fitness, inlier rmse, correspondences, stop reason).
    estimation: "point_to_point", or "point_to_plane" on the normals of `models` (a set without normals is refused).
    Enqueues on the current stream, reads nothing back: safe inside a graph capture."""
    if estimation not in ICP_ESTIMATIONS:
        raise ValueError("icp_polish: estimation must be one of %s, not %r" % (", ".join(ICP_ESTIMATIONS), estimation))
    plane = estimation == "point_to_plane"
    if plane and getattr(models, "normals_table", None) is None:
        raise ValueError("icp_polish: point_to_plane needs a ModelSet with normals (normal_radius=... or normals=...)")
    n, npts = int(points4.shape[0]), int(points4.shape[1])
    if not torch.is_tensor(obj_class) or not obj_class.is_cuda:
        host = [int(c) for c in (obj_class.tolist() if torch.is_tensor(obj_class) else obj_class)]
        bad = [c for c in host if not 0 <= c < models.n_classes]
        if bad:
            raise ValueError("icp_polish: class %d is outside the model table (%d classes)" % (bad[0], models.n_classes))
        obj_class = torch.tensor(host, dtype=torch.int32).to(points4.device)
    if float(max_correspondence_distance) > models.cell:
        raise ValueError("icp_polish: max_correspondence_distance %g exceeds the cell size %g the model grids were built for"
                         % (max_correspondence_distance, models.cell))
    if tuple(points4.shape[2:]) != (4,) or n_cand.shape[0] != n or obj_class.shape[0] != n or tuple(pose.shape) != (n, 7):
        raise ValueError("icp_polish: points4[n,N,4], n_cand[n], obj_class[n] and pose[n,7] must agree")
    pose_out = torch.empty(n, 7, dtype=torch.float64, device=points4.device)
    stats = torch.empty(n, 4, dtype=torch.float64, device=points4.device)
    head = (n, _lib.dptr(points4, torch.float32), _lib.dptr(n_cand, torch.int32), npts, _lib.dptr(obj_class, torch.int32),
            _lib.dptr(models.table, torch.int64))
    tail = (models.n_classes, models.max_points, models.cell, _lib.dptr(pose, torch.float64), float(max_correspondence_distance),
            float(criteria.relative_fitness), float(criteria.relative_rmse), int(criteria.max_iteration), float(min_fitness), _lib.dptr(pose_out),
            _lib.dptr(stats), _st())
    if plane:
        _lib.call.ape_icp_polish_plane_batch_f64(*head, _lib.dptr(models.normals_table, torch.int64), *tail)
    else:
        _lib.call.ape_icp_polish_batch_f64(*head, *tail)
    return pose_out, stats


# ---- overlays (csrc/overlay.hip) ------------------------------------------------------------------------------------------
OVERLAY_F64, OVERLAY_U8 = 0, 1      # blend arithmetic: full_prediction's float64 images / the review screens' uint8 arrays
_overlay_planes = {}


def overlay_planes(j, b, h, w, device):
    """the count planes [J,B,H,W] (u32 counts in an int32 tensor) of an overlay call: one cached buffer per device and stream, grown on
    demand (the stamp call clears what it uses); fresh memory while a graph is being captured"""
    n = j * b * h * w
    if CAPTURING:
        return torch.empty(n, dtype=torch.int32, device=device).view(j, b, h, w)
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    buf = _overlay_planes.get(key)
    if buf is None or buf.numel() < n:
        buf = _overlay_planes[key] = torch.empty(n, dtype=torch.int32, device=device)
    return buf[:n].view(j, b, h, w)


def overlay_stamp_counts(objs_host, clouds, pose, n_cand, intr, point_size, planes):
    """objs_host[n,4] int32 numpy (frame, first cloud row, rows, plane), clouds[sum M,3] f64, pose[n,7] (w,x,y,z,t) or [n,3,4] ([R|t]) f64,
    n_cand[n] i32 or None -> planes[J,B,H,W] cleared, then one count per stamp centre whose stamp lies inside the image"""
    import numpy as np
    objs_host = np.ascontiguousarray(objs_host, dtype=np.int32).reshape(-1, 4)
    n = objs_host.shape[0]
    j, b, h, w = planes.shape
    form = 0 if pose.dim() == 2 and pose.shape[1] == 7 else 1 if tuple(pose.shape[1:]) == (3, 4) else None
    if form is None or pose.shape[0] != n or (n_cand is not None and n_cand.numel() != n) or clouds.dim() != 2 or clouds.shape[1] != 3:
        raise _lib.ApeError("overlay_stamp_counts: pose[n,7] or [n,3,4], n_cand[n] and clouds[M,3] expected for %d objects, got %s, %s, %s"
                            % (n, tuple(pose.shape), None if n_cand is None else tuple(n_cand.shape), tuple(clouds.shape)))
    label = "overlay_stamp_counts_kernel"
    e0 = _prof_begin(label)
    _lib.call.ape_overlay_stamp_counts_f64(objs_host.ctypes.data_as(ctypes.c_void_p), n, _lib.dptr(clouds, torch.float64), clouds.shape[0],
                                           _lib.dptr(pose, torch.float64), form, _lib.dptr(n_cand, torch.int32) if n_cand is not None else None,
                                           float(intr["fx"]), float(intr["fy"]), float(intr["ppx"]), float(intr["ppy"]), int(point_size),
                                           _lib.dptr(planes, torch.int32), j, b, h, w, _st())
    rows = int(objs_host[:, 2].sum()) if n else 0
    _prof_end(e0, label, "%dx%dx%d n%d pts%d" % (b, h, w, n, rows), 40.0 * rows, 24.0 * rows + 4.0 * rows + 4.0 * j * b * h * w)
    return planes


def overlay_blend(rgb, objmap, slot_obj, obj_cls, seg_colour, mark, n_cand, planes, point_size, mode):
    """rgb[B,H,W,3] u8, objmap[B,H,W] u8 or None, slot_obj[B,J] i32, obj_cls[n] i32, seg_colour / mark [n,3] f64 or None (red), n_cand[n] i32
    or None, planes[J,B,H,W] -> (seg[B,H,W,3], pose[B,H,W,3]) u8"""
    j, b, h, w = planes.shape
    n = obj_cls.numel()
    if tuple(rgb.shape) != (b, h, w, 3) or tuple(slot_obj.shape) != (b, j) or (objmap is not None and tuple(objmap.shape) != (b, h, w)):
        raise _lib.ApeError("overlay_blend: rgb[B,H,W,3], objmap[B,H,W] and slot_obj[B,J] expected for planes %s, got %s, %s, %s"
                            % (tuple(planes.shape), tuple(rgb.shape), None if objmap is None else tuple(objmap.shape), tuple(slot_obj.shape)))
    for name, t in (("seg_colour", seg_colour), ("mark", mark)):
        if t is not None and tuple(t.shape) != (n, 3):
            raise _lib.ApeError("overlay_blend: %s[%d,3] expected, got %s" % (name, n, tuple(t.shape)))
    if n_cand is not None and n_cand.numel() != n:
        raise _lib.ApeError("overlay_blend: n_cand[%d] expected, got %s" % (n, tuple(n_cand.shape)))
    if rgb.data_ptr() & 3:
        rgb = rgb.clone()               # (a view that starts inside an allocation: the kernel reads dwords)
    seg = torch.empty_like(rgb)
    pose_img = torch.empty_like(rgb)
    label = "overlay_blend_kernel"
    e0 = _prof_begin(label)
    opt = lambda t, dt: _lib.dptr(t, dt) if t is not None else None  # noqa: E731
    _lib.call.ape_overlay_blend_u8(_lib.dptr(rgb, torch.uint8), opt(objmap, torch.uint8), _lib.dptr(slot_obj, torch.int32),
                                   _lib.dptr(obj_cls, torch.int32), opt(seg_colour, torch.float64), opt(mark, torch.float64),
                                   opt(n_cand, torch.int32), n, _lib.dptr(planes, torch.int32), j, b, h, w, int(point_size), int(mode),
                                   _lib.dptr(seg), _lib.dptr(pose_img), _st())
    px = b * h * w
    _prof_end(e0, label, "%dx%dx%d J%d" % (b, h, w, j), 12.0 * px, px * (3.0 + 1.0 + 4.0 * j + 6.0))
    return seg, pose_img


# ---- ADD / ADD-S ------------------------------------------------------------------------------------------------------
def adds_dis(pred_r, pred_t, points, model, target, symmetric, want_pred=False, want_std=True):
    """pred_r[N,4], pred_t[N,3], points[N,3]|None, model[M,3], target[M,3] -> dis[N], std[N]|None, pred[N,M,3]|None"""
    n, m = pred_r.shape[0], model.shape[0]
    dev = pred_r.device
    dis = torch.empty(n, dtype=torch.float32, device=dev)
    std = torch.empty(n, dtype=torch.float32, device=dev) if want_std else None
    pred = torch.empty(n, m, 3, dtype=torch.float32, device=dev) if want_pred else None
    _lib.call.ape_adds_dis_f32(_lib.dptr(pred_r, torch.float32), _lib.dptr(pred_t, torch.float32), _lib.dptr(points),
                               _lib.dptr(model, torch.float32), _lib.dptr(target, torch.float32), n, m,
                               int(bool(symmetric)), _lib.dptr(pred), _lib.dptr(dis), _lib.dptr(std), _st())
    return dis, std, pred


def adds_dis_batched(pred_r, pred_t, model, target, symmetric):
    """pred_r[B,4], pred_t[B,3], model[B,M,3], target[B,M,3] -> dis[B]: ADD / ADD-S of B objects, each against its own clouds, in one launch"""
    b, m = model.shape[0], model.shape[1]
    dis = torch.empty(b, dtype=torch.float32, device=model.device)
    ws = torch.empty(b, m, dtype=torch.float32, device=model.device)          # per-point distances (the mean is a second launch)
    _lib.call.ape_adds_dis_batched_f32(_lib.dptr(pred_r, torch.float32), _lib.dptr(pred_t, torch.float32), _lib.dptr(model, torch.float32),
                                       _lib.dptr(target, torch.float32), b, m, int(bool(symmetric)), _lib.dptr(ws), _lib.dptr(dis), _st())
    return dis


# the tile sizes of csrc/pose_errors.hip, for the tests' edge shapes: reference points per LDS chunk, model points a workgroup owns at one
# lane per point (POSE_ERRORS_QUERIES // lanes at more), and the lanes per model point a call may run with
POSE_ERRORS_CHUNK = 1024
POSE_ERRORS_QUERIES = 512
POSE_ERRORS_LANES = (1, 4, 16, 64)


def pose_errors_lanes(n_pairs, m_max):
    """the lanes per model point ape_pose_errors_f64 takes for n_pairs = n_inst * n_src (instance, source) pairs and a longest model of m_max"""
    return _lib.lib().ape_pose_errors_lanes(int(n_pairs), int(m_max))


def pose_errors(models, offsets, cls, rt_gt, rt_est, valid):
    """The YCB toolbox's adi, add, re and te (evaluate_poses_keyframe.m:148-217) of n_inst objects x n_src pose sources in one call, float64.
    models[sum M_c, 3] f64: the model points of all classes; offsets[n_models + 1] i32 into it; cls[n_inst] i32 (0-based); rt_gt[n_inst, 3, 4]
    and rt_est[n_inst, n_src, 3, 4] f64; valid[n_inst, n_src] u8 -> tensor[n_inst, n_src, 4] f64 = (adi, add, re in degrees, te); +inf where
    valid is 0 (that pose is not read).  Everything is device memory; the table and the classes are checked here (two small reads)."""
    lib = _lib.lib()
    if (lib.ape_pose_errors_chunk(), lib.ape_pose_errors_queries()) != (POSE_ERRORS_CHUNK, POSE_ERRORS_QUERIES):
        raise _lib.ApeError("engine.POSE_ERRORS_* do not mirror csrc/pose_errors.hip")
    for name, t, dt in (("models", models, torch.float64), ("offsets", offsets, torch.int32), ("cls", cls, torch.int32),
                        ("rt_gt", rt_gt, torch.float64), ("rt_est", rt_est, torch.float64), ("valid", valid, torch.uint8)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise _lib.ApeError("pose_errors: %s must be a contiguous %s tensor on the device" % (name, dt))
    if models.dim() != 2 or models.shape[1] != 3 or offsets.dim() != 1 or offsets.numel() < 2 or cls.dim() != 1:
        raise _lib.ApeError("pose_errors: models[sum M, 3], offsets[n_models + 1] and cls[n_inst] expected, got %s, %s, %s"
                            % (tuple(models.shape), tuple(offsets.shape), tuple(cls.shape)))
    n_inst = cls.shape[0]
    if rt_est.dim() != 4 or tuple(rt_est.shape[2:]) != (3, 4) or rt_est.shape[0] != n_inst or rt_est.shape[1] < 1:
        raise _lib.ApeError("pose_errors: rt_est[n_inst, n_src >= 1, 3, 4] expected, got %s" % (tuple(rt_est.shape),))
    n_src = rt_est.shape[1]
    if tuple(rt_gt.shape) != (n_inst, 3, 4) or tuple(valid.shape) != (n_inst, n_src):
        raise _lib.ApeError("pose_errors: rt_gt[n_inst, 3, 4] and valid[n_inst, n_src] expected, got %s, %s" % (tuple(rt_gt.shape), tuple(valid.shape)))
    off = offsets.cpu().numpy().astype("int64")
    n_models = off.size - 1
    lengths = off[1:] - off[:-1]
    if off[0] < 0 or (lengths < 0).any() or off[-1] > models.shape[0]:
        raise _lib.ApeError("pose_errors: offsets must rise from >= 0 to at most %d rows, got %s" % (models.shape[0], off.tolist()))
    out = torch.empty(n_inst, n_src, 4, dtype=torch.float64, device=models.device)
    if n_inst == 0:
        return out
    lo, hi = (int(v) for v in torch.aminmax(cls))
    if lo < 0 or hi >= n_models:
        raise _lib.ApeError("pose_errors: classes %d..%d outside the table's 0..%d" % (lo, hi, n_models - 1))
    m_max = max(1, int(lengths.max()))
    nbytes = lib.ape_pose_errors_workspace_bytes(n_inst * n_src, m_max)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=models.device)
    _lib.call.ape_pose_errors_f64(_lib.dptr(models), _lib.dptr(offsets), n_models, models.shape[0], _lib.dptr(cls), _lib.dptr(rt_gt),
                                  _lib.dptr(rt_est), _lib.dptr(valid), n_inst, n_src, m_max, _lib.dptr(out), _lib.dptr(ws), ws.numel(), _st())
    return out


def adds_select(dis, std, pred_c, pred_r, pred_t, points, w):
    """-> out9 (loss, dis[which], q[4], t[3]) f32 on device, which i32[1]"""
    out = torch.empty(9, dtype=torch.float32, device=dis.device)
    which = torch.empty(1, dtype=torch.int32, device=dis.device)
    _lib.call.ape_adds_select_f32(_lib.dptr(dis), _lib.dptr(std), _lib.dptr(pred_c, torch.float32), _lib.dptr(pred_r),
                                  _lib.dptr(pred_t), _lib.dptr(points), dis.shape[0], float(w), _lib.dptr(out),
                                  _lib.dptr(which), _st())
    return out, which


def recentre_qt(pts, qt7):
    """pts[n,3], qt7 (device f32 [7]: unnormalised quaternion + translation) -> (pts - t) . R(q)"""
    out = torch.empty_like(pts)
    _lib.call.ape_recentre_qt_f32(_lib.dptr(pts, torch.float32), _lib.dptr(qt7, torch.float32), _lib.dptr(out),
                                  pts.shape[0], _st())
    return out


# ---- classical RGB-D labeller (csrc/label_rgbd.hip; label_generator/utils.py) -------------------------------------------------------
RGBD_MODE_RGB, RGBD_MODE_HSV, RGBD_MODE_BOTH = 0, 1, 2
_F64 = torch.float64


def rgbd_gate(depth, measure_dist):
    """depth[B,H,W] u16, measure_dist[B] f64 -> f64 [B,H,W]: the value inside measure_dist +- 150, else 0"""
    b, h, w = depth.shape
    out = torch.empty(b, h, w, dtype=_F64, device=depth.device)
    _lib.call.ape_rgbd_gate_f64(_lib.dptr(depth, torch.uint16), _lib.dptr(measure_dist, _F64), _lib.dptr(out), b, h, w, _st())
    return out


def rgbd_plane_fill(b_depth, pts, valid, window):
    """the centre window (r0, r1, c0, c1) of the gated background depth b_depth[B,H,W] f64, IN PLACE: holes filled from the plane through
    pts[B,3,3] f64, then the 5 x 5 box filter; frames with valid[B] i32 == 0 stay as they are"""
    b, h, w = b_depth.shape
    r0, r1, c0, c1 = window
    tmp = torch.empty(b, r1 - r0, c1 - c0, dtype=_F64, device=b_depth.device)
    _lib.call.ape_rgbd_plane_fill_f64(_lib.dptr(b_depth, _F64), _lib.dptr(pts, _F64), _lib.dptr(valid, torch.int32), _lib.dptr(tmp), b, h, w,
                                      r0, r1, c0, c1, _st())
    return b_depth


def rgbd_score(f_rgb, b_rgb, f_depth, b_depth, measure_dist, mode, weights, depth_weight, threshold):
    """-> (score, color) f64 [B,H,W]; weights: up to six channel weights; depth_weight <= 0: no depth term (the depth arguments may be None)"""
    b, h, w, _ = f_rgb.shape
    score = torch.empty(b, h, w, dtype=_F64, device=f_rgb.device)
    color = torch.empty_like(score)
    w7 = (ctypes.c_double * 7)(*([float(v) for v in weights] + [0.0] * (6 - len(weights)) + [float(depth_weight)]))
    _lib.call.ape_rgbd_score_f64(_lib.dptr(f_rgb, torch.uint8), _lib.dptr(b_rgb, torch.uint8),
                                 _lib.dptr(f_depth, torch.uint16) if f_depth is not None else None,
                                 _lib.dptr(b_depth, _F64) if b_depth is not None else None,
                                 _lib.dptr(measure_dist, _F64) if measure_dist is not None else None, mode,
                                 ctypes.cast(w7, ctypes.c_void_p), float(threshold), _lib.dptr(score), _lib.dptr(color), b, h, w, _st())
    return score, color


def rgbd_morph(img, k, dilate, out=None):
    """erode / dilate of img[B,H,W] f64 with a k x k all-ones kernel; out may be img"""
    b, h, w = img.shape
    out = torch.empty_like(img) if out is None else out
    tmp = torch.empty_like(img)
    _lib.call.ape_rgbd_morph_f64(_lib.dptr(img, _F64), _lib.dptr(out, _F64), _lib.dptr(tmp), b, h, w, int(k), int(bool(dilate)), _st())
    return out


def rgbd_open_close(img, open, close):
    """MORPH_OPEN with `open`, then MORPH_CLOSE with `close` (0 skips); img itself is never written: it is returned when both are skipped"""
    cur = img
    for k, dil in ((open, 0), (open, 1), (close, 1), (close, 0)):
        if k > 0:
            cur = rgbd_morph(cur, k, dil, out=None if cur is img else cur)
    return cur


def rgbd_wrap_u8(img):
    out = torch.empty(img.shape, dtype=torch.uint8, device=img.device)
    _lib.call.ape_rgbd_wrap_u8(_lib.dptr(img, _F64), _lib.dptr(out), img.numel(), _st())
    return out


def _rgbd_ws(b, h, w, device):
    nbytes = _lib.lib().ape_rgbd_cca_workspace_bytes(b, h, w)
    if nbytes == 0 and b:
        raise ValueError("batch of %d frames of %d x %d is outside the labeller's limits" % (b, h, w))
    return _workspace(max(nbytes, 256), device)


def rgbd_component_stats(img):
    """img[B,H,W] f64 -> root i32 (index of the component's first pixel in the batch, -1 = background), and at those first pixels
    count u32 and sum f64 of img over the component"""
    b, h, w = img.shape
    root = torch.empty(b, h, w, dtype=torch.int32, device=img.device)
    count = torch.empty(b, h, w, dtype=torch.uint32, device=img.device)
    total = torch.empty(b, h, w, dtype=_F64, device=img.device)
    ws = _rgbd_ws(b, h, w, img.device)
    _lib.call.ape_rgbd_component_stats(_lib.dptr(img, _F64), _lib.dptr(root), _lib.dptr(count), _lib.dptr(total), b, h, w, _lib.dptr(ws),
                                       ws.numel(), _st())
    return root, count, total


def rgbd_cca_round(img, color, min_size, by_size, remove_one_std=False, final=False, want_mean_std=False):
    """one component round on img[B,H,W] f64: color is masked (and cut) IN PLACE, or with final=True the u8 mask is returned"""
    b, h, w = img.shape
    out = torch.empty(b, h, w, dtype=torch.uint8, device=img.device) if final else None
    ms = torch.empty(b, 2, dtype=_F64, device=img.device) if want_mean_std else None
    ws = _rgbd_ws(b, h, w, img.device)
    _lib.call.ape_rgbd_cca_round(_lib.dptr(img, _F64), _lib.dptr(color, _F64), _lib.dptr(out) if final else None,
                                 _lib.dptr(ms) if want_mean_std else None, b, h, w, int(min_size), int(bool(by_size)),
                                 int(bool(remove_one_std)), _lib.dptr(ws), ws.numel(), _st())
    if want_mean_std:
        return (out if final else color), ms
    return out if final else color


def rgbd_box(img, k=5):
    """the reference's `smoothing`: k x k box filter of img[B,H,W] f64 with float32 taps, BORDER_REFLECT_101"""
    b, h, w = img.shape
    out = torch.empty_like(img)
    _lib.call.ape_rgbd_box_f64(_lib.dptr(img, _F64), _lib.dptr(out), b, h, w, int(k), _st())
    return out


# ---- label-quality audit (csrc/label_audit.hip; experiments/gt_test.py) ---------------------------------------------------------------
def label_pair_counts(labels, pairs):
    """labels[B,L,H,W] u8 (L <= 8 label planes per sample, non-zero = foreground), pairs: up to 16 plane pairs (a, b) -> int64 [B,P,4]:
    per sample and pair the pixels with a fg & b fg, a fg & b bg, a bg & b fg, both bg -- compute_IoU's tp, fp, fn, tn, its naming"""
    if labels.dim() != 4:
        raise ValueError("labels must be [B, L, H, W], got %s" % (tuple(labels.shape),))
    b, l, h, w = labels.shape
    flat = [int(v) for pr in pairs for v in pr]
    if not flat or len(flat) % 2 or any(len(pr) != 2 for pr in pairs):
        raise ValueError("pairs must be a non-empty list of (a, b) plane indices")
    p = len(flat) // 2
    counts = torch.empty(b, p, 4, dtype=torch.int64, device=labels.device)
    table = (ctypes.c_int32 * (2 * p))(*flat)
    _lib.call.ape_label_pair_counts_u8(_lib.dptr(labels, torch.uint8), b, l, h * w, ctypes.cast(table, ctypes.c_void_p), p, _lib.dptr(counts),
                                       _st())
    return counts


def label_pair_blend(rgb, labels, first, second, c0, c1):
    """rgb[B,H,W,3] u8, labels[B,L,H,W] u8, first = (plane_a, ch_a), second = (plane_b, ch_b) -> u8 [B,H,W,3]: the frame with
    `v*c0 + label*c1` (float64, truncated) in channel ch_a where plane_a is set, then the same for plane_b / ch_b on that result"""
    if rgb.dim() != 4 or rgb.shape[3] != 3 or labels.dim() != 4 or labels.shape[0] != rgb.shape[0] or tuple(labels.shape[2:]) != tuple(rgb.shape[1:3]):
        raise ValueError("rgb must be [B, H, W, 3] and labels [B, L, H, W] of the same frames, got %s and %s"
                         % (tuple(rgb.shape), tuple(labels.shape)))
    if labels.device != rgb.device:
        raise ValueError("rgb is on %s, labels on %s" % (rgb.device, labels.device))
    b, h, w, _ = rgb.shape
    out = torch.empty_like(rgb)
    _lib.call.ape_label_pair_blend_u8(_lib.dptr(rgb, torch.uint8), _lib.dptr(labels, torch.uint8), b, labels.shape[1], h, w, int(first[0]),
                                      int(first[1]), int(second[0]), int(second[1]), float(c0), float(c1), _lib.dptr(out), _st())
    return out

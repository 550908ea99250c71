"""Inputs for the edge-shape tests of csrc/unet.hip (decoder conv and fused head) and of the split-K form of csrc/conv_gemm.hip, each named
for the shape and the branch it reaches.  tests/test_conv_edges_host.py proves the guards and the branch-reached claims on the CPU;
tests/test_gpu_unet_edges.py and tests/test_gpu_splitk_edges.py run them.  Below them, under the same input rules, the cases of the LDS-halo
3x3 kernels (csrc/conv3x3_halo.hip, csrc/conv3x3_halo_s32.hip): proofs in tests/test_halo_edges_host.py, run by tests/test_gpu_halo_edges.py.

Input rules ("Pinned at edge shapes" of the Unet decoder kernel and the split-K GEMM):
 1. fixed seeds; activations ~ N(0, 1), weights ~ N(0, 1) / sqrt(K) (head: 2 / sqrt(K), logits of scale >= 1), so outputs are of scale 1..10;
 2. every operand tensor is wider than the channels read and the unread channels are NaN: an over-read poisons the result;
 3. every output is a window of a wider buffer filled with a sentinel, with guard elements in front of and behind the buffer;
 4. every split-K case is one the library splits (splitk_plan mirrors splitk_tiles of conv_gemm.hip)."""
import functools
import math

import torch

import conv_products_reference as R

NAN = float("nan")
Y_SENTINEL, SCORE_SENTINEL, LABEL_SENTINEL, WS_SENTINEL = -777.0, -5.0, 171, -333.0
GUARD = 64                              # elements in front of and behind every device buffer
BAR = 2e-6                              # same products, other float32 summation order (test_gpu_conv.py, test_gpu_train.py)
TOL = {1: 2e-2, 3: 5e-5}                # against the plain (unsplit) float64 convolution: test_gpu_conv.py's TOL for bf16 / bf16x3
PRECISION = {1: "bf16", 3: "bf16x3"}
EXCLUDE_CAP = 1e-3

# ---- csrc/unet.hip: the decoder conv ----------------------------------------------------------------------------------------------------------
UNET_WAVES = 4
UNET_MAPS_UPS = ((1, 2, 2), (2, 10, 14), (3, 14, 18))                     # output maps (B, H, W), up-sampled from (H / 2, W / 2)
UNET_MAPS_FULL = ((1, 5, 7), (2, 1, 33), (1, 9, 1), (3, 13, 17))
UNET_MAPS = tuple((m, 1) for m in UNET_MAPS_UPS) + tuple((m, 0) for m in UNET_MAPS_FULL)
UNET_CHANNELS = ((16, 0), (16, 16), (48, 16), (32, 48), (80, 0), (64, 64))
UNET_COUT = (16, 32, 48, 64, 80, 128)
UNET_INSTANTIATIONS = ((4, 4), (2, 8), (1, 8))                            # (NC, NP) of launch_relu
HEAD_CLASSES = (1, 2, 3, 13, 16)
LDA_EXTRA, LDB_EXTRA, YOFF, LDY_EXTRA = 12, 4, 4, 8


def unet_instantiation(cout):
    """(NC, NP) launch_relu of csrc/unet.hip picks for `cout` output channels"""
    return (4, 4) if cout >= 64 else (2, 8) if cout in (32, 48) else (1, 8)


def _unet_name(kind, m, ups, ch, cout):
    return "%s_%s_%dx%dx%d_c%d+%d_o%d" % (kind, "ups" if ups else "full", m[0], m[1], m[2], ch[0], ch[1], cout)


def _unet_conv_cases():
    """every map and every channel split with every instantiation, every Cout with its own; the channel list is rotated per instantiation
    so that the up-sampled maps meet a k-step that holds both A and B channels under each of them"""
    cases = {}
    for k, inst in enumerate(UNET_INSTANTIATIONS):
        couts = [c for c in UNET_COUT if unet_instantiation(c) == inst]
        for i, (m, ups) in enumerate(UNET_MAPS):
            ch, cout = UNET_CHANNELS[(i + k) % 6], couts[i % len(couts)]
            cases[_unet_name("nc%dnp%d" % inst, m, ups, ch, cout)] = dict(map=m, ups=ups, C1=ch[0], C2=ch[1], Cout=cout, seed=100 * k + i)
    # the NC = 4 instantiation at Cout % 64 != 0 under a k-step that holds both A and B channels, without up-sampling
    cases[_unet_name("nc4np4", (3, 13, 17), 0, (48, 16), 80)] = dict(map=(3, 13, 17), ups=0, C1=48, C2=16, Cout=80, seed=77)
    return cases


UNET_CONV_CASES = _unet_conv_cases()


def _dup(C, pairs):
    d = list(range(C))
    for lo, hi in pairs:
        d[hi] = lo
    return tuple(d)


def _unet_head_cases():
    cases = {}
    for i, (m, ups) in enumerate(UNET_MAPS):
        ch, C = UNET_CHANNELS[(i + 3) % 6], HEAD_CLASSES[i % 5]
        cases[_unet_name("head%s" % ("" if i % 2 == 0 else "_nobias"), m, ups, ch, C)] = dict(
            map=m, ups=ups, C1=ch[0], C2=ch[1], Cout=C, bias=i % 2 == 0, dup=None, seed=500 + i)
    # planted ties: weight rows and biases duplicated between classes, so the two logits are bit-identical
    ties = (("tie_4_5_same_lane", 16, _dup(16, [(4, 5)])), ("tie_2_9_across_lanes", 13, _dup(13, [(2, 9)])), ("tie_all_equal", 16, (0,) * 16),
            ("tie_all_equal", 3, (0,) * 3))
    for j, (tname, C, dup) in enumerate(ties):
        for (m, ups), ch in (((3, 14, 18), 1), (16, 16)), (((3, 13, 17), 0), (48, 16)):
            cases[_unet_name(tname, m, ups, ch, C)] = dict(map=m, ups=ups, C1=ch[0], C2=ch[1], Cout=C, bias=True, dup=dup, seed=600 + 2 * j + ups)
    for name, seed in HEAD_SEEDS.items():
        cases[name]["seed"] = seed
    return cases


# every head case has fewer than 1000 pixels, so the 0.1 % cap on the label comparison's exclusion band allows none: these seeds replace the
# ones that put a pixel of the float64 restatement inside the band (tests/test_conv_edges_host.py asserts that none is left)
HEAD_SEEDS = {"tie_4_5_same_lane_full_3x13x17_c48+16_o16": 700, "tie_2_9_across_lanes_full_3x13x17_c48+16_o13": 700}


UNET_HEAD_CASES = _unet_head_cases()


def unet_case(name):
    c = dict(UNET_HEAD_CASES[name], head=True) if name in UNET_HEAD_CASES else dict(UNET_CONV_CASES[name], head=False, bias=True, dup=None)
    B, H, W = c["map"]
    c.update(B=B, H=H, W=W, M=B * H * W, Ha=H >> c["ups"], Wa=W >> c["ups"], lda=c["C1"] + LDA_EXTRA, ldb=c["C2"] + LDB_EXTRA if c["C2"] else 0,
             yoff=YOFF, ldy=YOFF + c["Cout"] + LDY_EXTRA, name=name)
    c["inst"] = (1, 8) if c["head"] else unet_instantiation(c["Cout"])
    return c


def _wide(shape, C, g):
    t = torch.full(shape, NAN)
    t[..., :C] = torch.randn(shape[:-1] + (C,), generator=g)
    return t


@functools.lru_cache(maxsize=None)
def unet_inputs(name):
    """-> a[B,Ha,Wa,lda], b[B,H,W,ldb] | None (unread channels NaN), w[Cout,Ctot,3,3], bias[Cout] | None"""
    c = unet_case(name)
    g = torch.Generator().manual_seed(c["seed"])
    Ctot = c["C1"] + c["C2"]
    a = _wide((c["B"], c["Ha"], c["Wa"], c["lda"]), c["C1"], g)
    b = _wide((c["B"], c["H"], c["W"], c["ldb"]), c["C2"], g) if c["C2"] else None
    w = torch.randn(c["Cout"], Ctot, 3, 3, generator=g) * ((2.0 if c["head"] else 1.0) / math.sqrt(9 * Ctot))
    bias = torch.randn(c["Cout"], generator=g) * 0.5
    if c["dup"] is not None:
        src = torch.tensor(c["dup"])
        w, bias = w[src].clone(), bias[src].clone()
    return a, b, w, (bias if c["bias"] else None)


def unet_branches(c):
    """which branches of unet_conv3x3_kernel the case takes (restated from the kernel's index arithmetic)"""
    NC, NP = c["inst"]
    M, W, H = c["M"], c["W"], c["H"]
    Ctot, C1 = c["C1"] + c["C2"], c["C1"]
    wave_px = 16 * NP
    n_waves = -(-M // (wave_px * UNET_WAVES)) * UNET_WAVES
    groups = [(wv * wave_px + 16 * p) for wv in range(n_waves) for p in range(NP)]
    br = set()
    if M % 16:
        br.add("lanes_past_M")                           # the py = -4 lanes of the last group
    if any(g0 >= M for g0 in groups):
        br.add("group_past_M")                           # the wave-uniform `continue`
    if any(g0 < M and (g0 % W) + 15 >= W for g0 in groups) and W % 2:
        br.add("group_straddles_row_odd_W")
    if any(g0 < M and g0 // (H * W) != min(g0 + 15, M - 1) // (H * W) for g0 in groups):
        br.add("group_straddles_image")
    if any(c0 < C1 < c0 + 32 for c0 in range(0, Ctot, 32)):
        br.add("kstep_holds_A_and_B")
    if Ctot % 32:
        br.add("half_empty_kstep")
    if M > wave_px * UNET_WAVES:
        br.add("more_than_one_workgroup")
    if not c["head"] and c["Cout"] % (16 * NC):
        br.add("channel_groups_past_Cout")
    if c["head"] and c["Cout"] < 16:
        br.add("class_rows_past_C")
    if c["lda"] > C1:
        br.add("wide_a")
    if c["C2"] and c["ldb"] > c["C2"]:
        br.add("wide_b")
    return br


@functools.lru_cache(maxsize=None)
def unet_expected(name, nsplit):
    """the restatement's pre-activation output [M, Cout] float64 (bias added); nsplit = 0: the plain float64 convolution"""
    c = unet_case(name)
    a, b, w, bias = unet_inputs(name)
    return R.unet_logits(a, b, w, bias, c["C1"], c["C2"], bool(c["ups"]), nsplit)


# ---- the head's bounds (derived in tests/test_gpu_unet_edges.py's docstring) -------------------------------------------------------------------
EXP_ONE = 2.0 ** -22        # |x| below which the head's fast exponential may return exactly 1 (2^-25 for a true expf; two bits of slack)
P_ROUNDING = 2.0 ** -20     # float32 error of one first-softmax probability on the device (a few ulp of values <= 1)


def logit_bar(ref_logits):
    return BAR * max(1.0, float(ref_logits.abs().max()))


def label_band(ref_logits, C, double_softmax):
    """tau: a pixel whose two largest first-softmax probabilities differ by at least this has the float64 label on the device"""
    d = logit_bar(ref_logits)
    if double_softmax:
        return 2 * d + 2 * C * (2 * P_ROUNDING + EXP_ONE)
    return 2 * d + EXP_ONE


def score_bound(ref_logits, score, double_softmax):
    """softmax is 1/2-Lipschitz in the max norm (sum_j |dp_i / dl_j| = 2 p_i (1 - p_i) <= 1/2), once per softmax; plus the 1e-5 relative of
    seg_head_finish's fast exponentials and reciprocals (test_gpu_segpost_edges.py)"""
    return (0.25 if double_softmax else 0.5) * logit_bar(ref_logits) + 1e-5 * score


# ---- csrc/conv_gemm.hip: the split-K form ----------------------------------------------------------------------------------------------------------
def splitk_plan(g):
    """(nk, nk_per, launched splits) by splitk_tiles' rule as written in conv_gemm.hip; nk_per = 0: the library does not split"""
    M = g["B"] * g["Ho"] * g["Wo"]
    nk = g["KH"] * g["KW"] * g["Cin"] // 32
    tiles = -(-M // 128) * -(-g["Cout"] // 128)
    if g["Cout"] <= 64 or tiles >= 96 or nk < 8:
        return nk, 0, 0
    splits = min(-(-256 // tiles), nk // 4, 32)
    if splits < 2:
        return nk, 0, 0
    nk_per = -(-nk // splits)
    return nk, nk_per, -(-nk // nk_per)


def splitk_requested(g):
    M = g["B"] * g["Ho"] * g["Wo"]
    tiles = -(-M // 128) * -(-g["Cout"] // 128)
    return min(-(-256 // tiles), g["KH"] * g["KW"] * g["Cin"] // 32 // 4, 32)


_G = R.conv_geometry
SPLITK_CASES = {
    # name: (geometry, bias: None | "shared" | "per_image", residual)
    "linear_M1_cout65": (_G(1, 1, 1, 256, 65, ldx=264, xoff=4, ldy=72, yoff=4), "shared", False),
    "pure_slices_per_image_bias_prelu": (_G(3, 37, 1, 288, 130, act=R.ACT_PRELU, alpha=0.25, ldx=352, xoff=32, ldy=160, yoff=8, bias_bstride=136,
                                            ldr=140, roff=4), "per_image", True),
    "dil2_second_split_starts_at_tap5_sigmoid": (_G(2, 9, 11, 32, 72, k=3, pad=2, dil=2, act=R.ACT_SIGMOID, ldx=40, xoff=4, ldy=80, yoff=4,
                                                    bias_bstride=80), "per_image", False),
    "pad1_splits_start_mid_chunk_last_has_3": (_G(2, 9, 11, 64, 72, k=3, pad=1, act=R.ACT_RELU, ldx=72, xoff=8, ldy=76, yoff=0, ldr=80, roff=8),
                                               "shared", True),
    "stride2_one_tap_not_pure": (_G(2, 9, 11, 256, 96, stride=2, act=R.ACT_RELU, ldx=260, xoff=4, ldy=100, yoff=4), "shared", False),
    "pure_cin672_last_split_one_ktile": (_G(1, 5, 9, 672, 80, ldx=680, xoff=8, ldy=88, yoff=4), None, False),
    "pure_cin1056_fewer_splits_launched": (_G(1, 20, 1, 1056, 66, act=R.ACT_PRELU, alpha=0.25, ldx=1060, xoff=0, ldy=68, yoff=0), "shared", False),
    "M129_cout129_ragged_second_tiles": (_G(1, 3, 43, 256, 129, act=R.ACT_RELU, ldx=256 + 8, xoff=8, ldy=129 + 7, yoff=4, ldr=132, roff=0),
                                         "shared", True),
}


@functools.lru_cache(maxsize=None)
def splitk_inputs(name):
    """-> geometry, x[B,H,W,ldx], w[Cout,Cin,k,k], bias (flat, NaN between the per-image rows) | None, res[B,Ho,Wo,ldr] | None"""
    g, bias_kind, with_res = SPLITK_CASES[name]
    gen = torch.Generator().manual_seed(1000 + list(SPLITK_CASES).index(name))
    x = torch.full((g["B"], g["H"], g["W"], g["ldx"]), NAN)
    x[..., g["xoff"]:g["xoff"] + g["Cin"]] = torch.randn(g["B"], g["H"], g["W"], g["Cin"], generator=gen)
    w = torch.randn(g["Cout"], g["Cin"], g["KH"], g["KW"], generator=gen) / math.sqrt(g["Cin"] * g["KH"] * g["KW"])
    bias = None
    if bias_kind == "shared":
        bias = torch.randn(g["Cout"], generator=gen)
    elif bias_kind == "per_image":
        bias = torch.full((g["B"], g["bias_bstride"]), NAN)
        bias[:, :g["Cout"]] = torch.randn(g["B"], g["Cout"], generator=gen)
        bias = bias.reshape(-1)
    res = None
    if with_res:
        res = torch.full((g["B"], g["Ho"], g["Wo"], g["ldr"]), NAN)
        res[..., g["roff"]:g["roff"] + g["Cout"]] = torch.randn(g["B"], g["Ho"], g["Wo"], g["Cout"], generator=gen)
    return g, x, w, bias, res


@functools.lru_cache(maxsize=None)
def splitk_expected(name, nsplit):
    g, x, w, bias, res = splitk_inputs(name)
    return R.conv(x, w, g, nsplit, bias, res)


# ---- csrc/conv3x3_halo.hip: ape_conv3x3_halo_bf16 through its raw entry point -------------------------------------------------------------------------
# (the engine routes only maps whose 16 x 16 tiles are at least 80 % full; the ABI takes any H, W >= 1)
S32_SENTINEL = -194.0                   # every bf16 of an S32 output buffer before the call (bits 0xC342 in both planes)
_H = R.halo_geometry
_PRELU = dict(act=R.ACT_PRELU, alpha=0.25)
HALO_CASES = {
    # name: (geometry, bias: None | "shared" | "per_image", residual)
    "d1_n64_1x1x1_cin32_one_chunk_cout4_null_bias_act_none": (_H(1, 1, 1, 32, 4, 1, ldx=40, xoff=4, ldy=12, yoff=4), None, False),
    "d4_n64_1x3x5_off_centre_taps_outside_cout13_scalar_nvalid1_sigmoid": (
        _H(1, 3, 5, 64, 13, 4, act=R.ACT_SIGMOID, ldx=76, xoff=8, ldy=24, yoff=4), "shared", False),
    "d2_n128_1x3x5_cin96_cout65_63_empty_rows_scalar_by_ldy": (_H(1, 3, 5, 96, 65, 2, act=R.ACT_RELU, ldx=104, xoff=4, ldy=70, yoff=4), "shared", False),
    "d1_n128_2x1x33_cout129_second_channel_tile_of_one_scalar_by_yoff_per_image_bias": (
        _H(2, 1, 33, 64, 129, 1, ldx=72, xoff=4, ldy=136, yoff=2, bias_bstride=136, **_PRELU), "per_image", False),
    "d2_n64_1x9x1_cin32_cout64_scalar_by_roff_null_bias": (
        _H(1, 9, 1, 32, 64, 2, act=R.ACT_RELU, ldx=36, xoff=4, ldy=72, yoff=4, ldr=72, roff=2), None, True),
    "d1_n128_1x16x16_one_full_tile_cin96_cout128_vector_residual_slice": (
        _H(1, 16, 16, 96, 128, 1, ldx=104, xoff=8, ldy=140, yoff=8, ldr=136, roff=4, **_PRELU), "shared", True),
    "d4_n128_1x17x16_second_tile_row_of_one_cout200_sigmoid": (
        _H(1, 17, 16, 32, 200, 4, act=R.ACT_SIGMOID, ldx=52, xoff=16, ldy=208, yoff=4, bias_bstride=204), "per_image", False),
    "d2_n128_3x13x17_second_tile_column_of_one_six_workgroups_act_none": (
        _H(3, 13, 17, 64, 128, 2, ldx=96, xoff=32, ldy=136, yoff=4, ldr=136, roff=4, bias_bstride=132), "per_image", True),
    "d1_n64_3x13x17_cin96_single_buffer_refill_odd_chunks": (_H(3, 13, 17, 96, 64, 1, act=R.ACT_RELU, ldx=100, xoff=4, ldy=72, yoff=4), "shared", False),
    "d4_n64_2x32x48_cin64_cout64_null_bias_vector_residual": (
        _H(2, 32, 48, 64, 64, 4, ldx=76, xoff=8, ldy=72, yoff=4, ldr=68, roff=4, **_PRELU), None, True),
    # fused x2 up-sampling (dil 1): H, W are the up-sampled map's
    "ups_n64_1x1x1_to_2x2_cin32_cout64": (_H(1, 2, 2, 32, 64, 1, 1, act=R.ACT_RELU, ldx=36, xoff=0, ldy=72, yoff=4), "shared", False),
    "ups_n128_2x5x7_to_10x14_xoff8_cout128_vector_residual": (
        _H(2, 10, 14, 64, 128, 1, 1, act=R.ACT_RELU, ldx=76, xoff=8, ldy=136, yoff=4, ldr=132, roff=4), "shared", True),
    "ups_n64_1x8x8_to_16x16_cin96_cout4_per_image_bias": (_H(1, 16, 16, 96, 4, 1, 1, ldx=100, xoff=0, ldy=12, yoff=4, bias_bstride=8, **_PRELU), "per_image", False),
    "ups_n128_3x9x12_to_18x24_cout65_null_bias_sigmoid": (_H(3, 18, 24, 32, 65, 1, 1, act=R.ACT_SIGMOID, ldx=40, xoff=0, ldy=72, yoff=4), None, False),
}


def _operands(g, bias_kind, with_res, gen, s32_in=False):
    """x (float32, unread channels NaN), w, bias (flat, NaN between the per-image rows) | None, res (float32, NaN outside its slice) | None"""
    hl, wl = (g["H"] >> 1, g["W"] >> 1) if g["ups"] else (g["H"], g["W"])
    x = torch.full((g["B"], hl, wl, g["ldx"]), NAN)
    x[..., g["xoff"]:g["xoff"] + g["Cin"]] = torch.randn(g["B"], hl, wl, g["Cin"], generator=gen)
    w = torch.randn(g["Cout"], g["Cin"], 3, 3, generator=gen) / math.sqrt(9 * g["Cin"])
    bias = None
    if bias_kind == "shared":
        bias = torch.randn(g["Cout"], generator=gen)
    elif bias_kind == "per_image":
        bias = torch.full((g["B"], g["bias_bstride"]), NAN)
        bias[:, :g["Cout"]] = torch.randn(g["B"], g["Cout"], generator=gen)
        bias = bias.reshape(-1)
    res = None
    if with_res:
        res = torch.full((g["B"], g["H"], g["W"], g["ldr"]), NAN)
        res[..., g["roff"]:g["roff"] + g["Cout"]] = torch.randn(g["B"], g["H"], g["W"], g["Cout"], generator=gen)
    return x, w, bias, res


@functools.lru_cache(maxsize=None)
def halo_inputs(name):
    """-> geometry, x[B,H,W,ldx] (with ups: [B,H/2,W/2,ldx]), w[Cout,Cin,3,3], bias | None, res[B,H,W,ldr] | None"""
    g, bias_kind, with_res = HALO_CASES[name]
    return (g,) + _operands(g, bias_kind, with_res, torch.Generator().manual_seed(2000 + list(HALO_CASES).index(name)))


@functools.lru_cache(maxsize=None)
def halo_expected(name, nsplit):
    g, x, w, bias, res = halo_inputs(name)
    return R.halo_conv(x, w, g, nsplit, bias, res)


def halo_branches(g, with_res):
    """what conv3x3_halo_kernel<NSPLIT, D, BNH, UPS> meets on this geometry (restated from its index arithmetic and its launcher)"""
    bnh = 64 if g["Cout"] <= 64 else 128
    tx, ty, nt = -(-g["W"] // 16), -(-g["H"] // 16), -(-g["Cout"] // bnh)
    vec_ok = g["ldy"] % 4 == 0 and g["yoff"] % 4 == 0 and (not with_res or (g["ldr"] % 4 == 0 and g["roff"] % 4 == 0))
    return dict(D=g["dil"], BNH=bnh, ups=g["ups"], tiles_x=tx, tiles_y=ty, n_tiles=nt, workgroups=g["B"] * tx * ty * nt,
                last_tile_rows=g["H"] - 16 * (ty - 1), last_tile_cols=g["W"] - 16 * (tx - 1), empty_weight_rows=nt * bnh - g["Cout"],
                chunks=g["Cin"] // 32, a_double=bnh == 128, vec_ok=vec_ok, nvalid_last=g["Cout"] % 4 or 4,
                scalar=(not vec_ok) or g["Cout"] % 4 != 0)


# ---- csrc/conv3x3_halo_s32.hip: ape_conv3x3_halo_s32 ---------------------------------------------------------------------------------------------------
# name: (geometry, bias kind, residual: None | "f32" | "s32", output: "f32" | "s32").  ldx, xoff are multiples of 32 and the unread 32-channel
# groups of the S32 operand hold NaN patterns in every bf16.  The kernel reads a bias row as float4: a per-image bias needs bias_bstride % 4 == 0
# (and a 16-byte aligned base), which the ABI does not check -- every case here keeps to it.
_F32_OUT = lambda cout: dict(ldy=cout + 12, yoff=4)  # noqa: E731
# the S32 output windows of a 160-channel buffer: Cout 136 at 8 takes the wide store, Cout 132 at 0 and Cout 128 at 4 the narrow one
_S32_AT_8, _S32_AT_0, _S32_AT_4 = dict(ldy=160, yoff=8), dict(ldy=160, yoff=0), dict(ldy=160, yoff=4)


HALO_S32_CASES = {
    "d1_1x1x1_cin32_xoff32_f32_out_null_bias_act_none": (_H(1, 1, 1, 32, 128, 1, ldx=64, xoff=32, **_F32_OUT(128)), None, None, "f32"),
    "d4_1x3x5_cin64_xoff64_s32_wide_store": (_H(1, 3, 5, 64, 136, 4, act=R.ACT_RELU, ldx=128, xoff=64, **_S32_AT_8), "shared", None, "s32"),
    "d2_2x12x16_rpw3_every_tile_cin96_xoff32_s32_narrow_by_cout132_s32_residual": (
        _H(2, 12, 16, 96, 132, 2, ldx=128, xoff=32, ldr=160, roff=4, bias_bstride=136, **_PRELU, **_S32_AT_0), "per_image", "s32", "s32"),
    "d1_1x13x16_rpw4_cin160_s32_narrow_by_yoff4_f32_residual_sigmoid": (
        _H(1, 13, 16, 160, 128, 1, act=R.ACT_SIGMOID, ldx=160, xoff=0, ldr=136, roff=4, **_S32_AT_4), "shared", "f32", "s32"),
    "d2_1x17x9_last_tile_row_rpw1_f32_residual_per_image_bias": (
        _H(1, 17, 9, 64, 128, 2, act=R.ACT_RELU, ldx=64, xoff=0, ldr=140, roff=4, bias_bstride=132, **_F32_OUT(128)), "per_image", "f32", "f32"),
    "d4_1x21x33_last_tile_row_rpw2_cout200_two_channel_tiles_sigmoid": (
        _H(1, 21, 33, 32, 200, 4, act=R.ACT_SIGMOID, ldx=32, xoff=0, **_F32_OUT(200)), None, None, "f32"),
    "d1_2x28x17_last_tile_row_rpw3_beside_one_column_tile_s32_wide_s32_residual": (
        _H(2, 28, 17, 96, 136, 1, ldx=96, xoff=0, ldr=160, roff=4, **_PRELU, **_S32_AT_8), "shared", "s32", "s32"),
}
# the persistent walk: more tiles than compute units (ncu, read from the device), so the geometry is a function of ncu.
# H = 17, W = 1: two tile rows per image, rpw 4 then rpw 1.  The kernel deals the logical tiles to the 8 XCDs in contiguous runs and a
# workgroup's next tile is grid / 8 logical tiles further on: with two tiles per image and an even stride the two tiles of a workgroup have
# the SAME rpw in cases a, b (tests/test_halo_edges_host.py proves which); case d (three tile rows per image, rpw 4, 4, 1) is the one whose
# workgroups 0 and 1 walk from an rpw = 4 tile into an rpw = 1 tile.
HALO_S32_WALK_CASES = {
    "walk_a_two_extra_tiles_f32_residual": (lambda ncu: _H(ncu // 2 + 1, 17, 1, 64, 128, 1, act=R.ACT_RELU, ldx=64, ldr=132, roff=4, **_F32_OUT(128)),
                                            "shared", "f32", "f32"),
    "walk_a_two_extra_tiles_s32_out": (lambda ncu: _H(ncu // 2 + 1, 17, 1, 64, 128, 1, act=R.ACT_RELU, ldx=64, ldy=128, yoff=0), "shared", None, "s32"),
    "walk_b_cout132_two_channel_tiles_four_extra_tiles": (lambda ncu: _H(ncu // 4 + 1, 17, 1, 64, 132, 1, ldx=64, **_PRELU, **_F32_OUT(132)),
                                                          "shared", None, "f32"),
    "walk_c_cin96_odd_chunks_one_workgroup_per_tile": (lambda ncu: _H(ncu // 2 + 1, 17, 1, 96, 128, 1, act=R.ACT_RELU, ldx=96, ldr=132, roff=4,
                                                                        **_F32_OUT(128)), "shared", "f32", "f32"),
    "walk_d_three_tile_rows_seam_rpw4_into_rpw1_s32_out": (lambda ncu: _H(ncu // 3 + 1, 33, 1, 64, 128, 1, act=R.ACT_RELU, ldx=64, ldy=128, yoff=0),
                                                           "shared", None, "s32"),
}
HALO_S32_NAMES = list(HALO_S32_CASES) + list(HALO_S32_WALK_CASES)


def halo_s32_case(name, ncu=256):
    if name in HALO_S32_CASES:
        return HALO_S32_CASES[name]
    mk, bias_kind, res_kind, out = HALO_S32_WALK_CASES[name]
    return mk(ncu), bias_kind, res_kind, out


@functools.lru_cache(maxsize=None)
def halo_s32_inputs(name, ncu=256):
    """-> geometry, (hi, lo) planes of x [B,H,W,ldx], w, bias | None, res: None | float32 [B,H,W,ldr] | its (hi, lo) planes, output format.
    R.s32_pack(hi, lo) is the device operand"""
    g, bias_kind, res_kind, out = halo_s32_case(name, ncu)
    x, w, bias, res = _operands(g, bias_kind, res_kind is not None, torch.Generator().manual_seed(3000 + HALO_S32_NAMES.index(name)))
    if res_kind == "s32":
        res = R.split(res)
    return g, R.split(x), w, bias, res, out


@functools.lru_cache(maxsize=None)
def halo_s32_expected(name, nsplit, ncu=256):
    """nsplit 3: the kernel's products; 0: the plain float64 convolution of hi + lo"""
    g, x, w, bias, res, _ = halo_s32_inputs(name, ncu)
    return R.halo_conv(x, w, g, nsplit, bias, res)


def halo_s32_rpw(g, y0):
    """rows per pixel-row group of waves in a tile at image row y0 (rows_per_wave of halo_s32_kernel)"""
    return (min(g["H"] - y0, 16) + 3) >> 2


def halo_s32_walk(g, ncu):
    """(grid, [[(image, y0, x0, channel tile) of every tile a workgroup walks, in order] per workgroup]) by launch_halo_s32's grid rule and
    the kernel's decode()"""
    tx, ty, nt = -(-g["W"] // 16), -(-g["H"] // 16), -(-g["Cout"] // 128)
    nwg = g["B"] * tx * ty * nt
    unit, grid = 8 * nt, nwg
    if nwg > ncu and ncu >= unit and (g["Cin"] // 32) % 2 == 0:
        grid = ncu // unit * unit
    q, r = divmod(nwg, 8)
    walks = []
    for wg in range(grid):
        tiles = []
        for orig in range(wg, nwg, grid):
            xcd = orig % 8
            logical = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + orig // 8
            n_tile, mt = logical % nt, logical // nt
            b, trem = divmod(mt, tx * ty)
            tiles.append((b, trem // tx * 16, trem % tx * 16, n_tile))
        walks.append(tiles)
    return grid, walks


def halo_s32_branches(g, res_kind, out, ncu=256):
    tx, ty, nt = -(-g["W"] // 16), -(-g["H"] // 16), -(-g["Cout"] // 128)
    grid, walks = halo_s32_walk(g, ncu)
    return dict(D=g["dil"], tiles_x=tx, tiles_y=ty, n_tiles=nt, workgroups=g["B"] * tx * ty * nt, grid=grid, chunks=g["Cin"] // 32,
                rpw=[halo_s32_rpw(g, 16 * t) for t in range(ty)], last_tile_cols=g["W"] - 16 * (tx - 1), empty_weight_rows=nt * 128 - g["Cout"],
                wide=out == "s32" and g["Cout"] % 8 == 0 and g["yoff"] % 8 == 0,
                narrow=out == "s32" and not (g["Cout"] % 8 == 0 and g["yoff"] % 8 == 0),
                max_tiles_per_workgroup=max(len(t) for t in walks),
                seam=any(halo_s32_rpw(g, a[1]) != halo_s32_rpw(g, b[1]) for t in walks for a, b in zip(t, t[1:])),
                one_channel_tile_per_workgroup=all(len({t[3] for t in tl}) == 1 for tl in walks))

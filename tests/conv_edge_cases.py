"""Inputs for the edge-shape tests of csrc/unet.hip (decoder conv and fused head) and of the split-K form of csrc/conv_gemm.hip, each named
for the shape and the branch it reaches.  tests/test_conv_edges_host.py proves the guards and the branch-reached claims on the CPU;
tests/test_gpu_unet_edges.py and tests/test_gpu_splitk_edges.py run them.

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

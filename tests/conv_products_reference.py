"""Plain float64 restatement of what csrc/unet.hip, the split-K form of csrc/conv_gemm.hip and the LDS-halo 3x3 kernels (csrc/conv3x3_halo.hip
with its fused x2 up-sampling, csrc/conv3x3_halo_s32.hip on pre-split S32 operands) compute: the sum of the very products the kernels form.
torch on the CPU only; reads nothing but its arguments.

Operand split, as pack_weights_kernel (weights) and split8 (activations) do it, in float32 with round-to-nearest-even:
    hi = bf16(v),  lo = bf16(v - float(hi))
and per 32-deep k-tile the kernels add   a_lo . w_hi,  a_hi . w_lo,  a_hi . w_hi   (nsplit = 3)  or  a_hi . w_hi  (nsplit = 1) into a float32
accumulator.  Every product of two bf16 values is exact in float32, so a float64 sum of them differs from the kernel's result by the
float32 accumulation alone.  nsplit = 0 stands for the unrounded operands (the plain float64 convolution).

The k-tiles come out of generators in the kernels' order (unet: tap outer, 32-channel chunk inner; conv_gemm and halo: chunk outer, tap inner), so
the same code serves the float64 sum (`total`), the float32 emulation of the kernels' accumulation (`accumulate_f32`) and the mutated
copies (`mutate`: the names of wrong rules, each one a defect the edge cases must be able to see; tests/test_conv_edges_host.py,
tests/test_halo_edges_host.py)."""
import torch

ACT_NONE, ACT_RELU, ACT_PRELU, ACT_SIGMOID = 0, 1, 2, 3
BK = 32
# wrong rules only the LDS-halo family can follow (tests/test_halo_edges_host.py names their cases)
HALO_MUTATIONS = ("left_column_wraps", "ups_half_pixel", "ups_weights_swapped", "residual_hi_only")
MUTATIONS = ("drop_cross_term", "nearest_rounds_up", "chunk_at_c1_from_a", "border_clamped", "split_starts_at_tap0", "last_split_dropped",
             "bias_of_image0", "residual_without_roff", "last_maximum") + HALO_MUTATIONS


def split(v):
    v = v.float()
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    return hi, lo


def _parts(v, nsplit):
    """v: float values, or the (hi, lo) planes of an operand that is already split (S32)"""
    if isinstance(v, tuple):
        hi, lo = v
        return {"v": hi.double() + lo.double()} if nsplit == 0 else {"hi": hi.double(), "lo": lo.double()}
    if nsplit == 0:
        return {"v": v.double()}
    hi, lo = split(v)
    return {"hi": hi.double(), "lo": lo.double()}


def _terms(nsplit, mutate=()):
    """(activation part, weight part) of each matrix instruction of a k-tile, in the kernels' order"""
    t = {0: (("v", "v"),), 1: (("hi", "hi"),), 3: (("lo", "hi"), ("hi", "lo"), ("hi", "hi"))}[nsplit]
    if "drop_cross_term" in mutate:
        t = tuple(p for p in t if p != ("hi", "lo"))
    return t


def total(tiles):
    s = None
    for t in tiles:
        s = t.clone() if s is None else s + t
    return s


def accumulate_f32(tiles):
    """the kernels' accumulator: one float32 rounding per matrix instruction (the 32-deep dot product itself taken exactly)"""
    acc = None
    for t in tiles:
        acc = t.float() if acc is None else (acc.double() + t).float()
    return acc


# ---- csrc/unet.hip -----------------------------------------------------------------------------------------------------------------------------
def unet_tiles(a, b, w, C1, C2, ups, nsplit, mutate=()):
    """a[B,Ha,Wa,lda], b[B,H,W,ldb] | None (float32 NHWC), w[Cout,C1+C2,3,3]: the [M, Cout] float64 product of every (tap, chunk, term) of
    the 3x3 / pad 1 convolution over the virtual input cat([nearest_up2(a[..., :C1]) | a[..., :C1], b[..., :C2]])"""
    B, Ha, Wa = a.shape[:3]
    H, W = (2 * Ha, 2 * Wa) if ups else (Ha, Wa)
    Ctot, Cout = C1 + C2, w.shape[0]
    wp = _parts(w.permute(0, 2, 3, 1).reshape(Cout, 9, Ctot), nsplit)
    ys, xs = torch.arange(H), torch.arange(W)
    for tap in range(9):
        yy, xx = ys + tap // 3 - 1, xs + tap % 3 - 1
        inside = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
        yc, xc = yy.clamp(0, H - 1), xx.clamp(0, W - 1)
        if "border_clamped" in mutate:
            inside = torch.ones_like(inside)
        ya, xa = yc, xc
        if ups:
            ya, xa = yc >> 1, xc >> 1
            if "nearest_rounds_up" in mutate:
                ya, xa = ((yc + 1) >> 1).clamp(max=Ha - 1), ((xc + 1) >> 1).clamp(max=Wa - 1)
        va = a[:, ya][:, :, xa]
        v = va[..., :C1]
        if C2:
            v = torch.cat([v, b[:, yc][:, :, xc][..., :C2]], -1)
            if "chunk_at_c1_from_a" in mutate:
                v = v.clone()
                v[..., C1:C1 + 8] = va[..., C1:C1 + 8]
        v = torch.where(inside[None, :, :, None], v, torch.zeros((), dtype=v.dtype))
        vp = _parts(v.reshape(-1, Ctot), nsplit)
        for c0 in range(0, Ctot, BK):
            for ta, tw in _terms(nsplit, mutate):
                yield vp[ta][:, c0:c0 + BK] @ wp[tw][:, tap, c0:c0 + BK].T


def unet_logits(a, b, w, bias, C1, C2, ups, nsplit, mutate=()):
    s = total(unet_tiles(a, b, w, C1, C2, ups, nsplit, mutate))
    return s if bias is None else s + bias.double()[None, :]


def unet_conv(a, b, w, bias, C1, C2, ups, nsplit, mutate=()):
    return unet_logits(a, b, w, bias, C1, C2, ups, nsplit, mutate).clamp(min=0)


def first_maximum(x, mutate=()):
    C = x.shape[-1]
    idx = torch.arange(C).expand_as(x)
    top = x == x.max(-1, keepdim=True).values
    if "last_maximum" in mutate:
        return torch.where(top, idx, torch.full_like(idx, -1)).max(-1).values
    return torch.where(top, idx, torch.full_like(idx, C)).min(-1).values


def head(logits, double_softmax, mutate=()):
    """logits[M, C] float64 -> label[M] (first maximum), score[M] (its probability after one or two softmaxes), p1[M, C] (first softmax)"""
    p1 = torch.softmax(logits, -1)
    p = torch.softmax(p1, -1) if double_softmax else p1
    return first_maximum(logits, mutate), p.max(-1).values, p1


def top2_gap(p1, duplicate_of=None):
    """difference of the two largest first-softmax probabilities of each pixel; a class that duplicates a lower one (duplicate_of[c] != c)
    is counted once.  inf where there is one class only"""
    C = p1.shape[-1]
    keep = [c for c in range(C) if duplicate_of is None or duplicate_of[c] == c]
    if len(keep) < 2:
        return torch.full(p1.shape[:-1], float("inf"), dtype=p1.dtype)
    t = p1[..., keep].topk(2, -1).values
    return t[..., 0] - t[..., 1]


# ---- csrc/conv_gemm.hip -------------------------------------------------------------------------------------------------------------------------
def conv_geometry(B, H, W, Cin, Cout, k=1, stride=1, pad=0, dil=1, act=ACT_NONE, alpha=0.0, ldx=None, xoff=0, ldy=None, yoff=0, bias_bstride=0,
                  ldr=0, roff=0):
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return dict(B=B, H=H, W=W, Cin=Cin, ldx=Cin if ldx is None else ldx, xoff=xoff, Ho=Ho, Wo=Wo, Cout=Cout, ldy=Cout if ldy is None else ldy, yoff=yoff,
                KH=k, KW=k, stride=stride, pad=pad, dil=dil, act=act, alpha=alpha, bias_bstride=bias_bstride, ldr=ldr, roff=roff, ups=0)


def n_ktiles(g):
    return g["KH"] * g["KW"] * g["Cin"] // BK


def conv_tile(x, w, g, nsplit, kt, mutate=()):
    """the term products [M, Cout] of k-tile kt of the general convolution; K order = 32-channel chunk outer, taps inner.
    x: float32 NHWC, or the (hi, lo) planes of an S32 operand"""
    taps = g["KH"] * g["KW"]
    chunk, tap = divmod(kt, taps)
    ky, kx = divmod(tap, g["KW"])
    iy = torch.arange(g["Ho"]) * g["stride"] - g["pad"] + ky * g["dil"]
    ix = torch.arange(g["Wo"]) * g["stride"] - g["pad"] + kx * g["dil"]
    inside = ((iy >= 0) & (iy < g["H"]))[:, None] & ((ix >= 0) & (ix < g["W"]))[None, :]
    c0 = g["xoff"] + chunk * BK
    if "border_clamped" in mutate:
        inside = torch.ones_like(inside)
    wraps = None
    if "left_column_wraps" in mutate:
        # a tap left or right of the row reads whatever pixel lies there in linear memory (zero only outside the whole tensor)
        lin = (torch.arange(g["B"])[:, None, None] * g["H"] + iy[None, :, None]) * g["W"] + ix[None, None, :]
        wraps = ((iy >= 0) & (iy < g["H"]))[None, :, None] & ~inside[None] & (lin >= 0) & (lin < g["B"] * g["H"] * g["W"])
        lin = lin.clamp(0, g["B"] * g["H"] * g["W"] - 1)

    def gather(t):
        v = t[:, iy.clamp(0, g["H"] - 1)][:, :, ix.clamp(0, g["W"] - 1)][..., c0:c0 + BK]
        v = torch.where(inside[None, :, :, None], v, torch.zeros((), dtype=v.dtype))
        if wraps is not None:
            v = torch.where(wraps[..., None], t.reshape(-1, t.shape[-1])[lin][..., c0:c0 + BK], v)
        return v.reshape(-1, BK)

    v = tuple(gather(t) for t in x) if isinstance(x, tuple) else gather(x)
    vp, wp = _parts(v, nsplit), _parts(w[:, chunk * BK:(chunk + 1) * BK, ky, kx], nsplit)
    return [vp[ta] @ wp[tw].T for ta, tw in _terms(nsplit, mutate)]


def conv_tiles(x, w, g, nsplit, kts=None, mutate=()):
    for kt in (range(n_ktiles(g)) if kts is None else kts):
        yield from conv_tile(x, w, g, nsplit, kt, mutate)


def splitk_ktiles(g, nk_per, mutate=()):
    """the k-tiles each launched split walks (conv_gemm_body<SK>: kt0 = split * nk_per, min(nk - kt0, nk_per) of them)"""
    nk, taps = n_ktiles(g), g["KH"] * g["KW"]
    out = []
    for kt0 in range(0, nk, nk_per):
        n = min(nk - kt0, nk_per)
        start = kt0 // taps * taps if "split_starts_at_tap0" in mutate else kt0
        out.append(list(range(start, start + n)))
    if "last_split_dropped" in mutate:
        out = out[:-1]
    return out


def conv_epilogue(s, g, bias, res, mutate=()):
    """s[M, Cout] float64 + bias row (m // HoWo) * bias_bstride + c + residual slice roff / ldr, then the activation"""
    M, Cout = s.shape
    if bias is not None:
        img = torch.arange(M) // (g["Ho"] * g["Wo"])
        if "bias_of_image0" in mutate:
            img = torch.zeros_like(img)
        s = s + bias.double().reshape(-1)[(img * g["bias_bstride"])[:, None] + torch.arange(Cout)[None, :]]
    if res is not None:
        roff = 0 if "residual_without_roff" in mutate else g["roff"]
        if isinstance(res, tuple):                # an S32 residual: float(hi) + float(lo)
            r = res[0].double() if "residual_hi_only" in mutate else res[0].double() + res[1].double()
        else:
            r = res.double()
        s = s + r.reshape(M, g["ldr"])[:, roff:roff + Cout]
    if g["act"] == ACT_RELU:
        s = s.clamp(min=0)
    elif g["act"] == ACT_PRELU:
        s = torch.where(s > 0, s, float(g["alpha"]) * s)
    elif g["act"] == ACT_SIGMOID:
        s = torch.sigmoid(s)
    return s


def conv(x, w, g, nsplit, bias=None, res=None, nk_per=0, mutate=()):
    """the general convolution; with nk_per the k-tiles are taken split by split (the same sum, unless a mutation moves a split)"""
    kts = None if not nk_per else [kt for sp in splitk_ktiles(g, nk_per, mutate) for kt in sp]
    return conv_epilogue(total(conv_tiles(x, w, g, nsplit, kts, mutate)), g, bias, res, mutate)


def conv_splitk_f32(x, w, g, nsplit, nk_per, bias=None, res=None):
    """float32 emulation of ape_conv_gemm_bf16_splitk: every split accumulates its k-tiles in float32, splitk_finish_kernel adds the splits
    in order, then bias, residual and activation, each with one float32 rounding"""
    v = None
    for sp in splitk_ktiles(g, nk_per):
        part = accumulate_f32(conv_tiles(x, w, g, nsplit, sp))
        v = part if v is None else v + part
    M, Cout = v.shape
    if bias is not None:
        img = torch.arange(M) // (g["Ho"] * g["Wo"])
        v = v + bias.float().reshape(-1)[(img * g["bias_bstride"])[:, None] + torch.arange(Cout)[None, :]]
    if res is not None:
        v = v + res.float().reshape(M, g["ldr"])[:, g["roff"]:g["roff"] + Cout]
    return conv_epilogue(v.double(), dict(g, bias_bstride=0), None, None).float()


# ---- csrc/conv3x3_halo.hip, csrc/conv3x3_halo_s32.hip ---------------------------------------------------------------------------------------------
def halo_geometry(B, H, W, Cin, Cout, dil=1, ups=0, **kw):
    """3x3 / stride 1 / pad == dil; H, W: the map the convolution runs on (with ups the x2 up-sampling of the [B, H/2, W/2, ldx] operand)"""
    return dict(conv_geometry(B, H, W, Cin, Cout, k=3, pad=dil, dil=dil, **kw), ups=ups)


def _ups_axis(n_lo, mutate=()):
    """source index pair and the weight of the second, per output coordinate of the x2 axis (ups_tbl of conv3x3_halo.hip), float32"""
    n = 2 * n_lo
    o = torch.arange(n, dtype=torch.float32)
    if "ups_half_pixel" in mutate:
        f = ((o + 0.5) * 0.5 - 0.5).clamp(min=0)
    else:
        f = (torch.tensor(float(n_lo - 1), dtype=torch.float32) / torch.tensor(float(n - 1), dtype=torch.float32)) * o
    i0 = f.to(torch.int64)
    l1 = f - i0.float()
    return i0, i0 + (i0 < n_lo - 1).long(), l1


def ups2x_f32(x, mutate=()):
    """x[B,hl,wl,C] float32 -> its bilinear x2 sample (align_corners=True) [B,2hl,2wl,C], float32 with one rounding per operation in the
    order of ups_lerp: o = ly0 (lx0 r0 + lx1 r1) + ly1 (lx0 r2 + lx1 r3)"""
    x = x.float()
    y0, y1, ly1 = _ups_axis(x.shape[1], mutate)
    x0, x1, lx1 = _ups_axis(x.shape[2], mutate)
    ly0, lx0 = 1.0 - ly1, 1.0 - lx1
    if "ups_weights_swapped" in mutate:
        lx0, lx1 = lx1, lx0
    ly0, ly1, lx0, lx1 = ly0[None, :, None, None], ly1[None, :, None, None], lx0[None, None, :, None], lx1[None, None, :, None]
    r0, r1, r2, r3 = x[:, y0][:, :, x0], x[:, y0][:, :, x1], x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return ly0 * (lx0 * r0 + lx1 * r1) + ly1 * (lx0 * r2 + lx1 * r3)


def halo_operand(x, g, mutate=()):
    """the tensor the nine taps read and the geometry that addresses it: with ups the float32 up-sampling of the channel slice"""
    if not g["ups"]:
        return x, g
    return ups2x_f32(x[..., g["xoff"]:g["xoff"] + g["Cin"]], mutate), dict(g, xoff=0, ldx=g["Cin"])


def halo_tiles(x, w, g, nsplit, mutate=()):
    """the k-tiles of a halo case in the kernels' order (32-channel chunk outer, tap inner); x: float32 NHWC or S32 (hi, lo) planes"""
    xv, gv = halo_operand(x, g, mutate)
    return conv_tiles(xv, w, gv, nsplit, None, mutate)


def halo_conv(x, w, g, nsplit, bias=None, res=None, mutate=()):
    return conv_epilogue(total(halo_tiles(x, w, g, nsplit, mutate)), g, bias, res, mutate)


def halo_conv_f32(x, w, g, nsplit, bias=None, res=None):
    """float32 emulation of the halo kernels: the k-tiles accumulate in float32 in their order, then bias, residual and activation"""
    v = accumulate_f32(halo_tiles(x, w, g, nsplit))
    M, Cout = v.shape
    if bias is not None:
        img = torch.arange(M) // (g["Ho"] * g["Wo"])
        v = v + bias.float().reshape(-1)[(img * g["bias_bstride"])[:, None] + torch.arange(Cout)[None, :]]
    if res is not None:
        r = (res[0].float() + res[1].float()) if isinstance(res, tuple) else res.float()
        v = v + r.reshape(M, g["ldr"])[:, g["roff"]:g["roff"] + Cout]
    return conv_epilogue(v.double(), dict(g, bias_bstride=0), None, None).float()


# ---- the S32 layout (engine.S32): per pixel and 32-channel group 128 B = 32 bf16 hi | 32 bf16 lo ------------------------------------------------------
def s32_pack(hi, lo):
    """(hi, lo)[..., C] of bf16-representable values -> the float32-typed buffer [..., C] that holds their S32 bytes"""
    C = hi.shape[-1]
    bits = [t.to(torch.bfloat16).view(torch.int16).reshape(t.shape[:-1] + (C // BK, BK)) for t in (hi, lo)]
    return torch.cat(bits, -1).reshape(hi.shape[:-1] + (2 * C,)).contiguous().view(torch.float32)


def s32_unpack(t):
    """the float32-typed S32 buffer [..., C] -> its (hi, lo) planes [..., C] as float32"""
    C = t.shape[-1]
    b = t.contiguous().view(torch.int16).reshape(t.shape[:-1] + (C // BK, 2, BK))
    return tuple(b[..., k, :].reshape(t.shape).contiguous().view(torch.bfloat16).float() for k in (0, 1))


def s32_from_f32(v):
    return s32_pack(*split(v))

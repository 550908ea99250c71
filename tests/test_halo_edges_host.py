"""CPU proofs about the LDS-halo cases of tests/conv_edge_cases.py (HALO_CASES: csrc/conv3x3_halo.hip; HALO_S32_CASES and the walk cases:
csrc/conv3x3_halo_s32.hip) and their restatement in tests/conv_products_reference.py, in the manner of tests/test_conv_edges_host.py: the
restatement of the unrounded operands is the plain float64 convolution (of the float64 bilinear sample for the fused up-sampling); every
case passes the kernels' own argument checks, holds NaN where the kernel must not read and reaches the branches its row of the branch
table names; the same products accumulated in float32 in the kernels' order stay within half the GPU bar; each wrong rule moves the result
by at least ten times the GPU bar on the cases named for it.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_edge_cases as EC
import conv_products_reference as R

HALO = list(EC.HALO_CASES)
S32 = list(EC.HALO_S32_CASES)
WALK = list(EC.HALO_S32_WALK_CASES)
NCUS = (256, 304)
S32_RUNS = [(n, 256) for n in S32] + [(n, ncu) for n in WALK for ncu in NCUS]


def _moved(x, y):
    return float(torch.nan_to_num((x - y).abs(), nan=float("inf")).max())


def _scale(ref):
    return max(1.0, float(ref.abs().max()))


def _nhwc_conv(x, w, dil):
    return F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 1, dil, dil).permute(0, 2, 3, 1).reshape(-1, w.shape[0])


# ---- the restatement of unrounded operands is the plain convolution -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HALO)
def test_halo_restatement_unrounded_equals_conv2d(name):
    g, x, w, bias, res = EC.halo_inputs(name)
    xs = x[..., g["xoff"]:g["xoff"] + g["Cin"]]
    got = R.total(R.halo_tiles(x, w, g, 0))
    if not g["ups"]:
        want = _nhwc_conv(xs, w, g["dil"])
        assert got.shape == want.shape and _moved(got, want) <= 1e-12 * _scale(want)
        return
    up = F.interpolate(xs.permute(0, 3, 1, 2).double(), size=(g["H"], g["W"]), mode="bilinear", align_corners=True)
    want = F.conv2d(up, w.double(), None, 1, 1).permute(0, 2, 3, 1).reshape(-1, g["Cout"])
    # float32 interpolation rounding: a source coordinate (< 16 on these maps) carries the roundings of s and of s * o, at most 2 ulp = 2^-19, which
    # moves a sample by that times the span of its two neighbours (<= 2 max|x|), on each axis: 2^-17 max|x|; the seven roundings of the blend add
    # 7 * 2^-24 max|x|.  Together below 2^-16 max|x| per sample, which the convolution scales by at most the largest sum of |w| of a channel.
    assert max(g["H"], g["W"]) // 2 <= 16
    bound = 2.0 ** -16 * float(xs.abs().max()) * float(w.double().abs().sum((1, 2, 3)).max())
    assert got.shape == want.shape and _moved(got, want) <= bound
    # and the sample itself, against the float64 one
    assert _moved(R.ups2x_f32(xs).double(), up.permute(0, 2, 3, 1)) <= 2.0 ** -16 * float(xs.abs().max())


@pytest.mark.parametrize("name,ncu", S32_RUNS)
def test_halo_s32_restatement_unrounded_equals_conv2d(name, ncu):
    g, (hi, lo), w, bias, res, out = EC.halo_s32_inputs(name, ncu)
    xs = (hi.double() + lo.double())[..., g["xoff"]:g["xoff"] + g["Cin"]]
    want = _nhwc_conv(xs, w, g["dil"])
    got = R.total(R.halo_tiles((hi, lo), w, g, 0))
    assert got.shape == want.shape and _moved(got, want) <= 1e-12 * _scale(want)


def test_halo_epilogue_written_out_per_element():
    """bias row, residual slice (S32: hi + lo) and activation of R.halo_conv on one case of each kind"""
    import math
    for kind, name in (("f32", "d2_n128_3x13x17_second_tile_column_of_one_six_workgroups_act_none"),
                       ("f32", "d4_n64_2x32x48_cin64_cout64_null_bias_vector_residual"),
                       ("s32", "d2_2x12x16_rpw3_every_tile_cin96_xoff32_s32_narrow_by_cout132_s32_residual"),
                       ("s32", "d1_1x13x16_rpw4_cin160_s32_narrow_by_yoff4_f32_residual_sigmoid")):
        g, x, w, bias, res = (EC.halo_inputs(name) if kind == "f32" else EC.halo_s32_inputs(name)[:5])
        pre, full = R.total(R.halo_tiles(x, w, g, 0)), R.halo_conv(x, w, g, 0, bias, res)
        M = pre.shape[0]
        for m, ch in ((0, 0), (M - 1, g["Cout"] - 1), (M // 2, g["Cout"] // 2)):
            v = float(pre[m, ch])
            if bias is not None:
                v += float(bias[(m // (g["H"] * g["W"])) * g["bias_bstride"] + ch])
            if res is not None:
                at = m * g["ldr"] + g["roff"] + ch
                v += float(res[0].reshape(-1)[at]) + float(res[1].reshape(-1)[at]) if isinstance(res, tuple) else float(res.reshape(-1)[at])
            v = {R.ACT_NONE: v, R.ACT_RELU: max(v, 0.0), R.ACT_PRELU: v if v > 0 else float(g["alpha"]) * v, R.ACT_SIGMOID: 1.0 / (1.0 + math.exp(-v))}[g["act"]]
            assert abs(float(full[m, ch]) - v) <= 1e-12 * max(1.0, abs(v))


def test_s32_layout_packer():
    """per pixel and 32-channel group 128 B = 32 bf16 hi | 32 bf16 lo (engine.S32); hi + lo is exact in float32"""
    v = torch.randn(2, 3, 96, generator=torch.Generator().manual_seed(1))
    v[..., 32:64] = EC.NAN
    hi, lo = R.split(v)
    t = R.s32_from_f32(v)
    assert t.dtype == torch.float32 and t.shape == v.shape
    raw = t.view(torch.int16).reshape(2, 3, 3, 64)
    want_hi = hi.to(torch.bfloat16).view(torch.int16).reshape(2, 3, 3, 32)
    assert torch.equal(raw[..., :32], want_hi) and torch.equal(raw[..., 32:], lo.to(torch.bfloat16).view(torch.int16).reshape(2, 3, 3, 32))
    uh, ul = R.s32_unpack(t)
    keep = ~torch.isnan(v)
    assert torch.equal(uh[keep], hi[keep]) and torch.equal(ul[keep], lo[keep])
    assert torch.isnan(uh[~keep]).all() and torch.isnan(ul[~keep]).all()          # an unread group: every bf16 a NaN pattern
    assert torch.equal((uh + ul)[keep].double(), uh[keep].double() + ul[keep].double())
    s = R.s32_unpack(torch.full((4, 32), 0.0).view(torch.int16).fill_(-15550).view(torch.float32))     # 0xC342
    assert (s[0] == EC.S32_SENTINEL).all() and (s[1] == EC.S32_SENTINEL).all()


# ---- guards ---------------------------------------------------------------------------------------------------------------------------------------
def _halo_supported(g):
    """ape_conv3x3_halo_supported of csrc/conv3x3_halo.hip"""
    return (g["KH"] == 3 and g["KW"] == 3 and g["stride"] == 1 and g["pad"] == g["dil"] and g["dil"] in (1, 2, 4) and g["Cin"] % 32 == 0
            and g["Cin"] >= 32 and g["H"] == g["Ho"] and g["W"] == g["Wo"])


def _halo_entry_ok(g, with_res):
    """the argument checks of ape_conv3x3_halo_bf16"""
    if not _halo_supported(g) or g["B"] < 0 or g["H"] < 1 or g["W"] < 1 or g["Cout"] < 1:
        return False
    if g["ldx"] % 4 or g["xoff"] % 4 or g["xoff"] + g["Cin"] > g["ldx"] or g["yoff"] + g["Cout"] > g["ldy"]:
        return False
    if with_res and g["roff"] + g["Cout"] > g["ldr"]:
        return False
    if not 0 <= g["act"] <= 3 or g["ups"] not in (0, 1):
        return False
    if g["B"] * g["H"] * g["W"] * g["ldx"] >= 1 << 31 or g["Cout"] * 9 * g["Cin"] >= 1 << 31:
        return False
    return not g["ups"] or (g["dil"] == 1 and g["H"] % 2 == 0 and g["W"] % 2 == 0)


def _halo_s32_supported(g):
    """halo_s32_supported of csrc/conv3x3_halo_s32.hip"""
    if g["KH"] != 3 or g["KW"] != 3 or g["stride"] != 1 or g["pad"] != g["dil"] or g["dil"] not in (1, 2, 4) or g["ups"] != 0:
        return False
    if g["B"] < 0 or g["H"] < 1 or g["W"] < 1 or g["Ho"] != g["H"] or g["Wo"] != g["W"]:
        return False
    if g["Cin"] < 32 or g["Cin"] % 32 or g["ldx"] % 32 or g["xoff"] % 32 or g["xoff"] + g["Cin"] > g["ldx"]:
        return False
    if g["Cout"] < 128 or g["Cout"] % 4 or g["yoff"] + g["Cout"] > g["ldy"] or g["ldy"] % 4 or g["yoff"] % 4:
        return False
    if not 0 <= g["act"] <= 3:
        return False
    return g["B"] * g["H"] * g["W"] * g["ldx"] * 4 < 1 << 31 and 128 * 9 * g["Cin"] * 4 < 1 << 31


def _halo_s32_entry_ok(g, res_kind, out):
    """the argument checks of ape_conv3x3_halo_s32"""
    if not _halo_s32_supported(g) or (out == "s32" and g["ldy"] % 32):
        return False
    if res_kind and (g["roff"] + g["Cout"] > g["ldr"] or g["ldr"] % 4 or g["roff"] % 4 or (res_kind == "s32" and g["ldr"] % 32)):
        return False
    return True


def _check_planted(g, x, bias, res, expected):
    """NaN sits where it was planted and nowhere else; the expected output is finite and cannot equal a sentinel"""
    rd = torch.zeros(g["ldx"], dtype=torch.bool)
    rd[g["xoff"]:g["xoff"] + g["Cin"]] = True
    for t in (x if isinstance(x, tuple) else (x,)):
        assert torch.isnan(t[..., ~rd]).all()
        assert torch.isfinite(t[..., rd]).all() and int(torch.isnan(t).sum()) == t[..., 0].numel() * (g["ldx"] - g["Cin"])
    if res is not None:
        rr = torch.zeros(g["ldr"], dtype=torch.bool)
        rr[g["roff"]:g["roff"] + g["Cout"]] = True
        assert g["ldr"] > g["Cout"]
        for t in (res if isinstance(res, tuple) else (res,)):
            assert tuple(t.shape) == (g["B"], g["H"], g["W"], g["ldr"]) and torch.isnan(t[..., ~rr]).all() and torch.isfinite(t[..., rr]).all()
    if g["bias_bstride"]:
        assert bias is not None and g["bias_bstride"] > g["Cout"]
        b2 = bias.reshape(g["B"], g["bias_bstride"])
        assert torch.isnan(b2[:, g["Cout"]:]).all() and torch.isfinite(b2[:, :g["Cout"]]).all()
    elif bias is not None:
        assert bias.numel() == g["Cout"] and torch.isfinite(bias).all()
    for e in expected:
        assert torch.isfinite(e).all() and float(e.abs().max()) < 100.0          # (the sentinels are -777 and -194)
    assert g["B"] * g["H"] * g["W"] <= 4000 and 9 * g["Cin"] // 32 <= 45
    assert g["ldy"] > g["Cout"] or g["yoff"] == 0


@pytest.mark.parametrize("name", HALO)
def test_halo_case_guards(name):
    g, x, w, bias, res = EC.halo_inputs(name)
    assert _halo_entry_ok(g, res is not None)
    assert (res is not None) == EC.HALO_CASES[name][2] and (bias is None) == (EC.HALO_CASES[name][1] is None)
    hl, wl = (g["H"] // 2, g["W"] // 2) if g["ups"] else (g["H"], g["W"])
    assert tuple(x.shape) == (g["B"], hl, wl, g["ldx"]) and g["ldx"] > g["Cin"] and g["ldy"] > g["yoff"] + g["Cout"] and g["yoff"] > 0
    _check_planted(g, x, bias, res, [EC.halo_expected(name, s) for s in (0, 1, 3)])


@pytest.mark.parametrize("name,ncu", S32_RUNS)
def test_halo_s32_case_guards(name, ncu):
    g, x, w, bias, res, out = EC.halo_s32_inputs(name, ncu)
    res_kind = EC.halo_s32_case(name, ncu)[2]
    assert _halo_s32_entry_ok(g, res_kind, out)
    assert isinstance(res, tuple) == (res_kind == "s32") and (res is None) == (res_kind is None)
    if g["bias_bstride"]:
        assert g["bias_bstride"] % 4 == 0                                   # read as float4; the ABI does not check it
    if g["xoff"]:
        assert g["xoff"] in (32, 64) and g["ldx"] >= g["xoff"] + g["Cin"]
    _check_planted(g, x, bias, res, [EC.halo_s32_expected(name, s, ncu) for s in (0, 3)])
    # the S32 operand really carries NaN patterns in every bf16 of an unread group
    hi, lo = R.s32_unpack(R.s32_pack(*x))
    rd = torch.zeros(g["ldx"], dtype=torch.bool)
    rd[g["xoff"]:g["xoff"] + g["Cin"]] = True
    assert torch.isnan(hi[..., ~rd]).all() and torch.isnan(lo[..., ~rd]).all() and torch.equal(hi[..., rd], x[0][..., rd])


# ---- the branches named are reached -----------------------------------------------------------------------------------------------------------------
# case -> what conv3x3_halo_kernel meets on it (a subset of EC.halo_branches)
HALO_BRANCHES = {
    "d1_n64_1x1x1_cin32_one_chunk_cout4_null_bias_act_none": dict(D=1, BNH=64, workgroups=1, last_tile_rows=1, last_tile_cols=1, chunks=1, vec_ok=True,
                                                                  scalar=False, empty_weight_rows=60),
    "d4_n64_1x3x5_off_centre_taps_outside_cout13_scalar_nvalid1_sigmoid": dict(D=4, BNH=64, last_tile_rows=3, last_tile_cols=5, chunks=2, vec_ok=True,
                                                                               nvalid_last=1, scalar=True),
    "d2_n128_1x3x5_cin96_cout65_63_empty_rows_scalar_by_ldy": dict(D=2, BNH=128, chunks=3, empty_weight_rows=63, vec_ok=False, a_double=True),
    "d1_n128_2x1x33_cout129_second_channel_tile_of_one_scalar_by_yoff_per_image_bias": dict(D=1, BNH=128, tiles_x=3, n_tiles=2, empty_weight_rows=127,
                                                                                            last_tile_cols=1, last_tile_rows=1, vec_ok=False),
    "d2_n64_1x9x1_cin32_cout64_scalar_by_roff_null_bias": dict(D=2, BNH=64, last_tile_rows=9, last_tile_cols=1, chunks=1, vec_ok=False),
    "d1_n128_1x16x16_one_full_tile_cin96_cout128_vector_residual_slice": dict(D=1, BNH=128, workgroups=1, last_tile_rows=16, last_tile_cols=16, chunks=3,
                                                                              vec_ok=True, scalar=False, empty_weight_rows=0),
    "d4_n128_1x17x16_second_tile_row_of_one_cout200_sigmoid": dict(D=4, BNH=128, tiles_y=2, last_tile_rows=1, n_tiles=2, empty_weight_rows=56, chunks=1),
    "d2_n128_3x13x17_second_tile_column_of_one_six_workgroups_act_none": dict(D=2, BNH=128, tiles_x=2, last_tile_cols=1, workgroups=6, vec_ok=True),
    "d1_n64_3x13x17_cin96_single_buffer_refill_odd_chunks": dict(D=1, BNH=64, a_double=False, chunks=3, workgroups=6),
    "d4_n64_2x32x48_cin64_cout64_null_bias_vector_residual": dict(D=4, BNH=64, tiles_x=3, tiles_y=2, workgroups=12, vec_ok=True, scalar=False),
    "ups_n64_1x1x1_to_2x2_cin32_cout64": dict(ups=1, BNH=64, last_tile_rows=2, last_tile_cols=2, chunks=1),
    "ups_n128_2x5x7_to_10x14_xoff8_cout128_vector_residual": dict(ups=1, BNH=128, last_tile_rows=10, last_tile_cols=14, chunks=2, vec_ok=True),
    "ups_n64_1x8x8_to_16x16_cin96_cout4_per_image_bias": dict(ups=1, BNH=64, last_tile_rows=16, last_tile_cols=16, chunks=3),
    "ups_n128_3x9x12_to_18x24_cout65_null_bias_sigmoid": dict(ups=1, BNH=128, tiles_x=2, tiles_y=2, last_tile_rows=2, last_tile_cols=8, workgroups=12,
                                                              nvalid_last=1),
}
# case -> (facts that hold for every ncu, {ncu: facts}) of halo_s32_kernel
HALO_S32_BRANCHES = {
    "d1_1x1x1_cin32_xoff32_f32_out_null_bias_act_none": (dict(D=1, rpw=[1], chunks=1, workgroups=1, wide=False, narrow=False), {}),
    "d4_1x3x5_cin64_xoff64_s32_wide_store": (dict(D=4, rpw=[1], chunks=2, wide=True, n_tiles=2, empty_weight_rows=120), {}),
    "d2_2x12x16_rpw3_every_tile_cin96_xoff32_s32_narrow_by_cout132_s32_residual": (dict(D=2, rpw=[3], chunks=3, narrow=True, empty_weight_rows=124), {}),
    "d1_1x13x16_rpw4_cin160_s32_narrow_by_yoff4_f32_residual_sigmoid": (dict(D=1, rpw=[4], chunks=5, narrow=True, empty_weight_rows=0), {}),
    "d2_1x17x9_last_tile_row_rpw1_f32_residual_per_image_bias": (dict(D=2, rpw=[4, 1], chunks=2, last_tile_cols=9), {}),
    "d4_1x21x33_last_tile_row_rpw2_cout200_two_channel_tiles_sigmoid": (dict(D=4, rpw=[4, 2], chunks=1, tiles_x=3, last_tile_cols=1, n_tiles=2), {}),
    "d1_2x28x17_last_tile_row_rpw3_beside_one_column_tile_s32_wide_s32_residual": (dict(D=1, rpw=[4, 3], chunks=3, tiles_x=2, last_tile_cols=1, wide=True), {}),
    # grid = ncu, two (four) tiles more than that: workgroups 0, 1 (0..3) walk two tiles.  Two tile rows per image and an even tile stride
    # (grid / 8 / n_tiles): both tiles of such a workgroup lie in the SAME tile row -- no rpw seam, except case b on 304 compute units (stride 19)
    "walk_a_two_extra_tiles_f32_residual": (dict(rpw=[4, 1], chunks=2, max_tiles_per_workgroup=2, one_channel_tile_per_workgroup=True),
                                            {256: dict(grid=256, workgroups=258, seam=False), 304: dict(grid=304, workgroups=306, seam=False)}),
    "walk_a_two_extra_tiles_s32_out": (dict(rpw=[4, 1], chunks=2, max_tiles_per_workgroup=2, wide=True),
                                       {256: dict(grid=256, workgroups=258, seam=False), 304: dict(grid=304, workgroups=306, seam=False)}),
    "walk_b_cout132_two_channel_tiles_four_extra_tiles": (dict(rpw=[4, 1], n_tiles=2, max_tiles_per_workgroup=2, one_channel_tile_per_workgroup=True),
                                                          {256: dict(grid=256, workgroups=260, seam=False), 304: dict(grid=304, workgroups=308, seam=True)}),
    "walk_c_cin96_odd_chunks_one_workgroup_per_tile": (dict(rpw=[4, 1], chunks=3, max_tiles_per_workgroup=1, seam=False),
                                                       {256: dict(grid=258), 304: dict(grid=306)}),
    # three tile rows per image: the stride of 32 (38) tiles moves a workgroup two tile rows on, rpw 4 -> rpw 1
    "walk_d_three_tile_rows_seam_rpw4_into_rpw1_s32_out": (dict(rpw=[4, 4, 1], chunks=2, max_tiles_per_workgroup=2, seam=True, wide=True),
                                                           {256: dict(grid=256, workgroups=258), 304: dict(grid=304, workgroups=306)}),
}


def _holds(facts, br, what):
    for k, v in facts.items():
        assert br[k] == v, (what, k, br[k], v)


@pytest.mark.parametrize("name", HALO)
def test_halo_cases_reach_the_branches_they_are_named_for(name):
    g, bias_kind, with_res = EC.HALO_CASES[name]
    _holds(HALO_BRANCHES[name], EC.halo_branches(g, with_res), name)


@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("name", S32 + WALK)
def test_halo_s32_cases_reach_the_branches_they_are_named_for(name, ncu):
    g, bias_kind, res_kind, out = EC.halo_s32_case(name, ncu)
    br = EC.halo_s32_branches(g, res_kind, out, ncu)
    always, per_ncu = HALO_S32_BRANCHES[name]
    _holds(always, br, name)
    _holds(per_ncu.get(ncu, {}), br, (name, ncu))
    if name in EC.HALO_S32_WALK_CASES:
        assert ncu % 16 == 0 and g["B"] * g["H"] * g["W"] <= 4000
        grid, walks = EC.halo_s32_walk(g, ncu)
        seen = sorted(t for tl in walks for t in tl)                       # every tile exactly once
        assert seen == sorted((b, y, 0, n) for b in range(g["B"]) for y in range(0, g["H"], 16) for n in range(br["n_tiles"]))
        if br["seam"] and name.startswith("walk_d"):
            first, second = walks[0]
            assert (EC.halo_s32_rpw(g, first[1]), EC.halo_s32_rpw(g, second[1])) == (4, 1)
            assert [EC.halo_s32_rpw(g, t[1]) for t in walks[1]] == [4, 1]


def test_halo_case_tables_cover_what_the_kernels_can_meet():
    hb = {n: EC.halo_branches(EC.HALO_CASES[n][0], EC.HALO_CASES[n][2]) for n in HALO}
    plain = [n for n in HALO if not hb[n]["ups"]]
    G = lambda n: EC.HALO_CASES[n][0]  # noqa: E731
    assert {(hb[n]["D"], hb[n]["BNH"]) for n in plain} == {(d, b) for d in (1, 2, 4) for b in (64, 128)}
    assert {(G(n)["B"], G(n)["H"], G(n)["W"]) for n in plain} == {(1, 1, 1), (1, 3, 5), (2, 1, 33), (1, 9, 1), (1, 16, 16), (1, 17, 16), (3, 13, 17), (2, 32, 48)}
    assert {(G(n)["dil"]) for n in plain if (G(n)["H"], G(n)["W"]) == (3, 5)} == {2, 4}
    assert {G(n)["Cin"] for n in plain} == {32, 64, 96} and {G(n)["Cout"] for n in plain} == {4, 13, 64, 65, 128, 129, 200}
    # the epilogue: the vector path with a residual slice; the scalar path by ldy, by yoff, by roff, by nvalid < 4
    assert any(hb[n]["vec_ok"] and not hb[n]["scalar"] and EC.HALO_CASES[n][2] and G(n)["ldr"] > G(n)["roff"] + G(n)["Cout"] and G(n)["roff"] for n in plain)
    assert any(G(n)["ldy"] % 4 and not G(n)["yoff"] % 4 for n in plain) and any(G(n)["yoff"] % 4 and not G(n)["ldy"] % 4 for n in plain)
    assert any(EC.HALO_CASES[n][2] and G(n)["roff"] % 4 and not (G(n)["ldy"] % 4 or G(n)["yoff"] % 4 or G(n)["ldr"] % 4) for n in plain)
    assert any(hb[n]["vec_ok"] and hb[n]["nvalid_last"] < 4 for n in plain)
    assert {EC.HALO_CASES[n][1] for n in plain} == {None, "shared", "per_image"} and {G(n)["act"] for n in plain} == {0, 1, 2, 3}
    assert {G(n)["dil"] for n in plain if G(n)["xoff"] > 0 and G(n)["ldx"] > G(n)["xoff"] + G(n)["Cin"]} == {1, 2, 4}
    ups = [n for n in HALO if hb[n]["ups"]]
    assert {(G(n)["B"], G(n)["H"] // 2, G(n)["W"] // 2) for n in ups} == {(1, 1, 1), (2, 5, 7), (1, 8, 8), (3, 9, 12)}
    assert {hb[n]["BNH"] for n in ups} == {64, 128} and any(G(n)["xoff"] > 0 for n in ups) and all(G(n)["dil"] == 1 for n in ups)
    # halo_s32
    S = lambda n: EC.halo_s32_case(n)[0]  # noqa: E731
    sb = {n: EC.halo_s32_branches(S(n), EC.halo_s32_case(n)[2], EC.halo_s32_case(n)[3]) for n in S32 + WALK}
    assert {S(n)["dil"] for n in S32} == {1, 2, 4} and {S(n)["dil"] for n in S32 if S(n)["xoff"] in (32, 64) and S(n)["ldx"] >= S(n)["xoff"] + S(n)["Cin"]} == {1, 2, 4}
    assert {(S(n)["B"], S(n)["H"], S(n)["W"]) for n in S32} == {(1, 1, 1), (1, 3, 5), (2, 12, 16), (1, 13, 16), (1, 17, 9), (1, 21, 33), (2, 28, 17)}
    assert {S(n)["Cin"] for n in S32} == {32, 64, 96, 160} and {sb[n]["rpw"][-1] for n in S32} == {1, 2, 3, 4}
    assert {(S(n)["Cout"], S(n)["yoff"], S(n)["ldy"]) for n in S32 if EC.halo_s32_case(n)[3] == "s32"} == {(136, 8, 160), (132, 0, 160), (128, 4, 160)}
    assert all((S(n)["yoff"], S(n)["ldy"]) == (4, S(n)["Cout"] + 12) for n in S32 if EC.halo_s32_case(n)[3] == "f32")
    assert {EC.halo_s32_case(n)[2] for n in S32} == {None, "f32", "s32"} and {EC.halo_s32_case(n)[1] for n in S32} == {None, "shared", "per_image"}
    assert all(S(n)["roff"] == 4 and S(n)["ldr"] > 4 + S(n)["Cout"] for n in S32 if EC.halo_s32_case(n)[2])
    assert {S(n)["act"] for n in S32} == {0, 1, 2, 3}
    assert set(HALO_BRANCHES) == set(HALO) and set(HALO_S32_BRANCHES) == set(S32 + WALK)


# ---- the same products accumulated in float32, in the kernels' order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", HALO)
def test_halo_float32_accumulation_stays_within_half_the_bar(name, nsplit):
    g, x, w, bias, res = EC.halo_inputs(name)
    ref = EC.halo_expected(name, nsplit)
    r = _moved(R.halo_conv_f32(x, w, g, nsplit, bias, res).double(), ref) / _scale(ref)
    assert r <= 0.5 * EC.BAR, (name, nsplit, r)


@pytest.mark.parametrize("name,ncu", S32_RUNS)
def test_halo_s32_float32_accumulation_stays_within_half_the_bar(name, ncu):
    g, x, w, bias, res, out = EC.halo_s32_inputs(name, ncu)
    ref = EC.halo_s32_expected(name, 3, ncu)
    r = _moved(R.halo_conv_f32(x, w, g, 3, bias, res).double(), ref) / _scale(ref)
    assert r <= 0.5 * EC.BAR, (name, r)


# ---- mutations: each wrong rule moves the result by at least 10 x the GPU bar on the cases named for it ------------------------------------------------
def _mutated(kind, name, nsplit, mutation):
    if kind == "halo":
        g, x, w, bias, res = EC.halo_inputs(name)
        ref = EC.halo_expected(name, nsplit)
    else:
        g, x, w, bias, res, _ = EC.halo_s32_inputs(name)
        ref = EC.halo_s32_expected(name, nsplit)
    return _moved(R.halo_conv(x, w, g, nsplit, bias, res, (mutation,)), ref) / _scale(ref)


_UPS_MOVING = [n for n in HALO if EC.HALO_CASES[n][0]["ups"] and EC.HALO_CASES[n][0]["H"] > 2]       # (one source pixel has one sample only)
HALO_MUTATION_CASES = {
    "drop_cross_term": [("halo", n, 3) for n in HALO] + [("s32", n, 3) for n in S32 + WALK],
    "border_clamped": [("halo", n, s) for n in HALO for s in (1, 3)] + [("s32", n, 3) for n in S32],
    "left_column_wraps": [("halo", n, s) for n in ("d1_n128_1x16x16_one_full_tile_cin96_cout128_vector_residual_slice",
                                                   "d2_n128_3x13x17_second_tile_column_of_one_six_workgroups_act_none",
                                                   "d4_n64_2x32x48_cin64_cout64_null_bias_vector_residual",
                                                   "ups_n128_2x5x7_to_10x14_xoff8_cout128_vector_residual") for s in (1, 3)]
                         + [("s32", n, 3) for n in ("d2_2x12x16_rpw3_every_tile_cin96_xoff32_s32_narrow_by_cout132_s32_residual",
                                                    "d2_1x17x9_last_tile_row_rpw1_f32_residual_per_image_bias",
                                                    "d1_2x28x17_last_tile_row_rpw3_beside_one_column_tile_s32_wide_s32_residual")],
    "ups_half_pixel": [("halo", n, s) for n in _UPS_MOVING for s in (1, 3)],
    "ups_weights_swapped": [("halo", n, s) for n in _UPS_MOVING for s in (1, 3)],
    "residual_hi_only": [("s32", n, 3) for n in S32 if EC.halo_s32_case(n)[2] == "s32"],
    "bias_of_image0": [("halo", n, s) for n in HALO if EC.HALO_CASES[n][1] == "per_image" and EC.HALO_CASES[n][0]["B"] > 1 for s in (1, 3)]
                      + [("s32", n, 3) for n in S32 if EC.halo_s32_case(n)[1] == "per_image" and EC.halo_s32_case(n)[0]["B"] > 1],
    "residual_without_roff": [("halo", n, s) for n in HALO if EC.HALO_CASES[n][2] for s in (1, 3)] + [("s32", n, 3) for n in S32 if EC.halo_s32_case(n)[2]],
}


@pytest.mark.parametrize("mutation", list(HALO_MUTATION_CASES))
def test_halo_mutation_moves_the_result(mutation):
    assert mutation in R.MUTATIONS
    assert len({c[1] for c in HALO_MUTATION_CASES[mutation]}) >= 2
    for kind, name, nsplit in HALO_MUTATION_CASES[mutation]:
        r = _mutated(kind, name, nsplit, mutation)
        assert r >= 10 * EC.BAR, (mutation, name, nsplit, r)


def test_every_halo_mutation_has_a_case():
    assert set(R.HALO_MUTATIONS) <= set(HALO_MUTATION_CASES)
    assert len(_UPS_MOVING) == 3

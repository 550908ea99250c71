"""CPU proofs about the inputs of tests/conv_edge_cases.py and the restatement tests/conv_products_reference.py: the restatement of the
unrounded operands is the plain float64 convolution; every case holds its guards (the kernels' `supported()` geometry, sentinels in place,
the split-K cases split, the head cases stay out of the label comparison's exclusion band) and reaches the branch it is named for; the
same products accumulated in float32 in the kernels' order stay within half the GPU bar; and each wrong rule, carried by a mutated copy of
the restatement, moves the result by at least ten times the GPU bar on the cases named for it.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_edge_cases as EC
import conv_products_reference as R

UNET_NAMES = list(EC.UNET_CONV_CASES) + list(EC.UNET_HEAD_CASES)
ALWAYS = {"lanes_past_M", "wide_a"}
# case -> branches of unet_conv3x3_kernel it is named for
UNET_BRANCHES = {
    "nc4np4_ups_1x2x2_c16+0_o64": {"group_past_M", "half_empty_kstep"},
    "nc4np4_ups_2x10x14_c16+16_o80": {"kstep_holds_A_and_B", "channel_groups_past_Cout", "more_than_one_workgroup", "group_straddles_image", "wide_b"},
    "nc4np4_ups_3x14x18_c48+16_o128": {"kstep_holds_A_and_B", "more_than_one_workgroup"},
    "nc4np4_full_1x5x7_c32+48_o64": {"group_straddles_row_odd_W", "half_empty_kstep", "wide_b"},
    "nc4np4_full_2x1x33_c80+0_o80": {"group_straddles_row_odd_W", "group_straddles_image", "half_empty_kstep", "channel_groups_past_Cout"},
    "nc4np4_full_1x9x1_c64+64_o128": {"group_straddles_row_odd_W", "group_past_M"},
    "nc4np4_full_3x13x17_c48+16_o80": {"kstep_holds_A_and_B", "channel_groups_past_Cout", "group_straddles_row_odd_W", "more_than_one_workgroup"},
    "nc2np8_ups_2x10x14_c48+16_o48": {"kstep_holds_A_and_B", "channel_groups_past_Cout", "group_past_M"},
    "nc2np8_ups_3x14x18_c32+48_o32": {"half_empty_kstep", "more_than_one_workgroup", "group_past_M"},
    "nc2np8_full_3x13x17_c16+16_o32": {"kstep_holds_A_and_B", "more_than_one_workgroup", "group_straddles_row_odd_W"},
    "nc1np8_ups_3x14x18_c80+0_o16": {"half_empty_kstep", "more_than_one_workgroup", "group_past_M"},
    "nc1np8_full_3x13x17_c48+16_o16": {"kstep_holds_A_and_B", "more_than_one_workgroup", "group_straddles_image"},
    "head_ups_1x2x2_c32+48_o1": {"class_rows_past_C", "half_empty_kstep", "wide_b"},
    "head_ups_3x14x18_c64+64_o3": {"class_rows_past_C", "more_than_one_workgroup", "wide_b"},
    "head_nobias_ups_2x10x14_c80+0_o2": {"half_empty_kstep", "kstep_holds_A_and_B", "group_straddles_image"},
    "head_full_3x13x17_c32+48_o2": {"more_than_one_workgroup", "group_straddles_row_odd_W", "wide_b"},
}


def _moved(x, y):
    return float(torch.nan_to_num((x - y).abs(), nan=float("inf")).max())


def _scale(ref):
    return max(1.0, float(ref.abs().max()))


# ---- the restatement of unrounded operands is the plain convolution -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UNET_NAMES)
def test_unet_restatement_unrounded_equals_conv2d_on_the_materialised_input(name):
    c = EC.unet_case(name)
    a, b, w, bias = EC.unet_inputs(name)
    x = a[..., :c["C1"]].permute(0, 3, 1, 2).double()
    if c["ups"]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    if c["C2"]:
        x = torch.cat([x, b[..., :c["C2"]].permute(0, 3, 1, 2).double()], 1)
    want = F.conv2d(x, w.double(), None if bias is None else bias.double(), 1, 1).permute(0, 2, 3, 1).reshape(c["M"], c["Cout"])
    got = EC.unet_expected(name, 0)
    assert got.shape == want.shape and _moved(got, want) <= 1e-12 * _scale(want)


@pytest.mark.parametrize("name", list(EC.SPLITK_CASES))
def test_conv_restatement_unrounded_equals_conv2d(name):
    g, x, w, bias, res = EC.splitk_inputs(name)
    xs = x[..., g["xoff"]:g["xoff"] + g["Cin"]].permute(0, 3, 1, 2).double()
    want = F.conv2d(xs, w.double(), None, g["stride"], g["pad"], g["dil"]).permute(0, 2, 3, 1)
    assert tuple(want.shape) == (g["B"], g["Ho"], g["Wo"], g["Cout"])
    want = want.reshape(-1, g["Cout"])
    got = R.total(R.conv_tiles(x, w, g, 0))
    assert _moved(got, want) <= 1e-12 * _scale(want)
    # the epilogue, written out per element
    full = R.conv(x, w, g, 0, bias, res)
    for m, ch in ((0, 0), (want.shape[0] - 1, g["Cout"] - 1), (want.shape[0] // 2, g["Cout"] // 2)):
        v = float(want[m, ch])
        if bias is not None:
            v += float(bias[(m // (g["Ho"] * g["Wo"])) * g["bias_bstride"] + ch])
        if res is not None:
            v += float(res.reshape(-1)[m * g["ldr"] + g["roff"] + ch])
        v = {R.ACT_NONE: v, R.ACT_RELU: max(v, 0.0), R.ACT_PRELU: v if v > 0 else float(g["alpha"]) * v, R.ACT_SIGMOID: 1.0 / (1.0 + math.exp(-v))}[g["act"]]
        assert abs(float(full[m, ch]) - v) <= 1e-12 * max(1.0, abs(v))


def test_operand_split_is_bf16_round_to_nearest_even():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -16, -3.1415927, 1e-30, 0.0])
    hi, lo = R.split(v)
    assert hi.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]          # ties go to the even mantissa
    assert lo.tolist()[:4] == [0.0, 2.0 ** -8, -(2.0 ** -8), 2.0 ** -16]
    assert float((v - hi - lo).abs().max()) <= 2.0 ** -16 * 4


# ---- guards -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", UNET_NAMES)
def test_unet_case_guards(name):
    c = EC.unet_case(name)
    a, b, w, bias = EC.unet_inputs(name)
    C1, C2, Cout = c["C1"], c["C2"], c["Cout"]
    # args_ok / ape_unet_conv3x3_supported of csrc/unet.hip
    assert C1 >= 16 and C1 % 16 == 0 and C2 >= 0 and C2 % 16 == 0 and c["lda"] >= C1 and c["lda"] % 4 == 0
    assert not C2 or (c["ldb"] >= C2 and c["ldb"] % 4 == 0)
    assert not c["ups"] or (c["H"] % 2 == 0 and c["W"] % 2 == 0)
    if c["head"]:
        assert 1 <= Cout <= 16
    else:
        assert Cout >= 16 and Cout % 16 == 0 and c["ldy"] % 4 == 0 and c["yoff"] % 4 == 0
        assert c["yoff"] > 0 and c["ldy"] > c["yoff"] + Cout
    assert c["M"] <= 4000
    # sentinels: what the kernel must not read is NaN, what it reads is finite
    assert tuple(a.shape) == (c["B"], c["Ha"], c["Wa"], c["lda"]) and c["lda"] >= C1 + 8
    assert torch.isnan(a[..., C1:]).all() and torch.isfinite(a[..., :C1]).all()
    if C2:
        assert tuple(b.shape) == (c["B"], c["H"], c["W"], c["ldb"]) and c["ldb"] > C2
        assert torch.isnan(b[..., C2:]).all() and torch.isfinite(b[..., :C2]).all()
    else:
        assert b is None
    assert (bias is None) == (not c["bias"])
    br = EC.unet_branches(c)
    assert ALWAYS <= br, name                                         # every case: a ragged last group and a wide operand
    assert UNET_BRANCHES.get(name, set()) <= br, (name, sorted(br))
    if c["dup"] is not None:
        for hi_c, lo_c in enumerate(c["dup"]):
            assert torch.equal(w[hi_c], w[lo_c]) and torch.equal(bias[hi_c], bias[lo_c])
        for nsplit in (1, 3):
            lg = EC.unet_expected(name, nsplit)
            assert torch.equal(lg, lg[:, list(c["dup"])])             # bit-identical logits by construction


def test_unet_case_table_covers_every_instantiation():
    """2 UPS x {(4,4), (2,8), (1,8), head} (x 2 nsplit: every case runs for both): a ragged last group, a wide operand, a group wholly past
    M and more than one workgroup under each; every map, every channel split with each instantiation; every Cout / class count"""
    seen = {}
    for name in UNET_NAMES:
        c = EC.unet_case(name)
        key = ("head" if c["head"] else c["inst"], c["ups"])
        s = seen.setdefault(key, dict(br=set(), maps=set(), ch=set(), co=set()))
        s["br"] |= EC.unet_branches(c)
        s["maps"].add(c["map"])
        s["ch"].add((c["C1"], c["C2"]))
        s["co"].add(c["Cout"])
    insts = list(EC.UNET_INSTANTIATIONS) + ["head"]
    assert set(seen) == {(i, u) for i in insts for u in (0, 1)}
    for (inst, ups), s in seen.items():
        assert {"lanes_past_M", "group_past_M", "wide_a", "wide_b", "more_than_one_workgroup", "kstep_holds_A_and_B", "half_empty_kstep"} <= s["br"], (inst, ups)
        assert s["maps"] == set(EC.UNET_MAPS_UPS if ups else EC.UNET_MAPS_FULL), (inst, ups)
        if not ups:
            assert "group_straddles_row_odd_W" in s["br"] and "group_straddles_image" in s["br"]
    for inst in insts:
        assert seen[(inst, 0)]["ch"] | seen[(inst, 1)]["ch"] == set(EC.UNET_CHANNELS), inst
        co = seen[(inst, 0)]["co"] | seen[(inst, 1)]["co"]
        if inst == "head":
            assert co == set(EC.HEAD_CLASSES)
        else:
            assert co == {c for c in EC.UNET_COUT if EC.unet_instantiation(c) == inst}
            if inst != (1, 8):
                assert "channel_groups_past_Cout" in seen[(inst, 0)]["br"] | seen[(inst, 1)]["br"]      # NC = 2 at 48, NC = 4 at Cout % 64 != 0
    heads = [EC.unet_case(n) for n in EC.UNET_HEAD_CASES]
    for ups in (0, 1):
        assert {bool(c["C2"]) for c in heads if c["ups"] == ups} == {False, True}                      # with and without a skip
        assert {c["bias"] for c in heads if c["ups"] == ups} == {False, True}
    dups = {c["dup"] for c in heads if c["dup"] is not None}
    assert any(d[5] == 4 and len(set(d)) == 15 for d in dups)            # a pair inside one lane's four classes
    assert any(d[9] == 2 and len(set(d)) == 12 for d in dups)            # a pair across lane groups
    assert any(len(set(d)) == 1 for d in dups)                           # all classes equal


@pytest.mark.parametrize("name", list(EC.UNET_HEAD_CASES))
def test_head_restatement_stays_inside_the_exclusion_cap(name):
    c = EC.unet_case(name)
    for nsplit in (1, 3):
        lg = EC.unet_expected(name, nsplit)
        assert float(lg.abs().max()) >= 1.0                               # logits of scale >= 1
        for dsm in (0, 1):
            gap = R.top2_gap(R.head(lg, dsm)[2], c["dup"])
            n = int((gap < EC.label_band(lg, c["Cout"], dsm)).sum())
            assert n <= EC.EXCLUDE_CAP * c["M"], (name, nsplit, dsm, n)


def _supported(g):
    """supported() of csrc/conv_gemm.hip"""
    ho = (g["H"] + 2 * g["pad"] - g["dil"] * (g["KH"] - 1) - 1) // g["stride"] + 1
    wo = (g["W"] + 2 * g["pad"] - g["dil"] * (g["KW"] - 1) - 1) // g["stride"] + 1
    return (g["Cin"] >= 32 and g["Cin"] % 32 == 0 and g["ldx"] % 4 == 0 and g["xoff"] % 4 == 0 and g["xoff"] + g["Cin"] <= g["ldx"]
            and g["yoff"] + g["Cout"] <= g["ldy"] and (ho, wo) == (g["Ho"], g["Wo"]) and g["ups"] == 0 and 0 <= g["act"] <= 3)


def _pure(g):
    return g["KH"] == 1 and g["KW"] == 1 and g["stride"] == 1 and g["pad"] == 0


@pytest.mark.parametrize("name", list(EC.SPLITK_CASES))
def test_splitk_case_guards(name):
    g, x, w, bias, res = EC.splitk_inputs(name)
    assert _supported(g)
    nk, nk_per, launched = EC.splitk_plan(g)
    assert nk_per > 0 and launched >= 2                                   # a case the library would not split tests nothing
    M = g["B"] * g["Ho"] * g["Wo"]
    assert M <= 4000
    # sentinels
    assert g["ldx"] > g["Cin"] and g["ldy"] > g["Cout"]
    rd = torch.zeros(g["ldx"], dtype=torch.bool)
    rd[g["xoff"]:g["xoff"] + g["Cin"]] = True
    assert torch.isnan(x[..., ~rd]).all() and torch.isfinite(x[..., rd]).all()
    if res is not None:
        assert g["roff"] + g["Cout"] <= g["ldr"] and g["ldr"] > g["Cout"] and int(torch.isnan(res).sum()) == M * (g["ldr"] - g["Cout"])
    if g["bias_bstride"]:
        assert g["bias_bstride"] > g["Cout"] and int(torch.isnan(bias).sum()) == g["B"] * (g["bias_bstride"] - g["Cout"])
    for nsplit in (1, 3):
        assert torch.isfinite(EC.splitk_expected(name, nsplit)).all()
    # the split walk: every k-tile exactly once, in order
    walk = R.splitk_ktiles(g, nk_per)
    assert len(walk) == launched and [kt for sp in walk for kt in sp] == list(range(nk))


def test_splitk_cases_reach_the_branches_they_are_named_for():
    plan = {n: (EC.splitk_inputs(n)[0],) + EC.splitk_plan(EC.splitk_inputs(n)[0]) for n in EC.SPLITK_CASES}
    taps = lambda g: g["KH"] * g["KW"]  # noqa: E731
    g, nk, per, n = plan["linear_M1_cout65"]
    assert g["B"] * g["Ho"] * g["Wo"] == 1 and (g["Cin"], g["Cout"]) == (256, 65) and _pure(g)
    g, nk, per, n = plan["pure_slices_per_image_bias_prelu"]
    assert _pure(g) and g["B"] == 3 and g["Ho"] * g["Wo"] == 37 and (g["Cin"], g["xoff"], g["ldx"]) == (288, 32, 352)
    assert (g["Cout"], g["yoff"], g["ldy"], g["roff"], g["ldr"], g["bias_bstride"], g["act"]) == (130, 8, 160, 4, 140, 136, R.ACT_PRELU)
    g, nk, per, n = plan["dil2_second_split_starts_at_tap5_sigmoid"]
    assert (nk, n, g["dil"], g["act"]) == (9, 2, 2, R.ACT_SIGMOID) and divmod(per, taps(g)) == (0, 5) and g["bias_bstride"] and g["Ho"] * g["Wo"] > 1
    g, nk, per, n = plan["pad1_splits_start_mid_chunk_last_has_3"]
    assert nk == 18 and [divmod(s * per, taps(g)) for s in range(n)] == [(0, 0), (0, 5), (1, 1), (1, 6)] and nk - (n - 1) * per == 3
    g, nk, per, n = plan["stride2_one_tap_not_pure"]
    assert taps(g) == 1 and not _pure(g) and g["Cin"] == 256
    g, nk, per, n = plan["pure_cin672_last_split_one_ktile"]
    assert _pure(g) and nk == 21 and nk - (n - 1) * per == 1
    g, nk, per, n = plan["pure_cin1056_fewer_splits_launched"]
    assert _pure(g) and nk == 33 and n < EC.splitk_requested(g)
    g, nk, per, n = plan["M129_cout129_ragged_second_tiles"]
    assert g["B"] * g["Ho"] * g["Wo"] == 129 and g["Cout"] == 129
    # conv_gemm_splitk_kernel<{1, 3}, {pure, not}>: every case runs for both nsplit
    assert {_pure(p[0]) for p in plan.values()} == {False, True}
    assert {p[0]["act"] for p in plan.values()} == {R.ACT_NONE, R.ACT_RELU, R.ACT_PRELU, R.ACT_SIGMOID}
    # a chip-filling shape is left alone
    assert EC.splitk_plan(R.conv_geometry(64, 20, 20, 256, 512))[1] == 0 and EC.splitk_plan(R.conv_geometry(1, 20, 20, 256, 64))[1] == 0


# ---- the same products accumulated in float32, in the kernels' order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", UNET_NAMES)
def test_unet_float32_accumulation_stays_within_half_the_bar(name, nsplit):
    c = EC.unet_case(name)
    a, b, w, bias = EC.unet_inputs(name)
    acc = R.accumulate_f32(R.unet_tiles(a, b, w, c["C1"], c["C2"], bool(c["ups"]), nsplit))
    if bias is not None:
        acc = acc + bias[None, :]
    ref = EC.unet_expected(name, nsplit)
    r = _moved(acc.double(), ref) / _scale(ref)
    assert r <= 0.5 * EC.BAR, (name, nsplit, r)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", list(EC.SPLITK_CASES))
def test_splitk_float32_accumulation_stays_within_half_the_bar(name, nsplit):
    g, x, w, bias, res = EC.splitk_inputs(name)
    emu = R.conv_splitk_f32(x, w, g, nsplit, EC.splitk_plan(g)[1], bias, res)
    ref = EC.splitk_expected(name, nsplit)
    r = _moved(emu.double(), ref) / _scale(ref)
    assert r <= 0.5 * EC.BAR, (name, nsplit, r)


# ---- mutations: each wrong rule moves the result by at least 10 x the GPU bar on the cases named for it ------------------------------------------------
def _unet_mutated(name, nsplit, mutation):
    c = EC.unet_case(name)
    a, b, w, bias = EC.unet_inputs(name)
    ref = EC.unet_expected(name, nsplit)
    return _moved(R.unet_logits(a, b, w, bias, c["C1"], c["C2"], bool(c["ups"]), nsplit, (mutation,)), ref) / _scale(ref)


def _splitk_mutated(name, nsplit, mutation):
    g, x, w, bias, res = EC.splitk_inputs(name)
    ref = EC.splitk_expected(name, nsplit)
    return _moved(R.conv(x, w, g, nsplit, bias, res, EC.splitk_plan(g)[1], (mutation,)), ref) / _scale(ref)


MUTATION_CASES = {
    "drop_cross_term": [("unet", n, 3) for n in EC.UNET_CONV_CASES] + [("splitk", n, 3) for n in EC.SPLITK_CASES],
    # (a 2 x 2 map up-sampled from one pixel has one source index only)
    "nearest_rounds_up": [("unet", n, s) for n in UNET_NAMES if EC.unet_case(n)["ups"] and EC.unet_case(n)["Ha"] > 1 for s in (1, 3)],
    "chunk_at_c1_from_a": [("unet", n, s) for n in UNET_NAMES if EC.unet_case(n)["C2"] for s in (1, 3)],
    "border_clamped": [("unet", n, s) for n in UNET_NAMES for s in (1, 3)],
    "split_starts_at_tap0": [("splitk", n, s) for n in ("dil2_second_split_starts_at_tap5_sigmoid", "pad1_splits_start_mid_chunk_last_has_3") for s in (1, 3)],
    "last_split_dropped": [("splitk", n, s) for n in EC.SPLITK_CASES for s in (1, 3)],
    "bias_of_image0": [("splitk", n, s) for n in ("pure_slices_per_image_bias_prelu", "dil2_second_split_starts_at_tap5_sigmoid") for s in (1, 3)],
    "residual_without_roff": [("splitk", n, s) for n in ("pure_slices_per_image_bias_prelu", "pad1_splits_start_mid_chunk_last_has_3") for s in (1, 3)],
}


@pytest.mark.parametrize("mutation", list(MUTATION_CASES))
def test_mutation_moves_the_result(mutation):
    assert mutation in R.MUTATIONS
    for kind, name, nsplit in MUTATION_CASES[mutation]:
        r = (_unet_mutated if kind == "unet" else _splitk_mutated)(name, nsplit, mutation)
        assert r >= 10 * EC.BAR, (mutation, name, nsplit, r)


def test_mutation_last_maximum_changes_the_label_of_the_duplicated_classes():
    n_cases = 0
    for name in EC.UNET_HEAD_CASES:
        c = EC.unet_case(name)
        if c["dup"] is None:
            continue
        n_cases += 1
        higher = torch.tensor([d != k for k, d in enumerate(c["dup"])])
        for nsplit in (1, 3):
            lg = EC.unet_expected(name, nsplit)
            first, last = R.head(lg, 1)[0], R.head(lg, 1, ("last_maximum",))[0]
            assert not higher[first].any()                                # the restatement never names a duplicate's higher index
            wrong = first != last
            assert wrong.any() and higher[last[wrong]].all(), name
            if len(set(c["dup"])) == 1:
                assert wrong.all() and (first == 0).all()
    assert n_cases >= 6
    assert set(MUTATION_CASES) | {"last_maximum"} == set(R.MUTATIONS) - set(R.HALO_MUTATIONS)      # (those: tests/test_halo_edges_host.py)

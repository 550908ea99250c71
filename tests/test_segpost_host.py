"""CPU proofs about the inputs of tests/segpost_edge_cases.py and the restatement tests/segpost_reference.py: every case holds its guards
(dyadic scores, exact sums or a margin, crops inside the image, B < 65536, the exclusion cap) and reaches the branch it is named for; the
restatement agrees with oracle/densefusion_oracle.py and scipy.ndimage.label where both are defined; and each wrong rule, carried by a
mutated copy of the restatement, fails on the cases named for it.  No GPU."""
import numpy as np
import pytest
import torch

import segpost_edge_cases as EC
import segpost_reference as R
from oracle import densefusion_oracle as O

ALL7 = set(EC.MERGE_BRANCHES)
# case -> (branches that must be taken, branches that must not)
BRANCHES = {
    "all_binary_3x4": (ALL7 - {"wave_left"}, set()),
    "all_ternary_3x3": (ALL7, set()),
    "checker_2x2": ({"nw_union", "ne_union"}, ALL7 - {"nw_union", "ne_union"}),
    "checker_5x5": ({"nw_union", "ne_union"}, ALL7 - {"nw_union", "ne_union"}),
    "size_64x1": ({"n_first"}, ALL7 - {"n_first"}),
    "size_65x1": ({"n_first"}, ALL7 - {"n_first"}),
    "size_1x65": ({"wave_left"}, ALL7 - {"wave_left"}),
    "size_3x129": (ALL7, set()),
    "stair_ne_w1_ov0": ({"ne_union"}, ALL7 - {"ne_union"}),
    "stair_ne_w3_ov0": ({"ne_union"}, ALL7 - {"ne_union"}),
    "stair_ne_w3_ov1": ({"ne_skip", "n_first"}, {"ne_union", "nw_union", "nw_skip"}),
    "stair_nw_w1_ov0": ({"nw_union"}, ALL7 - {"nw_union"}),
    "stair_nw_w3_ov0": ({"nw_union"}, ALL7 - {"nw_union"}),
    "stair_nw_w3_ov1": ({"nw_skip", "n_first"}, {"nw_union", "ne_union", "ne_skip"}),
    "labels_ge_C": (ALL7, set()),
}
for _w in (63, 65, 127, 128, 129):
    BRANCHES["fullrow_W%d" % _w] = ({"wave_left", "n_first", "n_skip"}, set())
BRANCHES["fullrow_W64"] = ({"n_first", "n_skip"}, {"wave_left"})
for _L in (1, 63, 64, 65, 129):
    BRANCHES["run_L%d_lane0" % _L] = ({"wave_left"}, set()) if _L > 64 else (set(), {"wave_left"})
    BRANCHES["run_L%d_lane63" % _L] = ({"wave_left"}, set()) if _L > 1 else (set(), {"wave_left"})
for _t in ("spiral", "comb", "u", "u_mirror", "rings"):
    BRANCHES["%s_x1" % _t] = ({"n_first"}, {"n_skip"})
    BRANCHES["%s_x2" % _t] = ({"n_first", "n_skip", "wave_left"}, set())


# ---- components: guards, branches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.COMPONENT_CASES))
def test_component_cases_hold_their_guards(name):
    case = EC.component_case(name)
    label, C = case["label"], case["C"]
    B, H, W = label.shape
    assert B < 65536 and label.dtype == np.uint8 and 1 <= C <= 64
    for sname, score in case["scores"]:
        assert score.dtype == np.float32 and score.shape == label.shape and EC.is_dyadic(score), (name, sname)
        assert sname == "zero" or score.min() >= 2.0 ** -8
    if name.startswith("all_"):
        assert H * W < 64                                   # several frames share a wave: no link may cross a frame
        assert len(np.unique(label.reshape(B, -1), axis=0)) == B == (C ** (H * W))
    took = EC.merge_branches(label)
    must, must_not = BRANCHES.get(name, (set(), set()))
    assert all(took[k] > 0 for k in must) and all(took[k] == 0 for k in must_not), (name, took)
    if B > 1000:
        return                                              # (the exhaustive batches: components of at most 12 pixels, checked below on a sample)
    for sname, score in case["scores"]:
        for mode in EC.MODES:
            objmap, tight, det, best = R.components(label, score, C, case["min_pixels"], mode)
            for b in range(B):
                for c, (root, win, second) in best[b].items():
                    n_px = int((objmap[b] == c).sum())
                    if n_px > 8192 and second is not None:          # rule 2: a margin where the sums are not exact
                        a, s = win[0] / win[1], second[0] / second[1]
                        assert a - s >= 2.0 ** -20 * a, (name, sname, b, c)
            valid = det[..., 0] == 1
            inside = (det[..., 1] >= 0) & (det[..., 2] <= H) & (det[..., 3] >= 0) & (det[..., 4] <= W)
            if case["in_image"]:
                assert inside[valid].all(), name
    if name in EC.BOX_SMALL:
        assert not inside[valid].all()                      # the box leaves the image exactly as dataset.py's arithmetic does


def test_named_component_cases_say_what_they_claim():
    c = EC.component_case("threshold_100")
    assert int((c["label"] == 1).sum()) == 100 and c["min_pixels"] == 100
    c = EC.component_case("threshold_101")
    assert int((c["label"] == 1).sum()) == 101 and len(np.unique(R.flood(c["label"][0], 3)[c["label"][0] == 1])) == 2
    for _, score in c["scores"]:
        objmap = R.components(c["label"], score, 3, 100, R.MEAN)[0]
        assert int((objmap == 1).sum()) in (60, 41) and not (objmap == 2).any()
    kept = {int((R.components(c["label"], s, 3, 100, R.MEAN)[0] == 1).sum()) for _, s in c["scores"]}
    assert kept == {60, 41}                                 # the 60 wins or loses by score
    for k in (2, 3):
        lab, sc = EC.component_case("tie%d" % k)["label"], EC.component_case("tie%d" % k)["scores"][0][1]
        ids = R.flood(lab[0], 3)
        roots = sorted(set(ids[ids >= 0].tolist()))
        assert len(roots) == k and len({tuple(sorted(sc[0][ids == r].tolist())) for r in roots}) == 1     # congruent, the same multiset
        for mode in EC.MODES:
            assert R.components(lab, sc, 3, 0, mode)[3][0][1][0] == roots[0]
            later = EC.component_case("tie%d_later_better" % k)["scores"][0][1]
            assert R.components(lab, later, 3, 0, mode)[3][0][1][0] == roots[-1]
    z = EC.component_case("tie_all_zero")
    assert not z["scores"][0][1][z["label"] == 1].any()
    assert R.components(z["label"], z["scores"][0][1], 3, 0, R.MEAN)[3][0][1][0] == int(np.flatnonzero(z["label"])[0])
    one = EC.component_case("tie_score_one")
    assert one["scores"][0][1].max() == 1.0
    ext = EC.component_case("box_extents")
    tight = R.components(ext["label"], ext["scores"][0][1], 2, 0, R.MEAN)[1]
    assert sorted((tight[:, 1, 1] - tight[:, 1, 0] + 1).tolist()) == [39, 40, 41, 80, 81]
    bord = EC.component_case("box_borders")
    t = R.components(bord["label"], bord["scores"][0][1], 3, 0, R.MEAN)[1]
    H, W = EC.FRAME
    assert (t[:, :, 0] == 0).any() and (t[:, :, 1] == H - 1).any() and (t[:, :, 2] == 0).any() and (t[:, :, 3] == W - 1).any()
    iso = EC.component_case("isolation_61x77")["label"]
    assert (iso.shape[1] * iso.shape[2]) % 64 != 0
    assert iso[0, -1].all() and iso[1, 0].all() and iso[1, -1, -1] == iso[2, 0, 0] != 0
    oob = EC.component_case("labels_ge_C")
    assert set(np.unique(oob["label"])) >= {5, 63, 64, 255} and oob["C"] == 5 and oob["label"][-1, -1, -1] == 255
    label, _ = EC.grid_stride_batch()
    assert label.shape == (14,) + EC.FRAME and label.size > EC.GRID_STRIDE_PIXELS >= 13 * 480 * 640


# ---- the restatement against the oracle and scipy ----------------------------------------------------------------------------------------------
def _pred_from(label, score, C):
    """a [C,H,W] probability tensor whose arg-max is `label` and whose winning probability is `score`"""
    H, W = label.shape
    pred = np.zeros((C, H, W), np.float32)
    yy, xx = np.indices((H, W))
    pred[label, yy, xx] = np.where(label == 0, 1.5, score)
    return torch.from_numpy(pred)


@pytest.mark.parametrize("name", [n for n in EC.COMPONENT_CASES if n != "tie_all_zero"])
def test_restatement_agrees_with_the_oracle(name):
    from scipy import ndimage
    case = EC.component_case(name)
    C, mp = case["C"], case["min_pixels"]
    label = np.where(case["label"] < C, case["label"], 0).astype(np.uint8)
    frames = range(0, len(label), 37) if len(label) > 1000 else range(len(label))
    for sname, score in case["scores"]:
        for b in frames:
            objmap, _, det, _ = R.components(label[b:b + 1], score[b:b + 1], C, mp, R.MEAN)
            want = O.seg_postprocess(_pred_from(label[b], score[b], C), min_pixels=mp)
            assert {c for c in range(1, C) if det[0, c, 0]} == set(want), (name, sname, b)
            for c, mask in want.items():
                assert np.array_equal(np.where(objmap[0] == c, 255, 0).astype(np.uint8), mask), (name, sname, b, c)
        ids = R.flood(label[frames[-1]], C)
        for c in range(1, C):                                # the same partition as scipy's labelling with a structure of ones
            lab, n = ndimage.label(label[frames[-1]] == c, structure=np.ones((3, 3), np.int32))
            pairs = set(zip(ids[lab > 0].tolist(), lab[lab > 0].tolist()))
            assert len(pairs) == n == len({p[0] for p in pairs}) and not (ids[(lab == 0) & (label[frames[-1]] == c)] >= 0).any()


# ---- each wrong rule fails on the cases named for it -------------------------------------------------------------------------------------------
def _components_differ(name, rules, modes=EC.MODES):
    case = EC.component_case(name)
    for _, score in case["scores"]:
        for mode in modes:
            a = R.components(case["label"], score, case["C"], case["min_pixels"], mode)
            b = R.components(case["label"], score, case["C"], case["min_pixels"], mode, rules)
            if not (np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])):
                return True
    return False


@pytest.mark.parametrize("rules,names,modes", [
    (dict(connectivity=4), ["checker_2x2", "checker_5x5", "stair_ne_w1_ov0", "stair_nw_w1_ov0", "stair_ne_w3_ov0", "stair_nw_w3_ov0", "all_binary_3x4"], EC.MODES),
    (dict(threshold="ge"), ["threshold_100"], EC.MODES),
    (dict(count="component"), ["threshold_101"], EC.MODES),
    (dict(ties="last"), ["tie2", "tie3", "tie_all_zero", "all_binary_3x4"], EC.MODES),
    (dict(score="mean_for_sum"), ["threshold_101", "all_ternary_3x3"], (R.SUM,)),
])
def test_wrong_component_rules_fail_their_cases(rules, names, modes):
    for name in names:
        assert _components_differ(name, rules, modes), (rules, name)


def test_wrong_choose_rules_fail_their_cases():
    om, dp, objs = EC.depth_case()
    assert {0, 1, 32768, 65535} <= set(np.unique(dp[0, 2:9, 3:12]).tolist())
    assert not np.array_equal(R.choose(om, dp, objs, 7, 0)[1], R.choose(om, dp, objs, 7, 0, dict(depth="signed_gt0"))[1])
    for name in ("n255_N256", "n999_N1000", "crop_15", "cand_4095_4096"):
        om, dp, objs, ns = EC.choose_case(name)
        assert not np.array_equal(R.choose(om, dp, objs, ns[-1], 0)[0], R.choose(om, dp, objs, ns[-1], 0, dict(wrap="end"))[0]), name
    for name in ("n513_N256", "n2001_N1000", "n257_N256", "crop_8193"):
        om, dp, objs, ns = EC.choose_case(name)
        for seed in EC.SEEDS:
            assert not np.array_equal(R.choose(om, dp, objs, ns[-1], seed)[0], R.choose(om, dp, objs, ns[-1], seed, dict(offset="none"))[0]), name


# ---- choose_points --------------------------------------------------------------------------------------------------------------------------------
def _inside(om, objs):
    _, H, W = om.shape
    return all(0 <= b < len(om) and 0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W for b, _, r0, r1, c0, c1 in objs.tolist())


@pytest.mark.parametrize("name", list(EC.CHOOSE_CASES))
def test_choose_cases_reach_their_counts(name):
    om, dp, objs, ns = EC.choose_case(name)
    assert _inside(om, objs)
    _, _, r0, r1, c0, c1 = objs[0].tolist()
    total, cand = (r1 - r0) * (c1 - c0), R.candidates(om, dp, objs[0])
    assert total <= om.shape[1] * om.shape[2]               # the engine's candidate stride
    if name.startswith("crop_"):
        want = int(name.split("_")[1])
        assert total == want == len(cand) and EC.passes(total) == {8193: 3, 4097: 2}.get(want, 1)
        assert (c1 - c0 == 1) == (want in (1, 16)) and (c1 - c0 == 3) == (want in (15, 8193))
    elif name.startswith("cand_"):
        assert total == 8192 and EC.passes(total) == 2
        assert cand.tolist() == {"cand_none": [], "cand_first": [0], "cand_last": [8191], "cand_4095_4096": [4095, 4096]}[name]
    else:
        n, N = int(name[1:].split("_N")[0]), ns[0]
        assert len(cand) == n and ns == (N,) and N in EC.N_VALUES
    crop_d = dp[0, r0:r1, c0:c1]
    crop_m = om[0, r0:r1, c0:c1] == objs[0, 1]
    if len(cand) >= 3:
        assert {1, 65535} <= set(crop_d.ravel()[cand].tolist())
    if len(cand) < total:
        assert (crop_m & (crop_d == 0)).any()               # depth 0 under a set mask
    for N in ns:
        for seed in EC.SEEDS:
            ch, n_cand = R.choose(om, dp, objs, N, seed)
            assert ch.shape == (1, N) and np.isin(ch[0], cand).all() if len(cand) else not ch.any()
            if len(cand) > N:
                assert np.all(np.diff(ch[0]) > 0)
            elif len(cand):
                assert np.array_equal(ch[0], np.pad(cand, (0, N - len(cand)), "wrap"))


def test_choose_cases_cover_the_listed_values():
    names = set(EC.CHOOSE_CASES)
    for N in EC.N_VALUES:
        for n in (0, 1, N - 1, N, N + 1, 2 * N, 2 * N + 1):
            assert "n%d_N%d" % (n, N) in names
    assert set(EC.CROP_SHAPES) == {1, 15, 16, 17, 4095, 4096, 4097, 8193} and EC.SEEDS == (0, 2 ** 32 - 1)
    assert R.hash32(0, 0) != R.hash32(2 ** 32 - 1, 0)
    om, dp, objs = EC.whole_frame_case()
    assert objs[0].tolist() == [0, 2, 0, 480, 0, 640] and len(R.candidates(om, dp, objs[0])) > 1000
    for n_obj in (1, 64, 300):
        om, dp, objs = EC.many_objects_case(n_obj)
        assert len(objs) == n_obj and _inside(om, objs) and len(om) == 3
        n_cand = R.choose(om, dp, objs, 1000, 0)[1]
        if n_obj > 1:
            assert (n_cand > 1000).any() and (n_cand < 1000).any() and (n_cand > 0).all()
            a, b = objs[0], objs[1]
            assert a[0] == b[0] and a[1] != b[1] and a[2] < b[3] and b[2] < a[3] and a[4] < b[5] and b[4] < a[5]      # overlapping crops


def test_preprocess_frame_holds_every_byte_in_every_channel():
    rgb = EC.preprocess_frame()
    for ch in range(3):
        assert len(np.unique(rgb[0, :, :, ch])) == 256
    for div255 in (False, True):
        full = R.preprocess(rgb, np.array([[0, 0, 0]]), 16, 16, div255)
        want = (O.seg_input(rgb[0]) if div255 else O.crop_image(rgb[0], 0, 16, 0, 16))[0].permute(1, 2, 0).numpy()
        assert np.array_equal(full[0, :, :, :3], want) and not full[..., 3].any()


# ---- seg_argmax / seg_head: the reference alone stays inside the exclusion cap ------------------------------------------------------------------
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("C,ld,npix", EC.ARGMAX_CASES)
def test_argmax_cases_stay_inside_the_exclusion_cap(C, ld, npix, double):
    logits = EC.argmax_logits(C, ld, npix)
    assert logits.shape == (npix, ld) and ld >= C
    if ld > C:
        assert (logits[:, C] == np.float32(1e30)).all() and np.isnan(logits[:, C + 1]).all()
    label, score, unsure = R.argmax_score(logits, C, double)
    assert np.isfinite(score).all() and (score > 0).all() and unsure.sum() <= EC.EXCLUDE_CAP * npix
    if not double:                                          # the float32 label is the float64 arg-max outside the band
        assert np.array_equal(label[~unsure], logits[:, :C].astype(np.float64).argmax(-1)[~unsure])
    if npix > EC.GRID_STRIDE_PIXELS:
        assert C == 2


def test_argmax_cases_cover_the_listed_values():
    assert {c[0] for c in EC.ARGMAX_CASES} == {1, 2, 13, 64} and (13, 16, 257) in EC.ARGMAX_CASES
    assert {c[2] for c in EC.ARGMAX_CASES} == {1, 255, 256, 257, 4194304 + 257}
    assert {c[0] for c in EC.HEAD_CASES} == {1, 2, 4, 5, 13, 16} and {c[1] for c in EC.HEAD_CASES} == {1, 15, 16, 17, 1000, 524288 + 19}
    assert {c[2:] for c in EC.HEAD_CASES} == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("C,npix,with_bias,double", EC.HEAD_CASES)
def test_head_cases_are_exact_and_inside_the_cap(C, npix, with_bias, double):
    feat, w, bias = EC.head_inputs(C, npix, with_bias)
    assert (bias is None) == (not with_bias)
    logits = feat.astype(np.float64) @ w.astype(np.float64).T + (bias.astype(np.float64) if with_bias else 0.0)
    terms = np.abs(feat.astype(np.float64)) @ np.abs(w.astype(np.float64)).T + (np.abs(bias) if with_bias else 0.0)
    assert np.array_equal(logits * 4096, np.round(logits * 4096)) and terms.max() * 4096 < 2 ** 24      # exact in float32, in any order
    if C > 1:
        top = np.sort(logits, -1)[:, -2:]
        assert (top[:, 1] - top[:, 0]).min() >= 2.0 ** -12
    label, score, unsure = R.head(feat, w, bias, C, double)
    assert not unsure.any()                                 # a gap of 2^-12 keeps every pixel outside the band
    assert np.array_equal(label, logits.argmax(-1))


# ---- label_trust_counts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", EC.TRUST_SIZES)
def test_trust_inputs_reach_their_edges(hw):
    objmap, bs, depth, gate = EC.trust_inputs(*hw)
    h, w = hw
    assert objmap.shape == (3, h, w) and len({tuple(g) for g in gate.tolist()}) == 3
    if h * w > 30:
        assert {0, 499, 500, 800, 801} <= set(np.unique(depth[0]).tolist())        # at dmin and dmax, one step outside, and 0
    assert (0, 0) in EC.TRUST_CUTS and (30, 50) in EC.TRUST_CUTS
    for cut0, cut1 in EC.TRUST_CUTS:
        want = R.trust_counts(objmap, 1, bs, depth, gate, cut0, cut1)
        window = max(h - 2 * cut0, 0) * max(w - 2 * cut1, 0)
        assert (want[:, 4] + want[:, 5] == window).all()
        assert (want[:, 0] + want[:, 1] == (bs != 0).reshape(3, -1).sum(1)).all()
        for b in range(3):                                  # the reference's own lines, create_labels.py:111-112 and :169-192
            pred = np.where(objmap[b] == 1, 255, 0).astype(np.uint8)
            d = depth[b].astype(float)
            d[d > gate[b, 1]] = 0
            d[d < gate[b, 0]] = 0
            assert (len(np.unique(pred[bs[b] != 0])) > 1) == (want[b, 0] > 0 and want[b, 1] > 0)
            assert (len(np.unique(pred[d != 0])) > 1) == (want[b, 2] > 0 and want[b, 3] > 0)
            if cut0 * 2 < h and cut1 * 2 < w:
                assert (len(np.unique(pred[cut0:h - cut0, cut1:w - cut1])) > 1) == (want[b, 4] > 0 and want[b, 5] > 0)
        assert not R.trust_counts(objmap, 1, None, depth, gate, cut0, cut1)[:, :2].any()
    assert any(c0 * 2 > h or c1 * 2 > w for c0, c1 in EC.TRUST_CUTS)                # an empty window
    if h == 61:
        assert R.trust_counts(objmap, 1, bs, depth, gate, 0, 0)[:, 2:4].sum(1).tolist() == [
            int(((depth[b] != 0) & (depth[b] >= gate[b, 0]) & (depth[b] <= gate[b, 1])).sum()) for b in range(3)]

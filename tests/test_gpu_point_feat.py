"""The point-feature front in one launch (ape_point_feat_bf16, csrc/point_feat.hip) against the five launches it replaces: the four
`engine.Conv` calls of `_FeatPlan` with their out= / xoff / yoff, then `S32.from_f32`.  Those kernels are pinned by the goldens of
tests/test_gpu_posenet.py; the fused launch must give every fp32 value and every S32 byte BIT FOR BIT (all comparisons are on int32
views, so -0.0 and NaN payloads count).  R = 256 rows per workgroup, 32 per wave, 16 per matrix-instruction block."""
import numpy as np
import pytest
import torch

from autoposeestimation_amd import synthetic as S

pytestmark = pytest.mark.gpu
CLASSES = ["obj%02d" % i for i in range(12)]
SENTINEL = -777.25
GUARD = 3                                     # sentinel rows in front of and behind every output, NaN rows behind every input
X_COLS = list(range(0, 64)) + list(range(128, 256))          # conv1 | conv2 (S32: the 128-byte groups of the same channels)
E_COLS = list(range(64, 128)) + list(range(256, 384))        # e_conv1 | e_conv2
ROWS = [1, 15, 16, 17, 255, 256, 257, 513, 1000]             # around the 16-row block, the 256-row workgroup (R - 1, R, R + 1, 2 R + 1), one crop
_LAYERS = {}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layers(kind):
    """seeded conv1 / e_conv1 / conv2 / e_conv2 of PoseNetFeat's or PoseRefineNetFeat's shapes as the `engine.Conv` objects _FeatPlan
    builds; zero-mean weights and biases, so about half of the pre-activations are negative (asserted where the reference is made)"""
    from autoposeestimation_amd import engine as E
    if kind not in _LAYERS:
        sd = S.posenet_state_dict(3, 0) if kind == "posenet" else S.refiner_state_dict(3, 0)
        gen = torch.Generator().manual_seed(11 if kind == "posenet" else 29)
        out = []
        for k in ("conv1", "e_conv1", "conv2", "e_conv2"):
            w = torch.randn(sd["feat.%s.weight" % k].shape, generator=gen) * 0.3
            b = torch.randn(sd["feat.%s.bias" % k].shape, generator=gen) * 0.2
            out.append(E.Conv(w, b, act=E.ACT_RELU, device="cuda", precision="bf16x3", splitk=True))
        _LAYERS[kind] = out
    return _LAYERS[kind]


def _inputs(m, seed, special=None):
    """x4[m + GUARD, 4], emb[m + GUARD, 32] with NaN in the rows behind m; the fourth component of x4 is 0 as pad3to4 leaves it"""
    gen = torch.Generator().manual_seed(seed)
    x4 = torch.randn(m + GUARD, 4, generator=gen)
    x4[:, 3] = 0
    emb = torch.randn(m + GUARD, 32, generator=gen) * 2 - 1          # (log-softmax values: mostly negative)
    if special == "w":
        x4[:, 3] = torch.randn(m + GUARD, generator=gen)             # a non-zero fourth component (its weight column is the zero pad)
    if special == "tiny":
        tiny = torch.tensor([-0.0, 1e-40, -1e-40, 1.4e-45, 0.0, -1e-38, 3e-39, 1.0])       # -0, denormals of both signs, the smallest one
        x4[: m // 2 + 1, :3] = tiny[torch.randint(0, 8, (m // 2 + 1, 3), generator=gen)]
        emb[: m // 2 + 1] = tiny[torch.randint(0, 8, (m // 2 + 1, 32), generator=gen)]
    x4[m:] = float("nan")
    emb[m:] = float("nan")
    return x4.cuda(), emb.cuda()


def _reference(layers, x4, emb, m):
    """the five launches on the first m rows -> pf[m, 384] f32, its S32 bytes as a float32 tensor"""
    from autoposeestimation_amd import engine as E
    c1, e1, c2, e2 = layers
    pf = torch.full((1, m, 1, 384), SENTINEL, device="cuda")
    c1(x4[:m].view(1, m, 1, 4), out=pf, yoff=0)
    e1(emb[:m].view(1, m, 1, 32), out=pf, yoff=64)
    c2(pf, out=pf, xoff=0, yoff=128)
    e2(pf, out=pf, xoff=64, yoff=256)
    return pf.view(m, 384), E.S32.from_f32(pf).t.view(m, 384)


def _fused(layers, x4, emb, m, want_f32, want_s32, parts):
    """the fused launch into sentinel-filled buffers with guard rows -> the whole buffers [GUARD + m + GUARD, 384] (None if not asked for)"""
    from autoposeestimation_amd import engine as E
    bufs = [torch.full((GUARD + m + GUARD, 384), SENTINEL, device="cuda") if w else None for w in (want_f32, want_s32)]
    pf = None if bufs[0] is None else bufs[0][GUARD:GUARD + m]
    pfs = None if bufs[1] is None else E.S32(bufs[1][GUARD:GUARD + m])
    E.point_feat(x4[:m], emb[:m], *layers, pf=pf, pf_s32=pfs, parts=parts)
    return bufs


def _check(buf, want, m, parts, tag):
    sent = torch.full((1,), SENTINEL).view(torch.int32).item()
    got = _bits(buf)
    assert bool((got[:GUARD] == sent).all()) and bool((got[GUARD + m:] == sent).all()), (tag, "guard rows written")
    body, wb = got[GUARD:GUARD + m], _bits(want)
    for bit, cols in ((1, X_COLS), (2, E_COLS)):
        if parts & bit:
            assert torch.equal(body[:, cols], wb[:, cols]), (tag, "half %d differs" % bit, int((body[:, cols] != wb[:, cols]).sum()))
        else:
            assert bool((body[:, cols] == sent).all()), (tag, "unselected half %d written" % bit)


def _run_all(kind, m, special=None):
    layers = _layers(kind)
    x4, emb = _inputs(m, 1000 + m, special)
    want_f32, want_s32 = _reference(layers, x4, emb, m)
    if m >= 255:                                  # the biases leave both signs in every layer: roughly half of the outputs are ReLU zeros
        zeros = float((want_f32 == 0).float().mean())
        assert 0.25 < zeros < 0.75, zeros
    for f32, s32 in ((True, False), (False, True), (True, True)):
        for parts in (1, 2, 3):
            bufs = _fused(layers, x4, emb, m, f32, s32, parts)
            if f32:
                _check(bufs[0], want_f32, m, parts, (kind, m, "f32", f32, s32, parts))
            if s32:
                _check(bufs[1], want_s32, m, parts, (kind, m, "s32", f32, s32, parts))
    return want_f32


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("kind", ["posenet", "refiner"])
def test_fused_launch_equals_the_five_launches(kind, m):
    """every output set (fp32, S32, both) and every `parts` value: the selected columns equal, the others and the guard rows untouched"""
    _run_all(kind, m)


def test_nonzero_fourth_component():
    _run_all("posenet", 257, special="w")


def test_negative_zero_and_denormal_inputs():
    want = _run_all("refiner", 257, special="tiny")
    assert bool(torch.isfinite(want).all())


def test_the_split_is_split_lo_of_the_fp32_values():
    """the S32 bytes against the host restatement of the split (hi = bf16(v), lo = bf16(v - hi), both round to nearest even)"""
    layers = _layers("posenet")
    x4, emb = _inputs(300, 7)
    f32, s32 = _fused(layers, x4, emb, 300, True, True, 3)
    v = f32[GUARD:GUARD + 300].cpu().view(300, 12, 32)
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    want = torch.cat([hi, lo], 2).contiguous().view(torch.int16).view(300, 384 * 2)
    assert torch.equal(s32[GUARD:GUARD + 300].cpu().view(torch.int16), want)


# ---- _FeatPlan, the refiner's cache and FramePipeline._bucket -------------------------------------------------------------------------------
def _models():
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet
    if "models" not in _LAYERS:
        est = PoseNet(1000, 12)
        est.load_state_dict(S.posenet_state_dict(12, 0))
        ref = PoseRefineNet(1000, 12)
        ref.load_state_dict(S.refiner_state_dict(12, 0))
        _LAYERS["models"] = (est.cuda().eval().set_precision("bf16x3"), ref.cuda().eval().set_precision("bf16x3"))
    return _LAYERS["models"]


def _switch(monkeypatch, on):
    from autoposeestimation_amd import engine as E
    monkeypatch.setattr(E, "USE_POINT_FEAT", on)


def _shape(rows):
    from autoposeestimation_amd.DenseFusion.lib import network as N
    if rows == "min":
        assert N.S32_MIN_ROWS % 1024 == 0
        return N.S32_MIN_ROWS // 1024, 1024
    return 1, rows


@pytest.mark.parametrize("rows", [771, "min"])
@pytest.mark.parametrize("refine", [False, True])
def test_featplan_equal_with_the_switch_on_and_off(refine, rows, monkeypatch):
    """pf, pf_s32 and the pooled ap of `_FeatPlan` below the pre-split threshold and at it; and the fused launch really ran"""
    from autoposeestimation_amd import engine as E
    b, n = _shape(rows)
    feat = _models()[1 if refine else 0].plan().feat
    gen = torch.Generator().manual_seed(b * n)
    x4 = torch.cat([torch.randn(b, n, 3, generator=gen), torch.zeros(b, n, 1)], 2).cuda().contiguous()
    emb = torch.log_softmax(torch.randn(b, n, 32, generator=gen), 2).cuda().contiguous()
    _switch(monkeypatch, False)
    pf0, ap0 = feat(x4, emb)
    s0 = feat.pf_s32
    _switch(monkeypatch, True)
    prof = E.LaunchProfile()
    monkeypatch.setattr(E, "PROFILE", prof)
    pf1, ap1 = feat(x4, emb)
    s1 = feat.pf_s32
    pf2, ap2 = feat(x4, emb, want_pf=False)
    s2 = feat.pf_s32
    monkeypatch.setattr(E, "PROFILE", None)
    torch.cuda.synchronize()
    labels = [r[0] for r in prof.records]
    assert labels.count(E.POINT_FEAT_LABEL) == 2 and not any("conv_bf16_kernel" in name for name in labels), labels
    assert (s0 is None) == (rows != "min") and (s1 is None) == (s0 is None) and (s2 is None) == (s0 is None)
    assert torch.equal(_bits(pf1), _bits(pf0)) and torch.equal(_bits(ap1), _bits(ap0)) and torch.equal(_bits(ap2), _bits(ap0))
    if s0 is not None:
        assert torch.equal(_bits(s1.t), _bits(s0.t)) and torch.equal(_bits(s2.t), _bits(s0.t))
        assert pf2 is None                        # on the pre-split route nothing reads the fp32 rows unless the caller does
    else:
        assert torch.equal(_bits(pf2), _bits(pf0))


@pytest.mark.parametrize("rows", [771, "min"])
def test_refiner_with_a_cache_over_two_iterations_equals_without(rows, monkeypatch):
    from autoposeestimation_amd.DenseFusion.lib.network import FeatCache
    b, n = _shape(rows)
    ref = _models()[1]
    gen = torch.Generator().manual_seed(5 + b * n)
    pts = [torch.cat([torch.randn(b, n, 3, generator=gen) * 0.05, torch.zeros(b, n, 1)], 2).cuda().contiguous() for _ in range(2)]
    emb = torch.log_softmax(torch.randn(b, n, 32, generator=gen), 2).cuda().contiguous()
    obj = (torch.arange(b) % 12).cuda()
    _switch(monkeypatch, False)
    old = [ref.forward_batch(p, emb, obj) for p in pts]
    _switch(monkeypatch, True)
    plain = [ref.forward_batch(p, emb, obj) for p in pts]
    cache = FeatCache()
    cached = [ref.forward_batch(p, emb, obj, cache=cache) for p in pts]
    assert cache.key is not None
    for a, c, d in zip(old, plain, cached):
        assert torch.equal(_bits(c), _bits(a)) and torch.equal(_bits(d), _bits(a))
    assert not torch.equal(old[0], old[1])        # (the two iterations really saw different points)


def _scene():
    from autoposeestimation_amd import engine as E
    frames = [S.synthetic_frame(31 + i, cls=1 + 2 * i, box=(100 + 40 * i, 200), size=(70, 70)) for i in range(2)]
    rgb = torch.from_numpy(np.stack([f[0] for f in frames])).cuda()
    depth = torch.from_numpy(np.stack([f[1] for f in frames])).cuda()
    label = torch.from_numpy(np.stack([f[2] for f in frames]).astype(np.uint8)).cuda()
    objmap, det = E.seg_components(label, torch.ones(label.shape, dtype=torch.float32, device="cuda"), 13, 100)
    det_h = det.cpu().numpy()
    fb, fc = np.nonzero(det_h[:, 1:, 0])
    objects = [(int(f), int(c) + 1, *map(int, det_h[f, c + 1, 1:5])) for f, c in zip(fb, fc)]
    assert len(objects) == 2
    return rgb, depth, objmap, objects


@pytest.mark.parametrize("presplit", [False, True])
@pytest.mark.parametrize("pose_graphs", [False, True])
@pytest.mark.parametrize("refine_mode", ["live_compat", "iterative"])
def test_bucket_equal_with_the_switch_on_and_off(refine_mode, pose_graphs, presplit, monkeypatch):
    """FramePipeline's pose stage on one bucket of two crops (2000 rows): pose, choose and n_cand with the fused launch and the refiner's
    cache equal those of the five launches, eagerly and (pose_graphs) in the eager, the capturing and a replayed step; presplit moves the
    pre-split threshold under the bucket's row count so that the S32 outputs and the cached S32 buffer are the ones in use"""
    from autoposeestimation_amd.DenseFusion.lib import network as N
    from autoposeestimation_amd.pipeline.utils import FramePipeline
    est, ref = _models()
    rgb, depth, objmap, objects = _scene()
    if presplit:
        monkeypatch.setattr(N, "S32_MIN_ROWS", 2000)
    outs = {}
    for on in (False, True):
        _switch(monkeypatch, on)
        pipe = FramePipeline(None, est, ref, CLASSES, refine_mode=refine_mode, pose_graphs=pose_graphs)
        outs[on] = [tuple(t.clone() for t in pipe.poses(rgb, depth, objmap, objects, S.REALSENSE_META, seed=3 + step)) for step in range(3)]
        torch.cuda.synchronize()
        assert len(pipe._graphs) == (1 if pose_graphs else 0)
    for step in range(3):
        for k, (a, c) in enumerate(zip(outs[False][step], outs[True][step])):
            assert torch.equal(a, c), (step, ("pose", "n_cand", "choose")[k])
        assert bool(torch.isfinite(outs[True][step][0]).all())

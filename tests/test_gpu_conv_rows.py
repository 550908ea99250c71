"""conv_rows_kernel (conv_gemm.hip variant 7: the small-M form of the pure 1x1 convolution, one wave per 16 x 16 output block, operands
straight from global memory) against the 128x128 block of conv_gemm_kernel (engine.GEMM_VARIANT = 2) on the same E.Conv call, BIT FOR
BIT: both form, per output element, the same sum -- k-tiles of 32 ascending into one accumulator, the three split products per k-tile
in the same order on the same operand positions, the same epilogue.  Then the pose networks' head chains with the form switched off."""
import pytest
import torch

from autoposeestimation_amd import synthetic as S

pytestmark = pytest.mark.gpu

SHAPES = [(32, 16), (96, 20), (384, 1280), (1024, 1920)]      # one k-tile / a 3-tile K tail and a ragged Cout / l1_rt / l1_global
ROWS = [1, 3, 16, 17, 64]
NSPLIT = {"bf16x3": 3, "bf16": 1}
_CONVS, _DATA = {}, {}


def _conv(cin, cout, act, precision):
    from autoposeestimation_amd import engine as E
    key = (cin, cout, act, precision)
    if key not in _CONVS:
        g = torch.Generator().manual_seed(cin * 7 + cout)
        wt = torch.randn(cout, cin, generator=g) / cin ** 0.5
        _CONVS[key] = E.Conv(wt, None, act=act, device="cuda", precision=precision)
    return _CONVS[key]


def _data(m, cin, cout):
    """x[m,1,1,cin+36] read at xoff 32, a shared bias[cout], a per-row bias[m,cout]"""
    key = (m, cin, cout)
    if key not in _DATA:
        g = torch.Generator().manual_seed(m * 1000 + cin + cout)
        _DATA[key] = ((torch.randn(m, 1, 1, cin + 36, generator=g) * 3).cuda(), torch.randn(cout, generator=g).cuda(),
                      torch.randn(m, cout, generator=g).cuda())
    return _DATA[key]


def _run(conv, x, variant, ldy, yoff, profile=None, **kw):
    """conv(x) into channels yoff.. of a buffer of ldy channels filled with 7, under engine.GEMM_VARIANT = variant -> (buffer, label of the launch)"""
    from autoposeestimation_amd import engine as E
    out = torch.full((x.shape[0], x.shape[1], x.shape[2], ldy), 7.0, device="cuda")
    keep = (E.GEMM_VARIANT, E.PROFILE)
    try:
        E.GEMM_VARIANT, E.PROFILE = variant, E.LaunchProfile()
        conv(x, out=out, yoff=yoff, **kw)
        labels = [r[0] for r in E.PROFILE.records]
    finally:
        E.GEMM_VARIANT, E.PROFILE = keep
    assert len(labels) == 1
    return out, labels[0]


@pytest.mark.parametrize("cin,cout", SHAPES)
@pytest.mark.parametrize("m", ROWS)
def test_rows_form_equals_the_128x128_block(m, cin, cout):
    from autoposeestimation_amd import engine as E
    x, bias, bias_rows = _data(m, cin, cout)
    for precision in ("bf16x3", "bf16"):
        for act in (E.ACT_NONE, E.ACT_RELU):
            conv = _conv(cin, cout, act, precision)
            for tag, kw in (("none", {}), ("shared", dict(bias=bias)), ("per row", dict(bias=bias_rows, bias_bstride=cout))):
                got, label = _run(conv, x, 0, cout + 8, 4, xoff=32, **kw)
                want, ref_label = _run(conv, x, 2, cout + 8, 4, xoff=32, **kw)
                assert label == "conv_rows_kernel<%d>" % NSPLIT[precision], label
                assert ref_label == "conv_gemm_kernel<%d,128,128,2,2,true,false>" % NSPLIT[precision], ref_label
                assert torch.equal(got, want), (m, cin, cout, precision, act, tag)
                assert bool((got[..., :4] == 7.0).all()) and bool((got[..., 4 + cout:] == 7.0).all())
            if act == E.ACT_RELU:
                assert bool((got[..., 4:4 + cout] == 0).any()) and bool((got[..., 4:4 + cout] > 0).any())


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_rows_form_scalar_stores_and_images_of_several_rows(precision):
    """an output slice that is not float4-aligned (the element-wise epilogue), and a per-image bias over images of 8 rows ([2,8,1,C])"""
    from autoposeestimation_amd import engine as E
    conv = _conv(96, 20, E.ACT_RELU, precision)
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(2, 8, 1, 96 + 36, generator=g) * 3).cuda()
    bias_img = torch.randn(2, 24, generator=g).cuda()
    for ldy, yoff in ((27, 3), (28, 4)):
        got, label = _run(conv, x, 0, ldy, yoff, xoff=32, bias=bias_img, bias_bstride=24)
        want, _ = _run(conv, x, 2, ldy, yoff, xoff=32, bias=bias_img, bias_bstride=24)
        assert label == "conv_rows_kernel<%d>" % NSPLIT[precision]
        assert torch.equal(got, want), (ldy, yoff)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_rows_form_is_not_taken_above_its_row_bound_nor_with_a_residual(precision):
    from autoposeestimation_amd import engine as E
    ns = NSPLIT[precision]
    conv = _conv(384, 1280, E.ACT_RELU, precision)
    m = E.GEMM_ROWS_MAX_M + 1
    x, bias, _ = _data(m, 384, 1280)
    got, label = _run(conv, x, 0, 1288, 4, xoff=32, bias=bias)
    want, _ = _run(conv, x, 2, 1288, 4, xoff=32, bias=bias)
    assert label == "conv_gemm_kernel<%d,128,128,2,2,true,false>" % ns, label
    assert torch.equal(got, want)
    x, bias, _ = _data(16, 384, 1280)
    res = torch.randn(16, 1, 1, 1280, generator=torch.Generator().manual_seed(9)).cuda()
    got, label = _run(conv, x, 0, 1288, 4, xoff=32, bias=bias, residual=res)
    want, _ = _run(conv, x, 2, 1288, 4, xoff=32, bias=bias, residual=res)
    assert label == "conv_gemm_kernel<%d,128,128,2,2,true,false>" % ns, label
    assert torch.equal(got, want)
    # forced, the form refuses what it does not compute; without a residual it takes any row count
    from autoposeestimation_amd._lib import ApeError
    with pytest.raises(ApeError):
        _run(conv, x, 7, 1288, 4, xoff=32, bias=bias, residual=res)
    x, bias, _ = _data(m, 384, 1280)
    got, _ = _run(conv, x, 7, 1288, 4, xoff=32, bias=bias)
    want, _ = _run(conv, x, 2, 1288, 4, xoff=32, bias=bias)
    assert torch.equal(got, want)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_pose_networks_equal_with_the_rows_form_switched_off(precision):
    """PoseNet.forward_pose and PoseRefineNet.forward_batch on 2 crops x 64 points: l1_global, l1_rt, l2, l3 / l1, l2 run on 2 rows"""
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.DenseFusion.lib.network import PoseNet, PoseRefineNet
    est = PoseNet(64, 12)
    est.load_state_dict(S.posenet_state_dict(12, 0))
    est = est.cuda().eval().set_precision(precision)
    ref = PoseRefineNet(64, 12)
    ref.load_state_dict(S.refiner_state_dict(12, 0))
    ref = ref.cuda().eval().set_precision(precision)
    gen = torch.Generator().manual_seed(2)
    b, n, hc = 2, 64, 40
    img4 = torch.cat([torch.randn(b, hc, hc, 3, generator=gen), torch.zeros(b, hc, hc, 1)], 3).cuda().contiguous()
    pts4 = torch.cat([torch.randn(b, n, 3, generator=gen) * 0.1, torch.zeros(b, n, 1)], 2).cuda().contiguous()
    choose = torch.randint(0, hc * hc, (b, n), generator=gen).cuda()
    obj = torch.tensor([3, 11], dtype=torch.int64).cuda()

    def run():
        prof = E.PROFILE = E.LaunchProfile()
        try:
            pose, which, newp, emb = est.forward_pose(img4, pts4, choose, obj)
            out = ref.forward_batch(newp, emb, obj)
        finally:
            E.PROFILE = None
        return (pose, which, newp, emb, out), sum(r[0].startswith("conv_rows_kernel") for r in prof.records)

    keep = E.USE_GEMM_ROWS
    try:
        E.USE_GEMM_ROWS = True
        got, n_rows = run()
        E.USE_GEMM_ROWS = False
        want, n_off = run()
    finally:
        E.USE_GEMM_ROWS = keep
    assert n_rows >= 9 and n_off == 0, (n_rows, n_off)       # l1_global, l1_rt, 2 x l2, 2 x l3; the refiner's l1, 2 x l2
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[4]).all())

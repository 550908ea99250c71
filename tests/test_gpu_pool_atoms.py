"""The PSP pools' first pass with one workgroup per ATOM (avgpool_atom_kernel) against the former one workgroup per atom ROW
(avgpool_atoms_kernel, engine.POOL_ATOM_ROWS): only the parallelism differs -- every (atom, channel) adds rows y = g (mod 4) per wave with
ascending columns, then acc_0 + part_0 + part_1 + part_2 -- so every pooled output is the same BIT FOR BIT."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# h, w, channels pooled, channels per pixel, pre-split input
MAPS = [(60, 80, 512, 576, True),       # the segmentor's layer-4 map with the folded form's 64 spare channels: 6 x 10 atoms, 13- and 1-pixel columns
        (20, 20, 512, 512, False),      # the crops' map: atoms of 3 and 4 pixels
        (7, 9, 64, 64, False)]          # overlapping bins: atoms of one pixel; one partial channel chunk (16 of 64 lanes)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w,c,ld,s32", MAPS)
def test_one_workgroup_per_atom_equals_one_per_atom_row(h, w, c, ld, s32, b):
    from autoposeestimation_amd import engine as E
    g = torch.Generator().manual_seed(h * 100 + w + b)
    x = (torch.randn(b, h, w, ld, generator=g) * 3 + 0.5).clamp_(-16, 16).cuda()
    src = E.S32.from_f32(x) if s32 else x
    keep = E.POOL_ATOM_ROWS
    try:
        E.POOL_ATOM_ROWS = False
        got = E.adaptive_avgpool_multi(src, (2, 3, 6), channels=c)
        E.POOL_ATOM_ROWS = True
        want = E.adaptive_avgpool_multi(src, (2, 3, 6), channels=c)
    finally:
        E.POOL_ATOM_ROWS = keep
    for s in (2, 3, 6):
        assert got[s].shape == (b, s, s, c)
        assert torch.equal(got[s], want[s]), (s, (got[s] - want[s]).abs().max().item())
    # and the values are the pools: a bin is a sequential fp32 sum of N <= 30 x 40 values |v| <= 16, so each of its N additions rounds a partial
    # sum <= 16 N by at most 2^-24 of it and the MEAN is off by at most 16 N 2^-24 = 1.2e-3 (worst case; the division adds half an ulp)
    ref = x[..., :c]
    if s32:
        ref = src.to_f32()[..., :c]
    ref = ref.permute(0, 3, 1, 2).double().cpu()
    for s in (2, 3, 6):
        exact = torch.nn.functional.adaptive_avg_pool2d(ref, s).permute(0, 2, 3, 1)
        assert (got[s].cpu().double() - exact).abs().max().item() <= 1.2e-3

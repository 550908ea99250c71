"""The label-audit kernels (csrc/label_audit.hip) and the label-quality driver (experiments/gt_test.py) on the GPU.  Counts must equal the
numpy restatement of the contract (tests/gt_test_reference.py) exactly, images byte for byte; the driver must print what the reference
printed (tests/golden/gt_test.npz) and return what its numpy path returns."""
import ctypes
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import golden

import gt_test_reference as R

pytestmark = pytest.mark.gpu
GOLD = golden("gt_test")
CLASSES = [str(c) for c in GOLD["classes"]]
EINVAL = -1
VALUES = np.array([0, 1, 128, 255], dtype=np.uint8)
# 1 pixel; 15 / 16 / 17: below, at and above one 16-byte group; 35: odd, every plane start unaligned; 2257: odd, body and tail;
# 12576 pixels: two workgroups, the second partial
SIZES = ((1, 1), (1, 15), (1, 16), (1, 17), (5, 7), (37, 61), (96, 131))
PAIRS16 = [(0, 0), (0, 1), (1, 0), (7, 7), (7, 0), (0, 7), (2, 5), (5, 2), (3, 4), (4, 3), (6, 1), (1, 6), (2, 2), (5, 7), (7, 5), (3, 6)]


def _pair_sets(L):
    from autoposeestimation_amd.experiments import gt_test as G
    return {2: [[(0, 1)], [(1, 0)], [(1, 1)]], 4: [list(G.PAIRS)], 8: [PAIRS16]}[L]


def _labels(b, L, h, w, seed):
    rng = np.random.default_rng(seed)
    lab = rng.choice(VALUES, (b, L, h, w), p=[0.4, 0.2, 0.2, 0.2])
    lab[0, 1] = 0                       # an all-zero plane
    lab[b - 1, L - 1] = 255             # an all-255 plane
    if b > 1:
        lab[1, 0] = 255
    return lab


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("L", (2, 4, 8))
@pytest.mark.parametrize("h,w", SIZES)
def test_counts_equal_the_restatement(h, w, L):
    from autoposeestimation_amd import engine as E
    for b in (1, 3):
        lab = _labels(b, L, h, w, seed=h * 1000 + w * 10 + L + b)
        for pairs in _pair_sets(L):
            got = E.label_pair_counts(_dev(lab), pairs)
            assert got.dtype == torch.int64 and tuple(got.shape) == (b, len(pairs), 4)
            want = R.pair_counts(lab, pairs)
            assert np.array_equal(got.cpu().numpy(), want), (b, pairs)
            assert (want.sum(axis=2) == h * w).all()


def test_counts_at_480x640_batch_2():
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.experiments import gt_test as G
    lab = _labels(2, 4, 480, 640, seed=5)
    assert np.array_equal(E.label_pair_counts(_dev(lab), G.PAIRS).cpu().numpy(), R.pair_counts(lab, G.PAIRS))


def test_counts_from_a_base_address_that_is_odd():
    """the whole label block one byte into an allocation: no plane of it is aligned to anything"""
    from autoposeestimation_amd import engine as E
    lab = _labels(3, 8, 37, 61, seed=11)
    buf = torch.zeros(lab.size + 64, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + lab.size].view(lab.shape)
    view.copy_(_dev(lab))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    assert np.array_equal(E.label_pair_counts(view, PAIRS16).cpu().numpy(), R.pair_counts(lab, PAIRS16))


def _raw_counts(lab_t, pairs, counts_t, b=None, L=None, hw=None, p=None, labels_ptr=True, pairs_ptr=True, counts_ptr=None):
    from autoposeestimation_amd import _lib
    table = (ctypes.c_int32 * (2 * len(pairs)))(*[v for pr in pairs for v in pr])
    shape = lab_t.shape
    return _lib.lib().ape_label_pair_counts_u8(
        ctypes.c_void_p(lab_t.data_ptr()) if labels_ptr else None, shape[0] if b is None else b, shape[1] if L is None else L,
        shape[2] * shape[3] if hw is None else hw, ctypes.cast(table, ctypes.c_void_p) if pairs_ptr else None,
        len(pairs) if p is None else p, ctypes.c_void_p(counts_t.data_ptr() if counts_ptr is None else counts_ptr), _lib.stream_ptr())


def test_counts_overwrite_a_buffer_full_of_garbage_and_do_not_accumulate():
    from autoposeestimation_amd.experiments import gt_test as G
    lab = _labels(3, 4, 37, 61, seed=3)
    lab_t = _dev(lab)
    counts = torch.full((3, 5, 4), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    want = R.pair_counts(lab, G.PAIRS)
    assert _raw_counts(lab_t, G.PAIRS, counts) == 0
    assert np.array_equal(counts.cpu().numpy(), want)
    assert _raw_counts(lab_t, G.PAIRS, counts) == 0
    assert np.array_equal(counts.cpu().numpy(), want)


def _rgb_and_labels(b, h, w, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (b, h, w, 3), dtype=np.uint8)
    rgb[0, 0, :3] = 0
    rgb[0, -1, -3:] = 255
    lab = rng.choice(np.array([0, 1, 255], dtype=np.uint8), (b, 3, h, w), p=[0.4, 0.3, 0.3])
    lab[0, :, 0, 0] = (255, 1, 255)                     # both labels set on a pixel of value 0, and on one of value 255
    lab[0, :, -1, -1] = (1, 255, 255)
    assert ((lab[:, 0] != 0) & (lab[:, 1] != 0)).sum() > 2
    return rgb, lab


@pytest.mark.parametrize("h,w", ((5, 7), (37, 61)))
def test_blend_is_byte_equal_to_the_restatement(h, w):
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    c0, c1 = 0.7, 1.0 - 0.7
    for b in (1, 2):
        rgb, lab = _rgb_and_labels(b, h, w, seed=h + b)
        rgb_t, lab_t = _dev(rgb), _dev(lab)
        for first, second in (((2, 2), (1, 0)), ((0, 1), (1, 1)), ((1, 0), (0, 2)), ((2, 0), (2, 0))):      # ch_a == ch_b among them
            got = E.label_pair_blend(rgb_t, lab_t, first, second, c0, c1)
            assert np.array_equal(got.cpu().numpy(), R.pair_blend(rgb, lab, first, second, c0, c1)), (b, first, second)
        out = torch.full_like(rgb_t, 0xA5)                      # a buffer full of garbage: every byte is written
        rc = _lib.lib().ape_label_pair_blend_u8(ctypes.c_void_p(rgb_t.data_ptr()), ctypes.c_void_p(lab_t.data_ptr()), b, 3, h, w, 0, 2, 1, 0,
                                                c0, c1, ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr())
        assert rc == 0 and np.array_equal(out.cpu().numpy(), R.pair_blend(rgb, lab, (0, 2), (1, 0), c0, c1))
        assert np.array_equal(rgb_t.cpu().numpy(), rgb)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from autoposeestimation_amd import synthetic as S
    root = str(tmp_path_factory.mktemp("gt_test_tree"))
    S.gt_test_tree(root)
    return root


def test_device_driver_equals_the_golden_and_the_host_path(tree, tmp_path, capsys):
    from autoposeestimation_amd.experiments import gt_test as G
    out = str(tmp_path / "overlays")
    dev = G.main(tree, classes=CLASSES, use_cuda=True, batch=5, overlay_dir=out)
    printed = capsys.readouterr().out
    host = G.main(tree, classes=CLASSES, use_cuda=False)
    capsys.readouterr()
    assert printed.split("\n") == str(GOLD["stdout"]).split("\n")
    assert [[s[n] for n in G.NAMES] for s in dev["per_sample"]] == GOLD["per_sample"].tolist()
    assert dev == host
    for cls, rot, sid in dev["order"]:
        paths = G._sample_paths(tree, cls, rot, sid)
        planes = np.stack([G._decode(paths[k]) for k in G.PLANES])
        rgb = np.array(Image.open(paths["image"]).convert("RGB"), dtype=np.uint8)
        for tag, pa, pb in G.OVERLAYS:
            got = np.array(Image.open(os.path.join(out, cls, rot, "%s.%s.png" % (sid, tag))))
            assert np.array_equal(got, R.pair_blend(rgb[None], planes[None], (pa, 2), (pb, 0), 0.7, 1.0 - 0.7)[0]), (cls, rot, sid, tag)
    labels = _dev(np.stack([np.stack([G._decode(G._sample_paths(tree, *o)[k]) for k in G.PLANES]) for o in dev["order"]]))
    assert G.pair_stats(labels) == GOLD["per_sample"].tolist()


def test_einval_leaves_the_output_untouched():
    from autoposeestimation_amd import _lib
    lab = _labels(2, 8, 5, 7, seed=1)
    lab_t = _dev(lab)
    fill = 0x5A5A5A5A5A5A5A5A
    counts = torch.full((2 * 16 * 4 + 1,), fill, dtype=torch.int64, device="cuda")
    one = [(0, 1)]
    cases = [dict(labels_ptr=False), dict(pairs_ptr=False), dict(counts_ptr=0),
             dict(L=0), dict(L=9), dict(p=0), dict(p=17), dict(b=0), dict(hw=0),
             dict(counts_ptr=counts.data_ptr() + 4)]
    for kw in cases:
        pairs = PAIRS16 + [(0, 0)] if kw.get("p") == 17 else one
        assert _raw_counts(lab_t, pairs, counts, **kw) == EINVAL, kw
    assert _raw_counts(lab_t, [(0, 8)], counts) == EINVAL and _raw_counts(lab_t, [(8, 0)], counts) == EINVAL      # a pair index equal to L
    assert _raw_counts(lab_t, [(0, -1)], counts) == EINVAL
    assert b"ape_label_pair_counts_u8" in _lib.lib().ape_last_error()
    torch.cuda.synchronize()
    assert (counts.cpu() == fill).all()

    rgb_t = torch.full((2, 5, 7, 3), 9, dtype=torch.uint8, device="cuda")
    out = torch.full_like(rgb_t, 0xA5)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    blend = _lib.lib().ape_label_pair_blend_u8
    st = _lib.stream_ptr()
    assert blend(None, P(lab_t), 2, 8, 5, 7, 0, 2, 1, 0, 0.7, 0.3, P(out), st) == EINVAL
    assert blend(P(rgb_t), None, 2, 8, 5, 7, 0, 2, 1, 0, 0.7, 0.3, P(out), st) == EINVAL
    assert blend(P(rgb_t), P(lab_t), 2, 8, 5, 7, 0, 2, 1, 0, 0.7, 0.3, None, st) == EINVAL
    assert blend(P(rgb_t), P(lab_t), 2, 8, 5, 7, 0, 2, 1, 0, 0.7, 0.3, P(rgb_t), st) == EINVAL          # out aliasing rgb
    assert blend(P(rgb_t), P(lab_t), 2, 8, 5, 7, 0, 3, 1, 0, 0.7, 0.3, P(out), st) == EINVAL            # channel 3
    assert blend(P(rgb_t), P(lab_t), 2, 8, 5, 7, 0, 2, 1, -1, 0.7, 0.3, P(out), st) == EINVAL
    assert blend(P(rgb_t), P(lab_t), 2, 8, 5, 7, 8, 2, 1, 0, 0.7, 0.3, P(out), st) == EINVAL            # plane equal to L
    assert blend(P(rgb_t), P(lab_t), 2, 8, 5, 7, 0, 2, -1, 0, 0.7, 0.3, P(out), st) == EINVAL
    for bad in ((0, 8, 5, 7), (2, 0, 5, 7), (2, 8, 0, 7), (2, 8, 5, 0)):
        assert blend(P(rgb_t), P(lab_t), *bad, 0, 2, 0, 0, 0.7, 0.3, P(out), st) == EINVAL, bad
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all() and (rgb_t.cpu() == 9).all()

"""The numpy restatement of the classical RGB-D labeller (tests/label_rgbd_reference.py) against what can be had without OpenCV, and the
host side of the device path: the per-pixel header compiled for the host (tools/check_label_px.py) and the argument handling of
label_generator/utils.py.  No GPU.  Parity with OpenCV unpinned: the checks below pin the restatement to OpenCV's DOCUMENTED semantics --
known colours and the float formula for HSV, scipy.ndimage for the morphology, the box filter and the labelling."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import label_rgbd_cases as C  # noqa: E402
import label_rgbd_reference as R  # noqa: E402

ndi = pytest.importorskip("scipy.ndimage")


# ---- HSV -----------------------------------------------------------------------------------------------------------------------------------
def test_hsv_known_colours():
    known = {(0, 0, 0): (0, 0, 0), (255, 255, 255): (0, 0, 255), (128, 128, 128): (0, 0, 128), (1, 1, 1): (0, 0, 1),
             (255, 0, 0): (0, 255, 255), (0, 255, 0): (60, 255, 255), (0, 0, 255): (120, 255, 255),
             (255, 255, 0): (30, 255, 255), (0, 255, 255): (90, 255, 255), (255, 0, 255): (150, 255, 255),
             # S of the next three: (100 * sdiv[200] + 2048) >> 12 = (100 * 5222 + 2048) >> 12 = 127 (the float formula gives 127.5)
             (200, 200, 100): (30, 127, 200),       # v == r == g: the r branch is taken, h = g - b: (100 * 1229 + 2048) >> 12 = 30
             (200, 100, 200): (150, 127, 200),      # v == r == b: the r branch, h = g - b = -100: (-122900 + 2048) >> 12 = -30, + 180
             (100, 200, 200): (90, 127, 200),       # v == g == b: the g branch, h = b - r + 2 diff = 300: (368700 + 2048) >> 12 = 90
             (255, 0, 1): (0, 255, 255)}            # just below red: (-1 * 482 + 2048) >> 12 = 0, no wrap
    for rgb, hsv in known.items():
        assert tuple(int(v) for v in R.hsv_u8(np.array(rgb, np.uint8))) == hsv, rgb


def test_hsv_agrees_with_the_float_formula_within_one_level():
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (100000, 3), dtype=np.uint8)
    got = R.hsv_u8(rgb).astype(np.int64)
    r, g, b = (rgb[:, i].astype(np.float64) for i in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    safe = np.where(diff == 0, 1.0, diff)
    h = np.where(v == r, (g - b) / safe, np.where(v == g, 2.0 + (b - r) / safe, 4.0 + (r - g) / safe)) * 60.0
    h = np.where(diff == 0, 0.0, np.where(h < 0, h + 360.0, h)) / 2.0
    s = np.where(v == 0, 0.0, diff / np.where(v == 0, 1.0, v)) * 255.0
    dh = np.abs(got[:, 0] - h)
    assert np.all(np.minimum(dh, 180.0 - dh) <= 1.0)                  # modulo 180
    assert np.all(np.abs(got[:, 1] - s) <= 1.0) and np.array_equal(got[:, 2], v.astype(np.int64))
    assert got[:, 0].min() >= 0 and got[:, 0].max() <= 179


def test_numpy_sums_the_channels_left_to_right():
    """the device adds the weighted channels left to right; np.sum(axis=2) over 3 or 6 contiguous values does the same"""
    rng = np.random.default_rng(2)
    for c in (3, 6):
        x = rng.uniform(0, 200, (50, 60, c))
        acc = np.zeros((50, 60))
        for i in range(c):
            acc = acc + x[:, :, i]
        assert np.array_equal(np.sum(x, axis=2).view(np.uint64), acc.view(np.uint64))


# ---- morphology, box filter, labelling against scipy.ndimage ---------------------------------------------------------------------------------
def _bordered(h, w, seed):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w))
    for r0, r1, c0, c1 in C.corner_rects(h, w):
        img[r0:r1, c0:c1] = rng.uniform(1.0, 400.0, (r1 - r0, c1 - c0))
    img[rng.random((h, w)) < 0.03] = 0.0
    return img


@pytest.mark.parametrize("k", [3, 6, 9])
def test_morphology_against_scipy(k):
    """offsets -(k // 2) .. k - 1 - (k // 2): scipy centres a size-k footprint at k // 2 as well, so origin 0 is that footprint for the
    erosion; its dilation mirrors the footprint, which for even k needs origin -1 to land on the SAME offsets (OpenCV's erode and dilate
    share one footprint).  Outside pixels do not take part (cval = +-inf)."""
    img = _bordered(37, 53, k)
    for o in (-(k // 2), k - 1 - (k // 2)):                          # the footprint really is asymmetric for even k
        probe = np.zeros((1, 21))
        probe[0, 10] = 1.0
        assert R.dilate(probe, k)[0, 10 - o] == 1.0                  # the pixel at offset o from x reaches x: x + o = 10
    assert np.array_equal(R.erode(img, k), ndi.grey_erosion(img, size=(k, k), origin=0, mode="constant", cval=np.inf))
    assert np.array_equal(R.dilate(img, k), ndi.grey_dilation(img, size=(k, k), origin=-1 if k % 2 == 0 else 0, mode="constant", cval=-np.inf))
    assert np.array_equal(R.opening(img, k), R.dilate(R.erode(img, k), k)) and np.array_equal(R.closing(img, k), R.erode(R.dilate(img, k), k))


def test_box_filter_against_scipy():
    img = _bordered(37, 53, 4) + 1.0
    want = ndi.correlate(img, np.full((5, 5), np.float64(np.float32(1) / np.float32(25))), mode="mirror")
    assert np.max(np.abs(R.smoothing(img, 5) - want)) <= 1e-12 * np.max(want)


def test_labelling_against_scipy():
    img = _bordered(70, 93, 5)
    img[35, :] = np.where(img[35, :] > 0, 256.25, 0.0)               # scores in [256, 257) wrap to background and split components
    assert (R.wrap_u8(img)[35] == 0).all() and (img[35] > 0).any()
    want, n = ndi.label(R.wrap_u8(img) != 0, structure=np.ones((3, 3)))
    got = R.connectedComponents(img)
    assert n >= 9 and np.array_equal(got, want)                      # scipy numbers in raster order of the first pixel too
    whole, n_whole = ndi.label(img != 0, structure=np.ones((3, 3)))
    assert n_whole < n


# ---- hand-built frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.hand_cases()))
def test_hand_built_frames(name):
    frames, expected = C.hand_cases()[name]
    st = {}
    got = R.createLabel_RGBD(*frames, stages=st, **C.HAND_KW)
    assert np.array_equal(got, expected)
    if name == "fallback_keeps_background":
        assert st["chosen1"] == 0
    if name == "no_background_pixel":
        assert st["labeled1"].min() == 1 and st["chosen1"] == 1
    if name == "equal_int_means_first_wins":
        assert st["chosen1"] == 1 and int(st["labeled1"].max()) == 2


def test_depth_arrays_are_left_alone_and_the_plane_fills_the_holes():
    bg, fg, bd, fd = C.frame_pair(70, 93, seed=8)
    keep = bd.copy(), fd.copy()
    rfd, rbd = R.depth_prepare(bd, fd, C.MEASURE_DIST)
    assert np.array_equal(bd, keep[0]) and np.array_equal(fd, keep[1])
    r0, r1, c0, c1 = R.window(70, 93)
    assert (r0, r1, c0, c1) == (14, 56, 18, 74)
    inside = np.zeros((70, 93), bool)
    inside[r0:r1, c0:c1] = True
    assert ((rbd == 0) & inside & (rfd != 0)).sum() == 0 and (R.gate(bd, C.MEASURE_DIST)[inside] == 0).any()


# ---- the per-pixel header, compiled for the host ---------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("c++") is None and shutil.which("hipcc") is None, reason="no host compiler")
def test_pixel_header_on_the_host():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import check_label_px
    colours, pixels = check_label_px.run(sanitize=False, verbose=False)
    assert colours == 1 << 24 and pixels >= 100000


# ---- argument handling -----------------------------------------------------------------------------------------------------------------------
def test_default_weights_per_mode():
    from autoposeestimation_amd.label_generator import utils as U
    assert U.default_p(True, False) == R.P_HSV == [0.08026211175912534, 1.2577782150904344, 1.9483549172969372, 1.392821046939864]
    assert U.default_p(True, True) == R.P_HSV                          # hsv wins over both, as the reference's if / elif
    assert U.default_p(False, True) == R.P_BOTH == [0.8, 0.6, 0.1, 0.3, 0.3, 0.5, 0.5]
    assert U.default_p(False, False) == R.P_RGB == [0.5, 0.5, 0.5, 1]


def test_signature_is_the_reference_s():
    import inspect
    from autoposeestimation_amd.label_generator import create_labels as CL, utils as U
    sig = inspect.signature(U.createLabel_RGBD)
    assert list(sig.parameters) == ["background", "foreground", "background_depth", "foreground_depth", "threshold", "intr", "p", "min_size",
                                    "open", "close", "hsv", "both", "plot", "do_cca", "remove_one_std", "measure_dist"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(threshold=100, intr=None, p=None, min_size=100, open=3, close=9, hsv=True, both=False, plot=False, do_cca=True,
                     remove_one_std=False, measure_dist=None)
    d = {k: v.default for k, v in inspect.signature(CL.create_labels).parameters.items()}
    assert (d["plot"], d["hsv"], d["both"], d["batch"]) == (False, False, True, 16) and d["reference_point"].size == 0
    for name in ("contrast_stretching", "connectedComponents", "smoothing", "opening", "closing", "label_frames_rgbd"):
        assert callable(getattr(U, name))


def test_argument_errors_come_before_the_device_is_touched(tmp_path):
    from autoposeestimation_amd.label_generator import utils as U
    from autoposeestimation_amd.label_generator.create_labels import create_labels
    bg, fg, bd, fd = C.frame_pair(37, 53, seed=1)
    with pytest.raises(ValueError, match="measure_dist"):
        U.createLabel_RGBD(bg, fg, bd, fd)                                              # p[-1] > 0, no measure_dist
    with pytest.raises(ValueError, match="measure_dist"):
        U.createLabel_RGBD(bg, fg, bd, fd, hsv=False, both=True, measure_dist=None)
    with pytest.raises(NotImplementedError):
        U.createLabel_RGBD(bg, fg, bd, fd, plot=True, measure_dist=800.0)
    with pytest.raises(ValueError, match="reference_point"):
        create_labels("thing", str(tmp_path))
    with pytest.raises(NotImplementedError):
        create_labels("thing", str(tmp_path), reference_point=np.zeros(3), plot=True)
    with pytest.raises(ValueError, match="measure_dist"):
        R.createLabel_RGBD(bg, fg, bd, fd)


def test_contrast_stretching_is_the_reference_s_numpy():
    from autoposeestimation_amd.label_generator import utils as U
    x = np.array([[2.0, 4.0], [6.0, 10.0]])
    assert np.array_equal(U.contrast_stretching(x), (x - 2.0) * (255 / 8.0))

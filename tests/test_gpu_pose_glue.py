"""The small kernels around PoseNet / PoseRefineNet and the segmentor held to plain high-precision references of the same op, at
the shapes, ties and magnitudes where such kernels go wrong:

  head_select     conv4_{r,t,c} of the selected object + sigmoid (network.py:115-126)        fp64 torch
  pose_select     my_estimator_prediction + get_new_points (tools/utils.py:7-18, :43-86)     oracle estimator_prediction, get_new_points
  pose_compose    my_refined_prediction (tools/utils.py:20-40)                                oracle refined_prediction
  pose_recentre   eval_ycb.py:205-210 re-centring with fp32 R, t                             fp64 numpy
  recentre_qt     loss.py:61-69 re-centring with an unnormalised fp32 quaternion              oracle quat_to_base + fp64
  adds_select     loss.py:50-59 loss value and most-confident pose                            fp64 torch, first-maximum arg-max
  log_softmax     pspnet.py:55                                                               F.log_softmax in fp64
  gather_rows     network.py:100-102                                                         torch indexing (bitwise)
  maxpool3x3s2    extractors.py:85,117                                                       F.max_pool2d (bitwise)
  adaptive_avgpool (single size) pspnet.py:15                                                F.adaptive_avg_pool2d in fp64

Arg-max ties are planted so that the first maximum sits in a different lane from a later equal one, in the same lane's stride,
at n-1, or everywhere; every arg-max must equal numpy's / torch.max's on the CPU (the first maximum, as the reference's
`torch.max(pred_c, 1)` returns).  All random data comes from fixed seeds.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import densefusion_oracle as O

pytestmark = pytest.mark.gpu


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _gen(*key):
    return torch.Generator().manual_seed(_seed(*key))


# ---- head_select ------------------------------------------------------------------------------------------------------
NUM_OBJ = 21


def _head_weights(k, g, wc_on=True):
    wr = torch.randn(NUM_OBJ * 4, k, generator=g) / k ** 0.5
    br = torch.randn(NUM_OBJ * 4, generator=g)
    wt = torch.randn(NUM_OBJ * 3, k, generator=g) / k ** 0.5
    bt = torch.randn(NUM_OBJ * 3, generator=g) * 0.1
    wc = torch.randn(NUM_OBJ, k, generator=g) / k ** 0.5 if wc_on else None
    bc = torch.randn(NUM_OBJ, generator=g) if wc_on else None
    return wr, br, wt, bt, wc, bc


def _head_ref(h, ldh, offs, weights, obj, b, n, k):
    """fp64: out[b, p, j] = h[b*n+p, off_j : off_j+K] . W_j(obj_b) + bias_j(obj_b) (j < 7), sigmoid(...) for j = 7; plus the
    per-element bound 1e-5 (sum_k |h_k w_k| + |bias|) on the pre-activation.  fmaf over K terms in sequence: the realised
    error is a random walk far below gamma_K; 1e-5 leaves a x50 margin over sqrt(K) u at K = 1024."""
    wr, br, wt, bt, wc, bc = (None if t is None else t.double() for t in weights)
    hd = h.double().view(b, n, ldh)
    o = obj.long()
    ws = [wr.view(NUM_OBJ, 4, k)[o], wt.view(NUM_OBJ, 3, k)[o],
          (wc.view(NUM_OBJ, 1, k)[o] if wc is not None else torch.zeros(b, 1, k, dtype=torch.float64))]
    bs = [br.view(NUM_OBJ, 4)[o], bt.view(NUM_OBJ, 3)[o], (bc[o].view(b, 1) if bc is not None else torch.zeros(b, 1, dtype=torch.float64))]
    val, mag = [], []
    for off, w, bias in zip(offs, ws, bs):
        x = hd[..., off:off + k]
        val.append(torch.einsum("bnk,bjk->bnj", x, w) + bias[:, None, :])
        mag.append(torch.einsum("bnk,bjk->bnj", x.abs(), w.abs()) + bias.abs()[:, None, :])
    return torch.cat(val, 2), torch.cat(mag, 2)


def _check_heads(got, val, mag, has_c):
    tol = 1e-5 * mag
    err = (got[..., :7].double() - val[..., :7]).abs()
    assert bool((err <= tol[..., :7]).all()), float((err / tol[..., :7]).max())
    if has_c:
        # sigmoid' <= 1/4 carries the logit's bound; expf, the add and the divide add <= a few ulp of a value <= 1
        gc = got[..., 7].double()
        assert not bool(torch.isnan(gc).any())
        err = (gc - torch.sigmoid(val[..., 7])).abs()
        assert bool((err <= 0.25 * tol[..., 7] + 1e-6).all()), float(err.max())
    else:
        assert bool((got[..., 7] == 0).all())


@pytest.mark.parametrize("obj_last", [False, True])
@pytest.mark.parametrize("bnk", [(1, 1, 128), (3, 257, 128), (64, 1000, 128), (2, 33, 1), (2, 9, 37), (1, 5, 1024)])
def test_head_select_vs_fp64(bnk, obj_last):
    """Wide rows (ldh > 3K) with all three slices at non-zero, unaligned offsets; objects 0 and 20 of a 21-object table."""
    from autoposeestimation_amd import engine as E
    b, n, k = bnk
    g = _gen("head", b, n, k, obj_last)
    offs = (3, 3 + k + 5, 3 + 2 * k + 7)
    ldh = offs[2] + k + 2
    h = torch.randn(b * n, ldh, generator=g)
    weights = _head_weights(k, g)
    obj = torch.tensor([((i + int(obj_last)) % 2) * (NUM_OBJ - 1) for i in range(b)], dtype=torch.int64)
    got = E.head_select(h.cuda(), *offs, *(t.cuda() for t in weights), obj.cuda(), b, n, k).cpu()
    assert got.shape == (b, n, 8)
    val, mag = _head_ref(h, ldh, offs, weights, obj, b, n, k)
    _check_heads(got, val, mag, True)


@pytest.mark.parametrize("b", [1, 5, 64])
def test_head_select_refiner_form(b):
    """PoseRefineNet's call (network.py:577): n = 1, off_c = 0, wc = bc = None -> column 7 exactly 0."""
    from autoposeestimation_amd import engine as E
    k = 128
    g = _gen("headref", b)
    h = torch.randn(b, 2 * k, generator=g)
    wr, br, wt, bt, _, _ = _head_weights(k, g, wc_on=False)
    obj = torch.tensor([(i * 7) % NUM_OBJ for i in range(b)], dtype=torch.int64)
    got = E.head_select(h.cuda(), 0, k, 0, wr.cuda(), br.cuda(), wt.cuda(), bt.cuda(), None, None, obj.cuda(), b, 1, k).cpu()
    val, mag = _head_ref(h, 2 * k, (0, k, 0), (wr, br, wt, bt, None, None), obj, b, 1, k)
    _check_heads(got, val, mag, False)


def test_head_select_saturated_confidence():
    """Confidence logits of +-100 (and +-1000): sigmoid is exactly 1 or 0 in fp32, never NaN (expf(100) = inf -> 1 / inf = 0)."""
    from autoposeestimation_amd import engine as E
    b, n, k = 2, 300, 128
    g = _gen("headsat")
    h = torch.randn(b * n, 3 * k, generator=g)
    wr, br, wt, bt, wc, bc = _head_weights(k, g)
    sign = torch.where(torch.rand(b * n, generator=g) < 0.5, -1.0, 1.0)
    h[:, 2 * k] = sign * torch.where(torch.arange(b * n) % 3 == 0, 10.0, 1.0)
    wc.zero_()
    wc[:, 0] = 100.0
    bc.zero_()
    obj = torch.tensor([3, NUM_OBJ - 1])
    got = E.head_select(h.cuda(), 0, k, 2 * k, wr.cuda(), br.cuda(), wt.cuda(), bt.cuda(), wc.cuda(), bc.cuda(), obj.cuda(), b, n, k).cpu()
    want = (sign > 0).float().view(b, n)
    assert torch.equal(got[..., 7], want)
    val, mag = _head_ref(h, 3 * k, (0, k, 2 * k), (wr, br, wt, bt, wc, bc), obj, b, n, k)
    _check_heads(got, val, mag, True)


def test_head_select_launch_limits():
    """K = 1025 exceeds the LDS slice (8 x 1024 floats) and is refused; n = 0 returns APE_OK and writes nothing."""
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    g = _gen("headlim")
    k = 1025
    h = torch.randn(2, 3 * k, generator=g).cuda()
    wr, br, wt, bt, wc, bc = (t.cuda() for t in _head_weights(k, g))
    obj = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.ApeError, match="code -1"):
        E.head_select(h, 0, k, 2 * k, wr, br, wt, bt, wc, bc, obj, 1, 2, k)
    out = torch.full((1, 4, 8), 12345.0, device="cuda")
    lib = _lib.lib()
    rc = lib.ape_head_select_f32(_lib.dptr(h), 3 * 128, 0, 128, 256, _lib.dptr(wr), _lib.dptr(br), _lib.dptr(wt), _lib.dptr(bt),
                                 _lib.dptr(wc), _lib.dptr(bc), _lib.dptr(obj), _lib.dptr(out), 1, 0, 128, E._st())
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all())


# ---- pose_select ------------------------------------------------------------------------------------------------------
TIE_PATTERNS = ("none", "lanes", "stride", "all_equal", "last")


def _plant(c, pattern, n):
    """Plant the maximum confidence 0.9 at several indices (c itself lies in [0, 0.5))."""
    if n == 1 or pattern == "none":
        return
    if pattern == "all_equal":
        c[:] = 0.75
        return
    if pattern == "lanes":          # equal maxima in two different threads of the 256-wide first pass
        idx = [300, 45] if n > 300 else [n - 1, (n - 1) // 2]
    elif pattern == "stride":       # equal maxima in one thread's stride (i and i + 256)
        idx = [5, 261] if n > 261 else ([0, 256] if n > 256 else [n - 1, n // 3])
    else:                           # the maximum at n-1 alone
        idx = [n - 1]
    c[idx] = 0.9


def _select_inputs(b, n):
    g = _gen("select", b, n)
    heads = torch.empty(b, n, 8)
    patterns = []
    for i in range(b):
        scale = (1e-3, 1.0, 1e3)[i % 3]                  # unnormalised quaternions of norm ~1e-3, ~1, ~1e3
        heads[i, :, 0:4] = torch.randn(n, 4, generator=g) * scale
        heads[i, :, 4:7] = torch.randn(n, 3, generator=g) * 0.05
        c = torch.rand(n, generator=g) * 0.5
        pattern = TIE_PATTERNS[(i + n) % len(TIE_PATTERNS)]
        _plant(c, pattern, n)
        patterns.append(pattern)
        heads[i, :, 7] = c
    pts4 = torch.randn(b, n, 4, generator=g) * 0.3
    pts4[..., 2] += 1.0
    pts4[..., 3] = torch.randn(b, n, generator=g)          # the pad lane is never read
    return heads, pts4, patterns


@pytest.mark.parametrize("b", [1, 7, 64])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 4097])
def test_pose_select_vs_oracle(n, b):
    from autoposeestimation_amd import engine as E
    heads, pts4, _ = _select_inputs(b, n)
    dh, dp = heads.cuda(), pts4.cuda()
    pose, which, newp = E.pose_select(dh, dp)
    pose2, which2, none = E.pose_select(dh, dp, want_new_points=False)
    assert none is None
    assert torch.equal(pose, pose2) and torch.equal(which, which2)
    pose, which, newp = pose.cpu(), which.cpu(), newp.cpu()
    c = heads[..., 7]
    want_which = torch.max(c, 1)[1]
    assert torch.equal(want_which, torch.from_numpy(np.argmax(c.numpy(), 1)))     # the first maximum, on the CPU
    assert torch.equal(which.long(), want_which)
    assert bool((newp[..., 3] == 0).all())
    for i in range(b):
        pr, pt, pc = heads[i:i + 1, :, 0:4], heads[i:i + 1, :, 4:7], heads[i:i + 1, :, 7:8]
        cloud = pts4[i:i + 1, :, :3].contiguous()
        _, my_r, my_t = O.estimator_prediction(pr, pt, pc, n, 1, cloud)
        np.testing.assert_allclose(pose[i, :4].numpy(), my_r.astype(np.float64), rtol=0, atol=1e-7)
        # t = points[which] + pred_t[which]: one fp32 add on both sides
        assert np.array_equal(pose[i, 4:].numpy(), my_t.astype(np.float64))
        want_new = O.get_new_points(pr, pt, pc, cloud)[0].double()
        # (p - t) . R in fp32: <= 3u per term of sum_i |d_i R_ij| <= sqrt(3) max|d| on each side
        scale = (cloud[0].double() - torch.from_numpy(my_t).double()).abs().max().item()
        err = (newp[i, :, :3].double() - want_new).abs().max().item()
        assert err <= 1e-6 * scale, (i, err, scale)


# ---- pose_compose -----------------------------------------------------------------------------------------------------
def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _qaxis(axis, deg):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    h = np.radians(deg) / 2
    return np.concatenate([[np.cos(h)], np.sin(h) * axis])


def _branch(my_r, ref_r):
    """Which branch of quaternion_from_matrix_precise the reference composition takes: 'trace', 0, 1 or 2; and whether its w comes
    out negative before the sign flip."""
    m1 = O.quaternion_matrix(my_r)
    q2 = ref_r / np.float32(np.sqrt(((ref_r[0] * ref_r[0] + ref_r[1] * ref_r[1]) + ref_r[2] * ref_r[2]) + ref_r[3] * ref_r[3]))
    M = m1 @ O.quaternion_matrix(q2)
    if np.trace(M) > M[3, 3]:
        return "trace", False
    i, j, k = 0, 1, 2
    if M[1, 1] > M[0, 0]:
        i, j, k = 1, 2, 0
    if M[2, 2] > M[i, i]:
        i, j, k = 2, 0, 1
    return i, (M[k, j] - M[j, k]) < 0


def _compose_check(pose0, ref_r, ref_t, got):
    """got[B,7] vs refined_prediction row by row: 1e-12 on q, 1e-12 max(1, |t|) on t; q up to sign where the reference's w is 0
    to rounding (an exact 180-degree composition leaves the sign to the last bit of M[k][j] - M[j][k])."""
    for i in range(pose0.shape[0]):
        my_r, my_t = pose0[i, :4].copy(), pose0[i, 4:].copy()
        _, r, t = O.refined_prediction(torch.from_numpy(ref_r[i].copy()), torch.from_numpy(ref_t[i].copy()), my_r, my_t)
        q = got[i, :4]
        if abs(r[0]) < 1e-9:
            err = min(np.abs(q - r).max(), np.abs(q + r).max())
        else:
            err = np.abs(q - r).max()
        assert err <= 1e-12, (i, q, r)
        assert np.abs(got[i, 4:] - t).max() <= 1e-12 * max(1.0, np.abs(t).max()), (i, got[i, 4:], t)


def _run_compose(pose0, ref_r, ref_t, strided):
    from autoposeestimation_amd import engine as E
    b = pose0.shape[0]
    pose = torch.from_numpy(pose0.copy()).cuda()
    if strided:                     # the pipeline passes the refiner's [B, 8] output as out[:, 0:4], out[:, 4:7]
        out = torch.zeros(b, 8, device="cuda")
        out[:, 0:4] = torch.from_numpy(ref_r).cuda()
        out[:, 4:7] = torch.from_numpy(ref_t).cuda()
        rr, rt = out[:, 0:4], out[:, 4:7]
        assert rr.stride(0) == 8 and rt.stride(0) == 8
    else:
        rr, rt = torch.from_numpy(ref_r).cuda(), torch.from_numpy(ref_t).cuda()
    E.pose_compose(pose, rr, rt)
    return pose.cpu().numpy()


@pytest.mark.parametrize("b", [1, 63, 64, 65, 1000])
def test_pose_compose_random_vs_oracle(b):
    rng = np.random.default_rng(_seed(11, b))
    my_r = rng.standard_normal((b, 4))
    my_r /= np.linalg.norm(my_r, axis=1, keepdims=True)
    pose0 = np.concatenate([my_r, rng.standard_normal((b, 3)) * 0.5], 1)
    scale = np.array([1e-3, 1.0, 7.0, 1e3])[np.arange(b) % 4][:, None]
    ref_r = (rng.standard_normal((b, 4)) * scale).astype(np.float32)          # unnormalised, as the refiner emits it
    ref_t = (rng.standard_normal((b, 3)) * 0.02).astype(np.float32)
    got = _run_compose(pose0, ref_r, ref_t, strided=True)
    _compose_check(pose0, ref_r, ref_t, got)


def test_pose_compose_every_branch():
    """Compositions built to land in each branch of quaternion_from_matrix_precise: trace > 0, the else branch with i = 0, 1, 2
    (150-180 degrees about x, y, z, including exactly 180), w negative before the sign flip, the identity.  Half the rows compose
    through a random first pose (ref_r = my_r^-1 (x) target), half through the identity."""
    rng = np.random.default_rng(5)
    targets = [_qaxis([1, 0, 0], 0), _qaxis([0.3, -0.5, 0.8], 40), _qaxis([1, 2, 3], 110)]
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0.1, -0.05], [0.05, 1, 0.1], [-0.1, 0.05, 1]):
        for deg in (150, 165, 179.5, -160, -175):
            targets.append(_qaxis(axis, deg))
    rows_r, rows_q = [], []
    for k, tq in enumerate(targets):
        for through_identity in (True, False):
            if through_identity:
                my = np.array([1.0, 0.0, 0.0, 0.0])
            else:
                my = rng.standard_normal(4)
                my /= np.linalg.norm(my)
            rel = _qmul(my * np.array([1, -1, -1, -1]), tq)                  # my^-1 (x) target
            s = (0.01, 1.0, 300.0)[k % 3]
            rows_r.append(my)
            rows_q.append((rel * s).astype(np.float32))
    # exactly 180 degrees about x, y, z: identity first pose, ref_r exactly (0, 3, 0, 0) etc. (|r| = 3 is exact in fp32)
    for a in range(3):
        e = np.zeros(4, np.float32)
        e[1 + a] = 3.0
        rows_r.append(np.array([1.0, 0.0, 0.0, 0.0]))
        rows_q.append(e)
    rows_r.append(np.array([1.0, 0.0, 0.0, 0.0]))                            # identity o identity
    rows_q.append(np.array([2.0, 0.0, 0.0, 0.0], np.float32))
    b = len(rows_r)
    my_r = np.stack(rows_r)
    pose0 = np.concatenate([my_r, rng.standard_normal((b, 3)) * 0.4], 1)
    ref_r = np.stack(rows_q)
    ref_t = (rng.standard_normal((b, 3)) * 0.03).astype(np.float32)
    branches = [_branch(pose0[i, :4], ref_r[i]) for i in range(b)]
    reached = {br for br, _ in branches}
    assert reached == {"trace", 0, 1, 2}, reached                            # the data really reaches every branch
    assert any(neg for _, neg in branches)
    for strided in (False, True):
        got = _run_compose(pose0, ref_r, ref_t, strided)
        _compose_check(pose0, ref_r, ref_t, got)
    assert np.array_equal(got[b - 1, :4], [1.0, 0.0, 0.0, 0.0])


# ---- pose_recentre / recentre_qt --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("bn", [(1, 1), (3, 255), (64, 257), (64, 1000)])
def test_pose_recentre_vs_fp64(bn, scale):
    """eval_ycb.py:205-210: R = quaternion_matrix(my_r)[:3, :3].astype(float32), T = my_t.astype(float32), new = (cloud - T) @ R.
    fp64 of exactly those fp32 R and T; the kernel's fp32 (p - t) . R carries <= ~4u sqrt(3) max|p - t| per element."""
    from autoposeestimation_amd import engine as E
    b, n = bn
    rng = np.random.default_rng(_seed(21, b, n, scale))
    q = rng.standard_normal((b, 4)) * np.array([1.0, 0.5, 2.0, 1e-3])[np.arange(b) % 4][:, None]
    t = rng.standard_normal((b, 3)) * scale
    pose = np.concatenate([q, t], 1)
    pts = np.zeros((b, n, 4), np.float32)
    pts[..., :3] = t[:, None, :] + rng.standard_normal((b, n, 3)) * 0.2 * scale
    pts[..., 3] = 5.0
    got = E.pose_recentre(torch.from_numpy(pts).cuda(), torch.from_numpy(pose).cuda()).cpu().numpy()
    assert np.all(got[..., 3] == 0)
    for i in range(b):
        R = O.quaternion_matrix(pose[i, :4])[:3, :3].astype(np.float32).astype(np.float64)
        t32 = pose[i, 4:].astype(np.float32).astype(np.float64)
        d = pts[i, :, :3].astype(np.float64) - t32
        want = d @ R
        err = np.abs(got[i, :, :3] - want).max()
        assert err <= 1e-6 * np.abs(d).max(), (i, err, np.abs(d).max())


@pytest.mark.parametrize("qscale", [1e-3, 2.5, 1e3])
@pytest.mark.parametrize("n", [1, 500, 2621, 300001])
def test_recentre_qt_vs_quat_to_base(n, qscale):
    """loss.py:61-69: q = pred_r / torch.norm(pred_r) and ori_base in fp32 (oracle quat_to_base), then (pts - t) @ base in fp64.
    n = 300001 runs the 1024-workgroup grid-stride loop."""
    from autoposeestimation_amd import engine as E
    g = _gen("rqt", n, qscale)
    qt = torch.empty(7)
    qt[:4] = torch.randn(4, generator=g) * qscale
    qt[4:] = torch.randn(3, generator=g) * 0.1
    pts = torch.randn(n, 3, generator=g) * 0.3
    got = E.recentre_qt(pts.cuda(), qt.cuda()).cpu().double()
    q = qt[:4] / torch.norm(qt[:4])
    base = O.quat_to_base(q).double()
    d = pts.double() - qt[4:].double()
    want = d @ base
    err = (got - want).abs().max().item()
    assert err <= 1e-6 * d.abs().max().item(), err


# ---- adds_select ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", TIE_PATTERNS + ("tiny",))
@pytest.mark.parametrize("with_points", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 5000])
def test_adds_select_vs_fp64(n, with_points, pattern):
    """which / dis[which] / q / t are copies (t: one fp32 add of points[which]): bitwise.  The loss is a 256-thread fp32 sum of
    positive terms ((dis + 2 std) c > 0, -w log c > 0 for c in (0, 1)): <= (N/256 + 9) u of the sum, within 1e-5 mean|term|."""
    from autoposeestimation_amd import engine as E
    g = _gen("adds", n, with_points, pattern)
    dis = torch.rand(n, generator=g) * 0.1
    std = torch.rand(n, generator=g) * 0.02
    r = torch.randn(n, 4, generator=g)
    t = torch.randn(n, 3, generator=g) * 0.05
    pts = torch.randn(n, 3, generator=g) * 0.3 if with_points else None
    if pattern == "tiny":           # confidences down to 1e-30: the -w log c term dominates
        c = 10.0 ** (-30 * torch.rand(n, generator=g))
        c[n // 2] = 0.9
    else:
        c = 0.05 + torch.rand(n, generator=g) * 0.45
        _plant(c, pattern, n)
    w = 0.015625                    # exact in fp32: the kernel takes w as a float
    out, which = E.adds_select(dis.cuda(), std.cuda(), c.cuda(), r.cuda(), t.cuda(), None if pts is None else pts.cuda(), w)
    out, which = out.cpu(), int(which.cpu()[0])
    want = int(np.argmax(c.numpy()))
    assert want == int(torch.max(c.view(1, n), 1)[1][0])
    assert which == want
    assert out[1].item() == dis[want].item()
    assert torch.equal(out[2:6], r[want])
    assert torch.equal(out[6:9], t[want] + pts[want] if pts is not None else t[want])
    term = (dis.double() + 2 * std.double()) * c.double() - w * torch.log(c.double())
    assert abs(out[0].item() - term.mean().item()) <= 1e-5 * term.abs().mean().item()


# ---- log_softmax_rows -------------------------------------------------------------------------------------------------
def _check_log_softmax(x):
    from autoposeestimation_amd import engine as E
    got = E.log_softmax_rows(x.cuda()).cpu().double()
    want = F.log_softmax(x.double(), -1)
    ninf = torch.isneginf(want)
    assert torch.equal(torch.isneginf(got), ninf)
    assert bool(torch.isfinite(got[~ninf]).all())
    # max-subtracted fp32: u |x - m| from the subtraction, ~sqrt(C) u from the sum of exps, 1 ulp each from expf / logf
    err = (got[~ninf] - want[~ninf]).abs()
    tol = 1e-6 * (1 + want[~ninf].abs())
    assert bool((err <= tol).all()), float((err / tol).max())
    return got, want


@pytest.mark.parametrize("rows", [1, 255, 64000])
@pytest.mark.parametrize("c", [1, 2, 13, 32, 64, 100])
def test_log_softmax_rows_vs_fp64(c, rows):
    """Rows offset by 0, +80, -80 and 1e4 in turn (exp(1e4) overflows without the max-subtraction)."""
    g = _gen("lsm", c, rows)
    x = torch.randn(rows, c, generator=g) * 3
    x += torch.tensor([0.0, 80.0, -80.0, 1e4])[torch.arange(rows) % 4].view(rows, 1)
    got, _ = _check_log_softmax(x)
    if c == 1:
        assert bool((got == 0).all())


@pytest.mark.parametrize("c", [1, 2, 13, 32, 64, 100])
def test_log_softmax_rows_equal_values(c):
    x = torch.tensor([0.0, -3.5, 80.0, 1e4, -1e4]).view(5, 1).expand(5, c).contiguous()
    got, _ = _check_log_softmax(x)
    assert (got + np.log(c)).abs().max().item() <= 1e-6 * (1 + np.log(c))


@pytest.mark.parametrize("c", [2, 13, 32, 64, 100])
def test_log_softmax_rows_neg_inf(c):
    """-inf entries stay -inf (exp(-inf - m) = 0), the rest stays finite, as F.log_softmax; every row keeps one finite entry."""
    g = _gen("lsminf", c)
    rows = 255
    x = torch.randn(rows, c, generator=g) * 4
    x[torch.rand(rows, c, generator=g) < 0.3] = float("-inf")
    x[torch.arange(rows), torch.randint(0, c, (rows,), generator=g)] = torch.randn(rows, generator=g)
    x[0, :] = 1.0
    x[0, c - 1] = float("-inf")                     # -inf last
    x[1, :] = float("-inf")
    x[1, 0] = 2.0                                    # one finite entry: log_softmax = 0 there
    got, _ = _check_log_softmax(x)
    assert got[1, 0].item() == 0.0


def test_log_softmax_rows_grid_stride():
    """More rows than the 8192 x 256-thread grid: the grid-stride loop covers the rest."""
    g = _gen("lsmbig")
    x = torch.randn(8192 * 256 + 1001, 2, generator=g)
    _check_log_softmax(x)


# ---- gather_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 5, 4), (2, 17, 33, 4), (3, 1000, 500, 1024), (4, 3000, 2100, 1024)])
def test_gather_rows_bitwise(shape):
    """y[b, i] = x[b, index[b, i]]; includes rows 0 and rows_in-1 and repeats.  (4, 3000, 2100, 1024) exceeds one grid."""
    from autoposeestimation_amd import engine as E
    b, rin, n, c = shape
    g = _gen("gather", *shape)
    x = torch.randn(b, rin, c, generator=g)
    idx = torch.randint(0, rin, (b, n), generator=g)
    idx[:, 0] = 0
    idx[:, -1] = rin - 1
    if n > 3:
        idx[:, 2] = idx[:, 3]
    got = E.gather_rows(x.cuda(), idx.cuda()).cpu()
    want = torch.stack([x[i][idx[i]] for i in range(b)])
    assert torch.equal(got, want)


def test_gather_rows_clamps_bad_indices():
    """ops.hip gather_rows_kernel: an index < 0 reads row 0, one >= rows_in reads row rows_in-1."""
    from autoposeestimation_amd import engine as E
    b, rin, c = 2, 9, 8
    x = torch.randn(b, rin, c, generator=_gen("gclamp"))
    idx = torch.tensor([[-1, -7, rin, rin + 5, 2 ** 40, -2 ** 40, 0, rin - 1, 4]] * b)
    idx[1, 8] = 2
    got = E.gather_rows(x.cuda(), idx.cuda()).cpu()
    want = torch.stack([x[i][idx[i].clamp(0, rin - 1)] for i in range(b)])
    assert torch.equal(got, want)


def test_gather_rows_empty_is_noop():
    """n = 0 through the C ABI (the engine wrapper's empty tensors would hand it null data pointers, which it refuses): APE_OK and a
    sentinel-filled output left untouched."""
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    x = torch.randn(2, 5, 8, device="cuda")
    idx = torch.zeros(2, 4, dtype=torch.int64, device="cuda")
    y = torch.full((2, 4, 8), -3.0, device="cuda")
    assert _lib.lib().ape_gather_rows_f32(_lib.dptr(x), _lib.dptr(idx), _lib.dptr(y), 2, 5, 0, 8, E._st()) == 0
    torch.cuda.synchronize()
    assert bool((y == -3.0).all())


# ---- maxpool3x3s2 -----------------------------------------------------------------------------------------------------
def _maxpool_case(b, h, w, c, kind, g):
    if kind == "randn":
        x = torch.randn(b, h, w, c, generator=g)
    elif kind == "negative":        # all < 0: padding read as 0 instead of -inf would show
        x = -1.0 - torch.rand(b, h, w, c, generator=g)
    else:                           # few distinct values: ties everywhere
        x = torch.randint(-3, 1, (b, h, w, c), generator=g).float()
    from autoposeestimation_amd import engine as E
    got = E.maxpool3x3s2(x.cuda()).cpu()
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert got.shape == want.shape
    assert torch.equal(got, want), (b, h, w, c, kind)


@pytest.mark.parametrize("w", [1, 4, 7])
@pytest.mark.parametrize("h", [1, 2, 3, 4, 5])
def test_maxpool3x3s2_small_maps(h, w):
    """Bitwise F.max_pool2d(x, 3, 2, 1).  NaN inputs are out of scope: fmaxf drops a NaN that torch propagates."""
    g = _gen("mp", h, w)
    for c in (4, 64, 68):
        for kind in ("randn", "negative", "ties"):
            _maxpool_case(2, h, w, c, kind, g)


@pytest.mark.parametrize("shape", [(2, 61, 77, 64), (1, 240, 320, 64), (7, 240, 320, 68)])
def test_maxpool3x3s2_maps(shape):
    """61 x 77 (odd), the Unet stem's 240 x 320 output, and 7 x 240 x 320 x 68 (more work than one 8192-workgroup grid)."""
    g = _gen("mpbig", *shape)
    for kind in ("randn", "negative", "ties"):
        _maxpool_case(*shape, kind, g)


# ---- adaptive_avgpool (single size) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3, 5, 6, 7, 8])
@pytest.mark.parametrize("shape", [(2, 13, 17, 8), (1, 3, 5, 4), (1, 1, 1, 4), (2, 7, 24, 12), (1, 20, 30, 260)])
def test_adaptive_avgpool_vs_fp64(shape, s):
    """Bins [floor(o H / S), ceil((o+1) H / S)) as ATen: S not dividing H, W; S > H (bins repeat rows); 1 x 1; C = 260 leaves a
    ragged 64-float4 channel chunk.  Four waves sum a bin's pixels in fp32, so the mean carries ~sqrt(npx / 4) u max|x|."""
    from autoposeestimation_amd import engine as E
    b, h, w, c = shape
    x = torch.randn(b, h, w, c, generator=_gen("aap", s, *shape)) + 0.5
    got = E.adaptive_avgpool(x.cuda(), s).cpu().double()
    want = F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), s).permute(0, 2, 3, 1)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= 2e-6 * x.abs().max().item()


@pytest.mark.parametrize("s", [1, 6])
def test_adaptive_avgpool_large_bin(s):
    """60 x 80 at S = 1: 4 800 pixels per bin split over 4 waves (the PSP module's map, pspnet.py:15)."""
    from autoposeestimation_amd import engine as E
    x = torch.randn(2, 60, 80, 64, generator=_gen("aapbig", s)) + 1.0
    got = E.adaptive_avgpool(x.cuda(), s).cpu().double()
    want = F.adaptive_avg_pool2d(x.double().permute(0, 3, 1, 2), s).permute(0, 2, 3, 1)
    assert (got - want).abs().max().item() <= 2e-6 * x.abs().max().item()

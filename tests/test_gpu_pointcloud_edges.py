"""GPU checks of the point-cloud kernels (csrc/pointcloud.hip) at their edge shapes, against the float64 restatement
(tests/pointcloud_reference.py) on the inputs of tests/pointcloud_edge_cases.py -- whose guards and branch-reached claims
tests/test_pointcloud_host.py proves on the CPU.

Bit for bit: surface points, keys / order / sorted / origin, voxel means, counts, k-NN means, nn1 index and d^2, selections and indices,
Mahalanobis with an injected (mu, Cinv), transform and concat, status words and the T == init cases.
Derived bounds, nothing measured: moments and ICP sums within (n + 1) 2^-53 sum|term| of math.fsum (any summation order); normals, for
EVERY point of every case: unit norm to 1e-12, n_z >= 0, n^T C n <= lambda_min + 1e-12 lambda_max with C from the restatement's
selection (1e-12 is ~4500 eps, room for the 36 Jacobi rotations, and six orders below what a wrong selection costs), and
1 - |cos| <= 1e-12 where lambda_1 - lambda_0 >= 1e-3 lambda_max; one ICP update within 1e-9 max(1, |coordinates|) of the restatement's.

Sizes: a few hundred points, except the sort cases (up to 2^20 + 1 points, 25 MB) and the 131 072 / 131 073-row reductions."""
import time

import numpy as np
import pytest
import torch

import pointcloud_edge_cases as EC
import pointcloud_reference as R

pytestmark = pytest.mark.gpu
_D = torch.float64
EINVAL, EWORKSPACE = -1, -3


def _mods():
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    return _lib, B, PC


def _dev(a, dtype=_D):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def _cloud(pts, normals=None):
    _, _, PC = _mods()
    pc = PC.PointCloud(np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3))
    if normals is not None:
        pc._n = _dev(normals)
    return pc


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _assert_grid(g, want):
    assert _same(g["origin"].cpu().numpy(), want["origin"])
    assert _same(g["order"].cpu().numpy().astype(np.uint32), want["order"])
    assert _same(g["keys"].cpu().numpy().view(np.uint64), want["keys"])
    assert _same(g["sorted"].cpu().numpy(), want["sorted"])


# ---- surface points -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", EC.SURFACE_SHAPES)
def test_surface_points_bit_equal(shape):
    _, B, _ = _mods()
    views, kinds = EC.surface_batch(shape)
    got = B.surface_points(views, None)
    assert len(got) == len(views)
    for (label, depth, T, intr), kind, pc in zip(views, kinds, got):
        want = R.surface_points(label, depth, intr, T)
        assert _same(np.array(pc.points).reshape(-1, 3), want), (shape, kind)
        assert len(pc) == (0 if kind == "zero" else len(want))
    if len(views) > 16:                                   # a view's cloud does not depend on its slot: the 17th alone
        alone = B.surface_points(views[16:], None)[0]
        assert torch.equal(alone._p, got[16]._p)


# ---- sort / grid build ------------------------------------------------------------------------------------------------------------------------
SMALL_SORT = [n for n in EC.SORT_CASES if n not in EC.SORT_LARGE]


@pytest.mark.parametrize("name", SMALL_SORT)
def test_grid_build_bit_equal(name):
    pts, cell, _, _ = EC.sort_case(name)
    _assert_grid(_cloud(pts)._grid(cell), R.grid(pts, cell, cell))


def test_grid_build_in_one_list_equals_each_alone():
    _, B, _ = _mods()
    cases = [EC.sort_case(n) for n in SMALL_SORT]
    grids = B.build_grids([_cloud(c[0]) for c in cases], 1.0)
    assert len(grids) == len(cases) and len({c[1] for c in cases}) == 1
    for g, c in zip(grids, cases):
        _assert_grid(g, R.grid(c[0], 1.0, 1.0))


@pytest.mark.parametrize("name", EC.SORT_LARGE)
def test_grid_build_large_bit_equal(name):
    pts, cell, _, _ = EC.sort_case(name)
    want = R.grid(pts, cell, cell)
    pc = _cloud(pts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = pc._grid(cell)
    torch.cuda.synchronize()
    print("sort %s: %d points in %.3f s" % (name, len(pts), time.perf_counter() - t0))
    _assert_grid(g, want)


# ---- voxel down-sample --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.VOXEL_CASES))
def test_voxel_down_sample_bit_equal(name):
    pts, voxel, _ = EC.voxel_case(name)
    got = _cloud(pts).voxel_down_sample(voxel)
    assert _same(got._p.cpu().numpy(), R.voxel_down_sample(pts, voxel))


def test_voxel_down_sample_in_one_list_equals_each_alone():
    _, B, _ = _mods()
    names = [n for n in EC.VOXEL_CASES if EC.VOXEL_CASES[n][1] == 0.5]
    got = B.voxel_down_sample([_cloud(EC.voxel_case(n)[0]) for n in names], 0.5)
    for n, pc in zip(names, got):
        assert _same(pc._p.cpu().numpy(), R.voxel_down_sample(EC.voxel_case(n)[0], 0.5)), n


# ---- radius count + selection ---------------------------------------------------------------------------------------------------------------------
def _counts(pc, r, queries):
    _lib, B, _ = _mods()
    g = pc._grid(r)
    q = _dev(queries)
    cnt = torch.full((len(queries),), -7, dtype=torch.int32, device="cuda")
    _lib.call.ape_grid_query_batch_f64(0, 1, *B._grid_args([g]), float(r), B._ptrs([q]), B._ints([len(queries)]), float(r), 0, B._ptrs([cnt]), None, None,
                                       B._st())
    return cnt.cpu().numpy()


@pytest.mark.parametrize("name", list(EC.RADIUS_CASES))
def test_radius_count_and_selection_bit_equal(name):
    pts, r, q, _ = EC.radius_case(name)
    queries = pts if q is None else q
    pc = _cloud(pts)
    want = R.radius_count(R.grid(pts, r, r), queries, r)
    assert _same(_counts(pc, r, queries), want)
    if q is not None:
        return
    c = int(np.sort(want)[len(want) // 2])
    for nb_points in (c - 1, c, c + 1):                   # strict >
        kept, idx = pc.remove_radius_outlier(nb_points, r)
        keep = R.select(0, want, nb_points)
        assert idx == keep.tolist() and _same(kept._p.cpu().numpy(), pts[keep])


def test_radius_outlier_of_17_clouds_equals_each_alone():
    _, B, _ = _mods()
    arrays = [EC.shuffled(EC.lattice(2 + i % 4, 3, 2 + i % 3), 500 + i) for i in range(15)] + [EC.radius_case("duplicates")[0], np.array([[0.5, 0.5, 0.5]])]
    clouds = [_cloud(a) for a in arrays]
    assert len(clouds) == 17
    got, idx = B.remove_radius_outlier(clouds, 9, 1.5, indices=True)
    for a, c, pc, kept in zip(arrays, clouds, got, idx):
        keep = R.select(0, R.radius_count(R.grid(a, 1.5, 1.5), a, 1.5), 9)
        assert kept == keep.tolist() and _same(pc._p.cpu().numpy(), a[keep])
        alone, alone_idx = c.remove_radius_outlier(9, 1.5)
        assert alone_idx == kept and torch.equal(alone._p, pc._p)
    assert any(len(k) for k in idx) and any(len(k) < len(a) for k, a in zip(idx, arrays))


# ---- normals --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.NORMAL_CASES))
def test_normals_within_the_derived_bounds_no_point_left_out(name):
    c = EC.normal_case(name)
    for max_nn in c["max_nns"]:
        pc = _cloud(c["pts"]).estimate_normals(radius=c["radius"], max_nn=max_nn)
        got = pc._n.cpu().numpy()
        assert got.shape == c["pts"].shape
        for i, (n, (sel, cnt, C, lam)) in enumerate(zip(got, EC.normal_expected(name, max_nn))):
            where = (name, max_nn, i, cnt)
            if cnt < 3:
                assert n.tolist() == [0.0, 0.0, 1.0], where
                continue
            assert abs(float(np.linalg.norm(n)) - 1.0) <= 1e-12 and n[2] >= 0, where
            assert float(n @ C @ n) <= lam[0] + 1e-12 * lam[2], (where, float(n @ C @ n), lam)
            if lam[1] - lam[0] >= 1e-3 * lam[2]:
                want = np.linalg.eigh(C)[1][:, 0]
                assert 1.0 - abs(float(n @ want)) <= 1e-12, where


def test_normals_in_one_list_equal_each_alone():
    _, B, _ = _mods()
    names = [n for n in EC.NORMAL_CASES if EC.NORMAL_CASES[n][1] == 1.0] * 3
    clouds = B.estimate_normals([_cloud(EC.normal_case(n)["pts"]) for n in names[:17]], 1.0, 30)
    assert len(clouds) == 17
    for n, pc in zip(names, clouds):
        alone = _cloud(EC.normal_case(n)["pts"]).estimate_normals(radius=1.0, max_nn=30)
        assert torch.equal(alone._n, pc._n), n


# ---- k-NN mean distance ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.KNN_CASES))
def test_knn_mean_bit_equal(name):
    _lib, B, _ = _mods()
    c = EC.knn_case(name)
    pc = _cloud(c["pts"])
    n = len(pc)
    g = pc._grid(c["cell"])
    for k in c["ks"]:
        want = R.knn_mean(c["pts"], k)
        a = torch.full((n,), -7.0, dtype=_D, device="cuda")
        b = torch.full((n,), -7.0, dtype=_D, device="cuda")
        _lib.call.ape_knn_mean_dist_f64(_lib.dptr(pc._p, _D), n, k, _lib.dptr(a), B._st())
        _lib.call.ape_grid_query_batch_f64(2, 1, *B._grid_args([g]), float(c["cell"]), None, None, 0.0, k, None, None, B._ptrs([b]), B._st())
        assert _same(a.cpu().numpy(), want), (name, k, "all pairs")
        assert _same(b.cpu().numpy(), want), (name, k, "grid")


# ---- statistical filter ---------------------------------------------------------------------------------------------------------------------------
def _stat_expected(pts, nb, ratio):
    means = R.knn_mean(pts, min(nb, len(pts)))
    return R.select(1, means, R.statistical_threshold(means, ratio))


def test_statistical_filter_bit_equal():
    _, B, _ = _mods()
    cases = EC.stat_cases()
    for pts, nb, ratio, kept in cases:
        got, idx = _cloud(pts).remove_statistical_outlier(nb, ratio)
        keep = _stat_expected(pts, nb, ratio)
        assert idx == keep.tolist() and _same(got._p.cpu().numpy().reshape(-1, 3), pts[keep])
        if kept is not None:
            assert idx == kept
    # clouds that differ in (cell, k) inside one call: k = min(8, n), the cell derived from each cloud's own extent
    clouds = [_cloud(c[0]) for c in cases]
    ratios = [c[2] for c in cases]
    assert len({min(8, len(c[0])) for c in cases}) > 1
    got, idx = B.remove_statistical_outlier(clouds, 8, ratios, indices=True)
    for c, pc, kept in zip(cases, got, idx):
        keep = _stat_expected(c[0], 8, c[2])
        assert kept == keep.tolist() and _same(pc._p.cpu().numpy().reshape(-1, 3), c[0][keep])


# ---- moments / Mahalanobis ------------------------------------------------------------------------------------------------------------------------
def test_moments_within_the_summation_bound():
    _lib, B, _ = _mods()
    arrays = [EC.moment_case(n) for n in EC.MOMENT_SIZES]
    clouds = [_cloud(a) for a in arrays]
    o9 = torch.zeros(len(clouds), 9, dtype=_D, device="cuda")
    ws = torch.empty(len(clouds) * 512 * 9 * 8, dtype=torch.uint8, device="cuda")
    _lib.call.ape_moments_batch_f64(len(clouds), B._ptrs([c._p for c in clouds]), B._ints([len(c) for c in clouds]), _lib.dptr(o9), _lib.dptr(ws),
                                    ws.numel(), B._st())
    got = o9.cpu().numpy()
    for a, row in zip(arrays, got):
        want, bound = R.moments_exact(a)
        print("moments n=%d: worst error / bound %.3g" % (len(a), float((np.abs(row - want) / bound).max())))
        assert (np.abs(row - want) <= bound).all(), (len(a), row - want, bound)
    mean, cov = clouds[0]._moments()                      # one point: its own mean, zero covariance
    assert _same(mean, arrays[0][0]) and not cov.any()


@pytest.mark.parametrize("count", [9, 16])
def test_mahalanobis_with_injected_moments_bit_equal(count):
    _lib, B, _ = _mods()
    arrays, mc = EC.mahalanobis_clouds(count)
    clouds = [_cloud(a) for a in arrays]
    outs = [torch.full((len(a),), -7.0, dtype=_D, device="cuda") for a in arrays]
    _lib.call.ape_mahalanobis_batch_f64(count, B._ptrs([c._p for c in clouds]), B._ints([len(a) for a in arrays]), B._dbls(mc.reshape(-1)), B._ptrs(outs),
                                        B._st())
    for a, m, o in zip(arrays, mc, outs):
        assert np.array_equal(o.cpu().numpy(), R.mahalanobis(a, m), equal_nan=True)


def test_mahalanobis_of_17_clouds_with_singular_ones():
    _, B, _ = _mods()
    arrays, _ = EC.mahalanobis_clouds(17)
    clouds = [_cloud(a) for a in arrays]
    got = B.mahalanobis(clouds)
    for a, c, m in zip(arrays, clouds, got):
        mean, cov = B.moments([c])[0]
        want = R.mahalanobis(a, np.r_[mean, B._inverse_or_nan(cov).reshape(-1)])
        assert np.array_equal(m, want, equal_nan=True)
        if len(a) == 1:
            assert np.isnan(m).all()                         # zero covariance: NaN for that cloud only
        if len(a) >= 10:
            assert np.isfinite(m).all()
        assert np.array_equal(m, c.compute_mahalanobis_distance(), equal_nan=True)


def test_a_singular_view_empties_itself_and_leaves_the_batch_alone():
    """get_surface_batch with a coplanar-lattice view and a one-point view among generic ones: np.linalg.inv used to raise for the whole
    batch; now those two views come out empty (NaN distances -> NaN std_ratio -> nothing kept, as with Eigen's inverse in the reference)
    and the others bit-equal to a run without them"""
    _, B, _ = _mods()
    views, bad = EC.singular_views()
    args = (None, 0, 5.0, 4, 1.0)
    with np.errstate(invalid="ignore"):
        full = B.get_surface_batch(views, *args)
    good = B.get_surface_batch([v for i, v in enumerate(views) if i not in bad], *args)
    assert all(len(full[i]) == 0 for i in bad)
    rest = [full[i] for i in range(len(views)) if i not in bad]
    assert len(rest) == len(good) == 3
    for a, b in zip(rest, good):
        assert len(a) > 10 and torch.equal(a._p, b._p)


# ---- transform / concat -----------------------------------------------------------------------------------------------------------------------------
def test_transform_and_concat_bit_equal():
    _, B, _ = _mods()
    rng = np.random.default_rng(110)
    T = EC.rigid(0.3, -0.2, 1.1, (500.0, 20.0, 300.0))
    for n in (0, 1, 257):
        pts, nrm = rng.uniform(-100, 100, (n, 3)), EC.unit(n, 111) if n else np.zeros((0, 3))
        plain = _cloud(pts).transform(T)
        assert _same(plain._p.cpu().numpy().reshape(-1, 3), R.transform(pts, T)) and plain._n is None
        if n:
            both = _cloud(pts, nrm).transform(T)
            wp, wn = R.transform(pts, T, nrm)
            assert _same(both._p.cpu().numpy(), wp) and _same(both._n.cpu().numpy(), wn)
        for m in (0, 1, 257):
            other = rng.uniform(-100, 100, (m, 3))
            cat = B.concat([_cloud(pts)], [_cloud(other)])[0]
            assert _same(cat._p.cpu().numpy(), np.concatenate([pts, other]))
        assert _same(B.concat([_cloud(pts)])[0]._p.cpu().numpy(), pts)
    sizes = [0, 1, 257] * 6
    clouds = [_cloud(rng.uniform(-100, 100, (n, 3))) for n in sizes[:17]]
    Ts = [EC.rigid(0.01 * i, 0.02, -0.03, (i, 2.0, 3.0)) for i in range(17)]
    want = [R.transform(c._p.cpu().numpy(), t) for c, t in zip(clouds, Ts)]
    for c, w in zip(B.transform(clouds, Ts), want):
        assert _same(c._p.cpu().numpy(), w)


# ---- ICP: correspondence search -------------------------------------------------------------------------------------------------------------------
def _nn1(target, cell, queries, max_dist):
    _lib, B, PC = _mods()
    g = _cloud(target)._grid(cell)
    q = _dev(queries)
    idx = torch.full((len(queries),), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((len(queries),), -7.0, dtype=_D, device="cuda")
    _lib.call.ape_grid_nn1_f64(*PC.PointCloud._gargs(g), _lib.dptr(q, _D), len(queries), float(max_dist), _lib.dptr(idx), _lib.dptr(d2), B._st())
    return idx.cpu().numpy(), d2.cpu().numpy()


@pytest.mark.parametrize("ns", [1, 8, 9, len(EC.NN1_QUERIES)])
def test_nn1_ties_and_thresholds_bit_equal(ns):
    q = EC.NN1_QUERIES[:ns]
    want = R.nn1(R.grid(EC.NN1_TARGET, EC.NN1_CELL, EC.NN1_CELL), q, EC.NN1_MAX_DIST)
    idx, d2 = _nn1(EC.NN1_TARGET, EC.NN1_CELL, q, EC.NN1_MAX_DIST)
    assert idx.tolist() == EC.NN1_EXPECT[:ns] == want[0].tolist() and _same(d2, want[1])


def test_nn1_one_point_target():
    tgt, q, expect = EC.NN1_ONE_TARGET
    idx, d2 = _nn1(tgt, 1.0, q, EC.NN1_MAX_DIST)
    want = R.nn1(R.grid(tgt, 1.0, 1.0), q, EC.NN1_MAX_DIST)
    assert idx.tolist() == expect == want[0].tolist() and _same(d2, want[1])


# ---- ICP: the reduced sums ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EC.SUM_SIZES)
def test_icp_sums_within_the_summation_bound(n):
    _lib, B, _ = _mods()
    c = EC.sums_case(n)
    src, tgt, tn, d2 = _dev(c["src"]), _dev(c["tgt"]), _dev(c["tn"]), _dev(c["d2"])
    corr = _dev(c["corr"], torch.int32)
    ws = torch.empty(512 * 29 * 8, dtype=torch.uint8, device="cuda")
    for kind, nv in ((0, 17), (1, 29)):
        out = torch.zeros(29, dtype=_D, device="cuda")
        _lib.call.ape_icp_sums_f64(kind, _lib.dptr(src), _lib.dptr(tgt), _lib.dptr(tn), _lib.dptr(corr), _lib.dptr(d2), n, _lib.dptr(out), _lib.dptr(ws),
                                   ws.numel(), B._st())
        got = out.cpu().numpy()[:nv]
        want, bound = R.icp_sums_exact(kind, c["src"], c["tgt"], c["tn"], c["corr"], c["d2"])
        print("icp sums kind %d n=%d: worst error / bound %.3g" % (kind, n, float((np.abs(got - want) / bound).max())))
        assert got[0] == want[0] == (c["corr"] >= 0).sum()
        assert (np.abs(got - want) <= bound).all(), (kind, n, got - want, bound)


# ---- ICP: exits of the step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EC.ICP_CASES))
def test_icp_step_exits(name):
    _, B, PC = _mods()
    c = EC.icp_case(name)
    crit = PC.ICPConvergenceCriteria(*c["crit"])
    st = B.icp_states([_cloud(c["src"])], [_cloud(c["tgt"], c["tn"])], EC.ICP_MAX_DIST, [c["init"]], c["kind"], crit)[0]
    want, _ = EC.icp_expected(name)
    e = c["expect"]
    assert st[0] == 1.0 and st[37] == e["status"] == want[37] and st[1] == e["updates"] == want[1], (name, st[[0, 1, 37]])
    assert st[4] == e["n_corr"] and st[2] == e["n_corr"] / len(c["src"]) == want[2] and abs(st[3] - want[3]) <= 1e-12
    T = st[5:21].reshape(4, 4)
    if e.get("T_is_init"):
        assert np.array_equal(T, c["init"])               # bit for bit: no update, or identity updates only
    elif e["updates"] == 1:
        np.testing.assert_allclose(T, want[5:21].reshape(4, 4), rtol=0, atol=1e-9 * max(1.0, float(np.abs(c["tgt"]).max())))
        np.testing.assert_allclose(st[21:37], want[21:37], rtol=0, atol=1e-9 * max(1.0, float(np.abs(c["tgt"]).max())))
    Rm = T[:3, :3]
    np.testing.assert_allclose(Rm @ Rm.T, np.eye(3), atol=1e-12)
    assert abs(np.linalg.det(Rm) - 1.0) < 1e-12 and T[3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_a_finished_chain_keeps_its_state_while_its_neighbour_goes_on():
    _lib, B, _ = _mods()
    a, b = EC.icp_case("p2p_2_corr"), EC.icp_case("max_iteration_1")
    pairs = [a, b]
    moved = B.transform(B.concat([_cloud(p["src"]) for p in pairs]), [p["init"] for p in pairs])
    tg = [_cloud(p["tgt"]) for p in pairs]
    grids = B.build_grids(tg, EC.ICP_MAX_DIST)
    ns = [len(m) for m in moved]
    corr = [torch.empty(x, dtype=torch.int32, device="cuda") for x in ns]
    d2 = [torch.empty(x, dtype=_D, device="cuda") for x in ns]
    sums = torch.zeros(2, 29, dtype=_D, device="cuda")
    st0 = np.zeros((2, 40))
    for k, p in enumerate(pairs):
        st0[k, 5:21] = p["init"].reshape(-1)
    state = _dev(st0)
    ws = torch.empty(2 * 512 * 29 * 8, dtype=torch.uint8, device="cuda")

    def run(n_iter, first):
        _lib.call.ape_icp_run_batch_f64(0, 2, *B._grid_args(grids), EC.ICP_MAX_DIST, B._ptrs([m._p for m in moved]), B._ints(ns), B._ptrs([t._p for t in tg]),
                                        None, EC.ICP_MAX_DIST, 0.0, 0.0, 30, n_iter, first, B._ptrs(corr), B._ptrs(d2),
                                        B._ptrs([sums[k] for k in range(2)]), B._ptrs([state[k] for k in range(2)]), _lib.dptr(ws), ws.numel(), B._st())
        return state.cpu().numpy().copy(), moved[0]._p.cpu().numpy().copy()

    s1, src1 = run(1, 1)
    assert s1[0, 0] == 1.0 and s1[0, 37] == 2.0 and s1[0, 1] == 0.0 and s1[1, 0] == 0.0 and s1[1, 1] == 2.0
    s2, src2 = run(3, 0)
    assert np.array_equal(s2[0], s1[0]) and np.array_equal(src2, src1)        # 40 words and the moved source, bit for bit
    assert s2[1, 1] == 5.0 and s2[1, 0] == 0.0 and np.array_equal(s2[0, 5:21].reshape(4, 4), a["init"])


# ---- rejections: what the host code returns before any launch ---------------------------------------------------------------------------------------
def test_rejections_before_any_launch():
    _lib, B, PC = _mods()
    L = _lib.lib()
    pts = EC.lattice(3, 3, 3)
    pc = _cloud(pts)
    n = len(pc)
    g = pc._grid(1.0)
    ga = B._grid_args([g])
    q, nq = B._ptrs([pc._p]), B._ints([n])
    cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    nrm = torch.zeros(n, 3, dtype=_D, device="cuda")
    mean = torch.zeros(n, dtype=_D, device="cuda")

    def query(op, nb, radius, m, cell=1.0):
        return L.ape_grid_query_batch_f64(op, nb, *ga, cell, q, nq, radius, m, B._ptrs([cnt]), B._ptrs([nrm]), B._ptrs([mean]), None)

    for m in (0, 65):
        assert query(1, 1, 1.0, m) == EINVAL and query(2, 1, 1.0, m) == EINVAL
    assert query(2, 1, 1.0, n + 1) == EINVAL             # k greater than the cloud size
    assert query(0, 1, 1.5, 0) == EINVAL and query(1, 1, 1.5, 30) == EINVAL      # radius > cell
    for nb in (0, 17):
        assert query(0, nb, 1.0, 0) == EINVAL and query(1, nb, 1.0, 30) == EINVAL and query(2, nb, 1.0, 3) == EINVAL
    out = torch.zeros(n, 3, dtype=_D, device="cuda")
    n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = B._ws(1, n, "cuda")

    def voxel(v, nb=1, ws_bytes=None):
        return L.ape_voxel_down_sample_batch_f64(nb, B._ptrs([pc._p]), B._ints([n]), v, B._ptrs([out]), _lib.dptr(n_out), _lib.dptr(ws),
                                                 ws.numel() if ws_bytes is None else ws_bytes, None)

    for v in (0.0, -1.0, float("nan")):
        assert voxel(v) == EINVAL
    assert voxel(1.0, nb=0) == EINVAL and voxel(1.0, nb=17) == EINVAL
    assert voxel(1.0, ws_bytes=ws.numel() - 1) == EWORKSPACE and voxel(1.0, ws_bytes=0) == EWORKSPACE
    sorted_, keys, order, origin = (torch.zeros(n, 3, dtype=_D, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda"),
                                    torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=_D, device="cuda"))
    assert L.ape_grid_build_batch_f64(1, B._ptrs([pc._p]), B._ints([n]), 1.0, B._ptrs([sorted_]), B._ptrs([keys]), B._ptrs([order]), B._ptrs([origin]),
                                      _lib.dptr(ws), ws.numel() - 1, None) == EWORKSPACE
    o9 = torch.zeros(9, dtype=_D, device="cuda")
    assert L.ape_moments_batch_f64(1, B._ptrs([pc._p]), B._ints([n]), _lib.dptr(o9), _lib.dptr(ws), 512 * 9 * 8 - 1, None) == EINVAL
    with pytest.raises(_lib.ApeError) as err:
        pc.estimate_normals(radius=1.0, max_nn=65)
    assert err.value.code == EINVAL
    with pytest.raises(ValueError, match="voxel_size"):   # 2^21 or more voxels along an axis: refused by the Python layer, nothing launched
        _cloud(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])).voxel_down_sample(2.0 ** -21)
    assert not cnt.any().item() and not nrm.any().item() and not mean.any().item() and not out.any().item()     # nothing ran

"""The round-1 ICP loop with the solve on the host -- test infrastructure, the parity reference of the device loop
(pointcloud.registration_icp -> batched.icp_states): the correspondence search and the 17 / 29 reduced sums run on the device through the
one-record entry points ape_grid_nn1_f64 / ape_icp_sums_f64, the sums come back once per iteration, and the 3x3 SVD (numpy / LAPACK) or the
6x6 solve, T <- update . T and open3d's convergence test run here.  It was `registration_icp(host_solve=True)` until the product function
lost its test-only branch."""
import math

import numpy as np
import torch

from autoposeestimation_amd import _lib
from autoposeestimation_amd.pc_reconstruction import pointcloud as PC

_D = torch.float64


def _umeyama(s):
    """Eigen::umeyama(src, dst, with_scaling=false) from the one-pass sums s[17]."""
    n = s[0]
    mu_s, mu_t = s[2:5] / n, s[5:8] / n
    cov = s[8:17].reshape(3, 3).T / n - np.outer(mu_t, mu_s)        # (1/n) sum (t - mu_t)(s - mu_s)^T
    U, d, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mu_t - R @ mu_s
    return T


def _vec6_to_mat4(x):
    """open3d TransformVector6dToMatrix4d: R = Rz(x[2]) Ry(x[1]) Rx(x[0]), t = x[3:6]"""
    cx, sx, cy, sy, cz, sz = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:6]
    return T


def _point_to_plane(s):
    JTJ = np.zeros((6, 6))
    k = 2
    for a in range(6):
        for b in range(a, 6):
            JTJ[a, b] = JTJ[b, a] = s[k]
            k += 1
    JTr = s[23:29]
    try:
        x = np.linalg.solve(JTJ, -JTr)
    except np.linalg.LinAlgError:
        return np.eye(4)
    return _vec6_to_mat4(x)


def registration_icp_host(source, target, max_correspondence_distance, init=None, estimation_method=None, criteria=None):
    """pointcloud.registration_icp's arguments and result, one device-to-host copy per iteration"""
    estimation_method = estimation_method or PC.TransformationEstimationPointToPoint()
    criteria = criteria or PC.ICPConvergenceCriteria()
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    ns, nt = len(source), len(target)
    if ns == 0 or nt == 0:
        return PC.RegistrationResult(T, 0.0, 0.0, 0)
    if estimation_method.kind == 1 and not target.has_normals():
        raise RuntimeError("TransformationEstimationPointToPlane requires target normals")
    dev = source.device
    pcd = source.clone().transform(T)
    grid = target._grid(max_correspondence_distance)
    corr = torch.empty(ns, dtype=torch.int32, device=dev)
    d2 = torch.empty(ns, dtype=_D, device=dev)
    sums = torch.empty(29, dtype=_D, device=dev)
    ws = torch.empty(512 * 29 * 8, dtype=torch.uint8, device=dev)

    def evaluate():
        _lib.call.ape_grid_nn1_f64(*PC.PointCloud._gargs(grid), _lib.dptr(pcd._p, _D), ns, float(max_correspondence_distance),
                                   _lib.dptr(corr), _lib.dptr(d2), _lib.stream_ptr())
        _lib.call.ape_icp_sums_f64(estimation_method.kind, _lib.dptr(pcd._p, _D), _lib.dptr(target._p, _D), _lib.dptr(target._n),
                                   _lib.dptr(corr), _lib.dptr(d2), ns, _lib.dptr(sums), _lib.dptr(ws), ws.numel(), _lib.stream_ptr())
        s = sums.cpu().numpy()
        n_corr = int(round(s[0]))
        fitness = n_corr / ns
        rmse = math.sqrt(s[1] / n_corr) if n_corr else 0.0
        return s, n_corr, fitness, rmse

    s, n_corr, fitness, rmse = evaluate()
    for _ in range(criteria.max_iteration):
        if n_corr < (3 if estimation_method.kind == 0 else 6):
            break
        update = _umeyama(s) if estimation_method.kind == 0 else _point_to_plane(s)
        T = update @ T
        pcd.transform(update)
        prev_f, prev_r = fitness, rmse
        s, n_corr, fitness, rmse = evaluate()
        if abs(prev_f - fitness) < criteria.relative_fitness and abs(prev_r - rmse) < criteria.relative_rmse:
            break
    return PC.RegistrationResult(T, fitness, rmse, n_corr)

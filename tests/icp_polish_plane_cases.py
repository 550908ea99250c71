"""Point-to-plane side of the depth ICP polish cases (csrc/icp_polish.hip kPointToPlane), shared by
test_icp_polish_plane_host.py and test_gpu_icp_polish_plane.py: the launch the tests run (the objects and classes of the point-to-point
tests, normals at 0.02 m so that the 63-point model has support) and the float64 reference built on
oracle/pointcloud_oracle.py:registration_icp(point_to_plane=True)."""
import math

import numpy as np

import icp_polish_cases as C
from oracle import pointcloud_oracle as PO

NORMAL_RADIUS = 0.02
NORMAL_MAX_NN = 30
# the launch of the parity tests: every case, mixed order, four objects on the 1000-point model
OBJECTS = (("big", 0), ("mid", 0), ("three", 0), ("odd", 0), ("noisy", 0), ("tiny", 0), ("mid", 1))
CLASS_OF_M = {1000: 0, 257: 1, 63: 2, 2600: 3}
SIZES = (1000, 500)                   # N: at 500, `big` has more candidates than rows


def clouds():
    return {k: C.model(m, 0)[0] for m, k in CLASS_OF_M.items()}


def cases():
    return [C.named(name, seed) for name, seed in OBJECTS]


def sources(p4, n_cand, N):
    """what the kernel reads of points4: the first min(n_cand, N) rows of every object, widened to float64"""
    return [p4[i, :min(int(n_cand[i]), N), :3].astype(np.float64) for i in range(len(p4))]


def icp_plane_with_reason(source, target, normals, max_dist, init, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """oracle/pointcloud_oracle.py:registration_icp(point_to_plane=True) with the two things it does not return: the correspondence count
    and why it stopped (1 converged, 2 fewer than 6 correspondences, 3 iteration limit; the limit is looked at before the count, as
    icp_step of csrc/pointcloud.hip does).  The point-to-plane twin of icp_polish_cases.icp_with_reason; like the oracle it raises
    numpy.linalg.LinAlgError on singular normal equations.  -> (T, fitness, rmse, correspondences, reason, updates)"""
    from scipy.spatial import cKDTree
    T = np.array(init, float)
    tree = cKDTree(target)
    src = source @ T[:3, :3].T + T[:3, 3]

    def evaluate(src):
        dd, j = tree.query(src, k=1)
        ok = dd ** 2 < max_dist ** 2
        n = int(ok.sum())
        return ok, j, n, n / len(src), (math.sqrt((dd[ok] ** 2).sum() / n) if n else 0.0)

    ok, j, n, fit, rmse = evaluate(src)
    updates = 0
    while True:
        if updates >= max_iteration:
            reason = 3
            break
        s, tt = src[ok], target[j[ok]]
        if len(s) < 6:
            reason = 2
            break
        nrm = normals[j[ok]]
        r = np.einsum("ij,ij->i", s - tt, nrm)
        J = np.concatenate([np.cross(s, nrm), nrm], 1)
        x = np.linalg.solve(J.T @ J, -(J.T @ r))
        U = PO.vec6_to_mat4(x)
        T = U @ T
        src = src @ U[:3, :3].T + U[:3, 3]
        updates += 1
        pf, pr = fit, rmse
        ok, j, n, fit, rmse = evaluate(src)
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            reason = 1
            break
    return T, fit, rmse, n, reason, updates


def reference(obs, m, normals, pose, max_dist=C.MAX_DIST, criteria=C.CRITERIA, min_fitness=0.0):
    """what ape_icp_polish_plane_batch_f64 must return for one object: (pose_out (7,), (fitness, rmse, correspondences, reason), T)"""
    pose = np.asarray(pose, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64).reshape(-1, 3)
    init = C.rigid_inverse(C.pose_matrix(pose))
    if len(obs) == 0:
        return pose.copy(), (0.0, 0.0, 0, 2), init
    T, fit, rmse, n, reason, updates = icp_plane_with_reason(obs, m, normals, max_dist, init, *criteria)
    if updates == 0 or fit < min_fitness:
        return pose.copy(), (fit, rmse, n, reason), T
    Ti = C.rigid_inverse(T)
    return C.pose7(Ti[:3, :3], Ti[:3, 3]), (fit, rmse, n, reason), T

"""The cases behind tests/golden/registration_one_pair.npz -- test infrastructure, no GPU at import.

The fixture holds what the one-pair global-registration API (pc_reconstruction.pointcloud / open3d_utils) returned on an MI355X at the last
commit that still had a one-pair implementation of its own beside the list one (ABI 21).  Since then the one-pair functions are one-element
calls into pc_reconstruction/batched.py, and test_gpu_registration.py::test_one_pair_api_equals_the_recorded_parent holds them to the
recorded bits: the kernels are float64 with fixed summation orders, so equality is exact.  tools/gen_golden_registration.py writes the file
from the same case list; only outputs are stored, the inputs are the seeded cases of registration_edge_cases.py and test_gpu_registration.py.

GROUPS[group]() -> [(case, fields, run)]; run() does the device work and returns {field: ndarray}; the key of a stored array is
"group/case/field".  An FPFH feature is stored as its shape and the SHA-256 of its float64 bytes -- equal digests are equal bits, and the
2 314 rows of the five clouds at their max_nn values would be 450 KB of incompressible doubles otherwise."""
import hashlib
import os

import numpy as np

import registration_edge_cases as EC

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "registration_one_pair.npz")
RANSAC_FIELDS = ("transformation", "fitness", "inlier_rmse", "correspondence_count", "validated", "iterations")
FPFH_CASES = ("lattice7_r6", "clusters_256_257", "n1", "triples", "zero_normals")
MATCH_CASES = ((1, 1), (129, 65), (128, 64))
# name, ransac_n, (edge, dist) of EC.CHECKERS, (max_iteration, max_validation), seed -- on EC.ransac_pair() at EC.MAX_DIST
RANSAC_RUNS = ([("n%d" % n, n, 3, (1000, 1000), 0) for n in (3, 4, 16)] +
               [("checkers%d" % k, 4, k, (1000, 1000), 0) for k in range(3)] +
               [("crit40000_50_n%d" % n, n, 3, (40000, 50), 0) for n in (4, 16)] +          # n16: nothing fills, the 16 k chunk then the 32 k one
               [("crit20000_17000_checkers%d" % k, 4, k, (20000, 17000), 0) for k in (0, 3)] +   # 0: every iteration passes, full inside the second chunk
               [("seed7", 4, 3, (1000, 1000), 7)])


def _mods():
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    return U, PC


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda").contiguous()


def _cloud(pts, normals=None):
    pc = _mods()[1].PointCloud(pts)
    if normals is not None:
        pc._n = _dev(normals)                                # injected, not estimated
    return pc


def _feature(a):
    return _mods()[1].Feature(_dev(a))


def _digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).digest(), np.uint8)


def _fpfh(name, max_nn):
    _, PC = _mods()
    c = EC.fpfh_cases()[name]
    f = PC.compute_fpfh_feature(_cloud(c["pts"], c["normals"]), PC.KDTreeSearchParamHybrid(radius=c["radius"], max_nn=max_nn)).t.cpu().numpy()
    return {"shape": np.array(f.shape, np.int64), "sha256": _digest(f)}


def fpfh_group():
    return [("%s_nn%d" % (n, m), ("shape", "sha256"), lambda n=n, m=m: _fpfh(n, m)) for n in FPFH_CASES for m in EC.fpfh_cases()[n]["max_nns"]]


def _nn(fs, ft):
    return {"nn": _mods()[1].feature_nn(_feature(fs), _feature(ft)).cpu().numpy()}


def feature_nn_group():
    out = [("%dx%d" % s, ("nn",), lambda s=s: _nn(*EC.matching_case(*s)[:2])) for s in MATCH_CASES]
    return out + [("nan", ("nn",), lambda: _nn(EC.nan_case()["fs"], EC.nan_case()["ft"]))]


def result_fields(r):
    return {"transformation": np.asarray(r.transformation, np.float64), "fitness": np.float64(r.fitness), "inlier_rmse": np.float64(r.inlier_rmse),
            "correspondence_count": np.int64(r.correspondence_count), "validated": np.asarray(r.validated), "iterations": np.int64(r.iterations)}


def _ransac(src, tgt, fs, ft, max_dist, ransac_n, checkers, crit, seed):
    _, PC = _mods()
    edge, dist = EC.CHECKERS[checkers]
    ch = ([PC.CorrespondenceCheckerBasedOnEdgeLength(edge)] if edge >= 0 else []) + ([PC.CorrespondenceCheckerBasedOnDistance(dist)] if dist >= 0 else [])
    return result_fields(PC.registration_ransac_based_on_feature_matching(src, tgt, fs, ft, max_dist, None, ransac_n, ch,
                                                                          PC.RANSACConvergenceCriteria(*crit), seed=seed))


def _tiny_features(p):
    """features that give tiny_pair's nn: distinct target rows, every source row an exact copy of its match's"""
    ft = np.random.default_rng(600).uniform(0.0, 200.0, (len(p["tgt"]), 33))
    return ft[p["nn"]], ft


def ransac_group():
    p = EC.ransac_pair()
    pair = lambda: (_cloud(p["src"]), _cloud(p["tgt"]), _feature(p["fs"]), _feature(p["ft"]))  # noqa: E731
    out = [(name, RANSAC_FIELDS, lambda a=(n, k, crit, seed): _ransac(*pair(), EC.MAX_DIST, *a)) for name, n, k, crit, seed in RANSAC_RUNS]
    out.append(("empty_source", RANSAC_FIELDS,
                lambda: _ransac(_mods()[1].PointCloud(), _cloud(p["tgt"]), _mods()[1].Feature(device="cuda"), _feature(p["ft"]), EC.MAX_DIST, 4, 3, (1000, 10), 0)))
    t = EC.tiny_pair(2)
    out.append(("tiny2", RANSAC_FIELDS, lambda: _ransac(_cloud(t["src"]), _cloud(t["tgt"]), *map(_feature, _tiny_features(t)), 2.0, 3, 0, (64, 64), 9)))
    return out


def _global():
    import test_gpu_registration as T
    U, PC = _mods()
    tgt, src, _ = T._pair()
    sd, _ = U.preprocess_point_cloud(PC.PointCloud(src), T.VOXEL)
    td, _ = U.preprocess_point_cloud(PC.PointCloud(tgt), T.VOXEL)
    return result_fields(U.execute_global_registration(sd, td, None, None, T.VOXEL))


def _icp_regression():
    import test_gpu_registration as T
    U, PC = _mods()
    tgt, src, _ = T._pair()
    return {"transformation": U.icp_regression(PC.PointCloud(tgt), PC.PointCloud(src), voxel_size=T.VOXEL, threshold=10, global_regression=True)[2]}


def drivers_group():
    return [("execute_global_registration", RANSAC_FIELDS, _global), ("icp_regression_global", ("transformation",), _icp_regression)]


GROUPS = {"fpfh": fpfh_group, "feature_nn": feature_nn_group, "ransac": ransac_group, "drivers": drivers_group}


def key(group, case, field):
    return "%s/%s/%s" % (group, case, field)


def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}

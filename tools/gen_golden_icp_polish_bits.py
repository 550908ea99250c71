"""Records tests/golden/icp_polish_p2p_bits.npz: what ape_icp_polish_batch_f64 (point-to-point, through engine.icp_polish) returns on the
GPU for the 7-object launch of tests/icp_polish_plane_cases.py at N = 1000 and N = 500 -- pose [7,7] and stats [7,4] float64 each.

    python tools/gen_golden_icp_polish_bits.py [--package-root DIR] [--label TEXT] [out.npz]        (MI355X; default: the fixture itself)

--package-root: a directory holding another checkout's `autoposeestimation_amd` with its built library, imported instead of this tree's
(the cases always come from this tree's tests/).  The script uses only ModelSet(clouds, device, max_dist) and the first eight arguments
of engine.icp_polish, so it runs unchanged on every commit that has the polish.  The committed fixture was recorded from the library of
the commit BEFORE the estimator became a compile-time parameter of the kernel's loop (ABI 22); the file names the toolchain and the
label given.  tests/test_gpu_icp_polish_plane.py::test_point_to_point_keeps_the_parents_bits compares the tree with it bit for bit.
Run it again only when a change is MEANT to alter the point-to-point results, and say so in the commit."""
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    root, label = REPO, ""
    if "--package-root" in argv:
        root = os.path.abspath(argv.pop(argv.index("--package-root") + 1))
        argv.remove("--package-root")
    if "--label" in argv:
        label = argv.pop(argv.index("--label") + 1)
        argv.remove("--label")
    out_path = argv[0] if argv else os.path.join(REPO, "tests", "golden", "icp_polish_p2p_bits.npz")
    sys.path[:0] = [root, REPO, os.path.join(REPO, "tests")]
    import torch
    import icp_polish_cases as C
    import icp_polish_plane_cases as P
    import autoposeestimation_amd
    from autoposeestimation_amd import _lib
    from autoposeestimation_amd import engine as E
    from autoposeestimation_amd.pipeline.polish import ModelSet
    assert os.path.abspath(autoposeestimation_amd.__file__).startswith(root + os.sep), autoposeestimation_amd.__file__

    class Criteria:
        relative_fitness, relative_rmse, max_iteration = C.CRITERIA
    try:
        hipcc = subprocess.run(["hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()[0]
    except (OSError, IndexError):
        hipcc = "hipcc not on PATH"
    toolchain = "%s; torch %s, HIP %s; %s; library ABI %d%s" % (hipcc, torch.__version__, torch.version.hip, torch.cuda.get_device_name(0),
                                                               _lib.lib().ape_abi_version(), "; " + label if label else "")
    out = {"toolchain": np.array(toolchain), "objects": np.array(["%s:%d" % o for o in P.OBJECTS])}
    models = ModelSet(P.clouds(), "cuda", C.MAX_DIST)
    cases = P.cases()
    cls = [P.CLASS_OF_M[len(c["model"])] for c in cases]
    pose_in = torch.from_numpy(np.stack([c["pose"] for c in cases])).cuda()
    for N in P.SIZES:
        p4 = torch.from_numpy(np.stack([C.points4(c["obs"], N) for c in cases])).cuda()
        n_cand = torch.from_numpy(np.array([len(c["obs"]) for c in cases], np.int32)).cuda()
        pose, stats = E.icp_polish(p4, n_cand, cls, models, pose_in, C.MAX_DIST, Criteria, 0.0)
        torch.cuda.synchronize()
        out["pose_%d" % N], out["stats_%d" % N] = pose.cpu().numpy(), stats.cpu().numpy()
        assert np.isfinite(out["pose_%d" % N]).all() and np.isfinite(out["stats_%d" % N]).all()
        print("N = %d: stop reasons %s, correspondences %s" % (N, out["stats_%d" % N][:, 3].tolist(), out["stats_%d" % N][:, 2].tolist()), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **out)
    print("wrote %s: %d bytes; %s" % (out_path, os.path.getsize(out_path), toolchain))


if __name__ == "__main__":
    main(sys.argv[1:])

"""Records tests/golden/registration_one_pair.npz: what the one-pair global-registration API returns on the GPU for the cases listed in
tests/registration_golden.py (FPFH, feature matching, RANSAC, execute_global_registration, icp_regression with global_regression).

    python tools/gen_golden_registration.py [out.npz]        (MI355X; default: the fixture itself)

It calls only the public one-pair Python API (pc_reconstruction.pointcloud / open3d_utils), so it runs unchanged on any commit that has that
API: the committed fixture was recorded at the last commit whose one-pair functions had an implementation of their own (ABI 21), and
tests/test_gpu_registration.py::test_one_pair_api_equals_the_recorded_parent compares the tree with it bit for bit.  Run it again only
when a change is MEANT to alter these results, and say so in the commit."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import registration_golden as G  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else G.FIXTURE
    from autoposeestimation_amd import _lib
    out = {"abi": np.int64(_lib.lib().ape_abi_version())}
    for group, cases in G.GROUPS.items():
        for case, fields, run in cases():
            got = run()
            assert set(got) == set(fields), (group, case)
            for f in fields:
                a = np.asarray(got[f])
                assert a.dtype.kind in "iu" or np.isfinite(a).all(), (group, case, f)
                out[G.key(group, case, f)] = a
            print(group, case, {f: (np.asarray(got[f]).tolist() if np.asarray(got[f]).size <= 3 else np.asarray(got[f]).shape) for f in fields}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **out)
    print("wrote %s: %d arrays, %d bytes" % (out_path, len(out), os.path.getsize(out_path)))


if __name__ == "__main__":
    main()

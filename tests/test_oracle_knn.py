"""Pins oracle/knn_oracle.c against (a) golden indices produced by the reference's own knn_cpu.cpp and
(b) the reference object oracle/_ref/libknn_ref.so on seeded cases: its indices are stored in tests/golden/knn_ref_object.npz
(tools/gen_golden.py), and where the object is present (build container only) it must still give them."""
import ctypes
import os

import numpy as np

from conftest import REPO, golden, run_oracle_knn


def test_oracle_knn_matches_reference_golden(oracle_knn_lib):
    g = golden("knn")
    for i in range(int(g["n_cases"])):
        ref, qry, want = g["ref_%d" % i], g["query_%d" % i], g["idx_%d" % i]
        got = run_oracle_knn(oracle_knn_lib, ref, qry, want.shape[1])
        assert np.array_equal(got, want), "case %d" % i


def test_oracle_knn_matches_reference_object(oracle_knn_lib):
    g = golden("knn_ref_object")
    path = os.path.join(REPO, "oracle", "_ref", "libknn_ref.so")
    lib = None
    if os.path.exists(path):
        import torch  # noqa: F401  (resolves the torch symbols the reference object links against)
        lib = ctypes.CDLL(path)
        lib.ref_knn.restype = ctypes.c_int
        lib.ref_knn.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_long] * 5
    rng = np.random.default_rng(123)
    for i, (b, d, nr, nq, k, qz) in enumerate([(1, 3, 300, 400, 1, 0), (1, 3, 128, 256, 1, 0.5), (2, 5, 40, 33, 3, 0.5)]):
        ref = rng.standard_normal((b, d, nr)).astype(np.float32)
        qry = rng.standard_normal((b, d, nq)).astype(np.float32)
        if qz:
            ref, qry = (np.round(ref / qz) * qz).astype(np.float32), (np.round(qry / qz) * qz).astype(np.float32)
        assert np.array_equal(ref, g["ref_%d" % i]) and np.array_equal(qry, g["query_%d" % i]), "case %d inputs" % i
        want = g["idx_%d" % i]
        if lib is not None:
            live = np.zeros((b, k, nq), np.int64)
            assert lib.ref_knn(ref.ctypes.data, qry.ctypes.data, live.ctypes.data, b, d, nr, nq, k) == 1
            assert np.array_equal(live, want), "case %d: the reference object no longer gives the stored indices" % i
        assert np.array_equal(run_oracle_knn(oracle_knn_lib, ref, qry, k), want), "case %d" % i

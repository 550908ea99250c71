"""CPU checks of the fast-global-registration restatement (tests/fgr_reference.py) and of the inputs the GPU tests use
(tests/fgr_cases.py): the restatement recovers a known motion, every case reaches the branch it names, and every case that the GPU test
compares at 1e-9 is stable under another summation order to 1e-10."""
import inspect

import numpy as np
import pytest

import fgr_cases as C
import fgr_reference as F


def test_restatement_recovers_a_known_rigid_transform():
    """12 x 12 x 3 lattice with a bump, about 25 degrees plus a translation, exact one-to-one features, decrease_mu with a floor of 1e-6:
    R and t to 1e-6 (SURVEY section 8c's bar for a recovered transform)"""
    c = C.recover_case()
    assert c["src"].shape == (432, 3)
    ang = np.degrees(np.arccos((np.trace(c["M"][:3, :3]) - 1) / 2))
    assert 24.0 < ang < 26.0 and np.linalg.norm(c["M"][:3, 3]) > 0.5
    r = F.fgr(c["src"], c["tgt"], c["fs"], c["ft"], c["opt"])
    assert r["mutual"] == 432 and r["tuples"] == 1000 and r["iterations"] == 64
    assert np.array_equal(r["matches"], np.stack([np.arange(432)] * 2, 1))
    assert np.abs(r["T"][:3, :3] - c["M"][:3, :3]).max() < 1e-6 and np.abs(r["T"][:3, 3] - c["M"][:3, 3]).max() < 1e-6
    assert np.array_equal(r["T"][3], [0, 0, 0, 1])


def test_public_surface_and_defaults():
    """the option class carries open3d 0.9's defaults plus the seed; the drivers' new keyword defaults to RANSAC"""
    from autoposeestimation_amd.pc_reconstruction import batched as B
    from autoposeestimation_amd.pc_reconstruction import open3d_utils as U
    from autoposeestimation_amd.pc_reconstruction import pointcloud as PC
    o = PC.FastGlobalRegistrationOption()
    assert {k: getattr(o, k) for k in F.DEFAULTS} == F.DEFAULTS
    assert list(inspect.signature(PC.registration_fast_based_on_feature_matching).parameters) == ["source", "target", "source_feature",
                                                                                                  "target_feature", "option"]
    assert list(inspect.signature(B.registration_fast).parameters) == ["sources", "targets", "source_features", "target_features", "options"]
    assert list(inspect.signature(U.execute_fast_global_registration).parameters) == ["source_down", "target_down", "source_fpfh", "target_fpfh",
                                                                                      "voxel_size"]
    for fn in (U.icp_regression, U.align_point_clouds, B.icp_regression_batch):
        p = inspect.signature(fn).parameters
        assert p["global_method"].default == "ransac" and p["global_regression"].default is False
        assert list(p)[-1] == "global_method"                     # appended: positional calls keep their meaning
    with pytest.raises(ValueError):
        U._global_registration("teaser")
    with pytest.raises(ValueError):
        B._global_registration_batch("teaser")


@pytest.mark.parametrize("name", list(C.matching_cases()))
def test_matching_cases_reach_their_branch(name):
    c, want = C.matching_cases()[name]
    nn_st, nn_ts = F.feature_nn(c["fs"], c["ft"]), F.feature_nn(c["ft"], c["fs"])
    e = C.expected(name)
    assert np.array_equal(e["matches"], want) and e["mutual"] == len(want)
    assert e["tuples"] == 0 and np.array_equal(e["T"], np.eye(4))            # at most two matches: no trial without a repeated draw
    if name == "ncorr0":
        assert (nn_st == -1).all() and (nn_ts == -1).all()                   # a NaN in every source row: no finite distance either way
    if name == "ncorr1":
        assert C.repeated_draws(0, np.arange(100), 1).all()
    if name == "one_way":
        assert nn_st[2] == 1 and nn_ts[1] == 1
    if name == "ties":
        assert nn_st.tolist() == [0, 0, 2] and nn_ts.tolist() == [0, 0, 2]


@pytest.mark.parametrize("name", list(C.optimisation_cases()))
def test_optimisation_cases_reach_their_branch_and_are_stable(name):
    C.check_guards(name)
    e, r = C.expected(name), C.expected_reversed(name)
    assert np.array_equal(e["kept"], r["kept"]) and e["iterations"] == r["iterations"]
    assert np.abs(e["T"] - r["T"]).max() <= C.REVERSE_ATOL


def test_tuple_cases_reach_their_branch():
    # strict boundary: lengths 1 and 2 at tuple_scale 0.5 fail, and only the boundary makes them fail
    t = C.triangle_case(0.5)
    e = F.fgr(t["src"], t["tgt"], t["fs"], t["ft"], t["opt"])
    assert e["mutual"] == 3 and e["tuples"] == 0
    assert not C.repeated_draws(0, np.arange(300), 3).all()
    t = C.triangle_case(0.49)
    e49 = F.fgr(t["src"], t["tgt"], t["fs"], t["ft"], t["opt"])
    assert e49["tuples"] > 0 and not C.repeated_draws(0, e49["kept"], 3).any()
    assert np.array_equal(e49["kept"], np.flatnonzero(~C.repeated_draws(0, np.arange(300), 3)))
    # repeated draws, and a list that never fills: trials beyond 100 * ncorr would pass but are never drawn
    s = C.small_pair()
    e = C.expected("small_never_full")
    rep = C.repeated_draws(0, np.arange(500), 5)
    assert rep.any() and not rep[e["kept"]].any() and e["kept"].max() < 500
    assert F.tuple_pass(s["src"], s["tgt"], e["matches"], 0, np.arange(500, 1024), 0.95).any()
    # a list of TUPLE_FILL on the base pair fills in the second block of the first 1024 trials, and not at a multiple of the block size
    p = C.base_pair()
    m = F.mutual_matches(F.feature_nn(p["fs"], p["ft"]), F.feature_nn(p["ft"], p["fs"]))
    k = F.kept_trials(p["src"], p["tgt"], m, 0, 0.95, C.TUPLE_FILL)
    assert len(k) == C.TUPLE_FILL and C.BLOCK < k[-1] + 1 < 1024 and (k[-1] + 1) % C.BLOCK != 0
    assert F.tuple_pass(p["src"], p["tgt"], m, 0, np.arange(k[-1] + 1, 2048), 0.95).any()


def test_shared_option_list_spans_two_launches_with_different_pairs():
    """the lock-step test's pairs: one option set, more than 16 of them live, and no two alike in what a launch shares between its pairs"""
    cases, exp = C.shared_option_list(), C.shared_expected()
    live = [i for i, c in enumerate(cases) if c is not None]
    assert len(live) > 16 and 0 < len(live) % 16 and len(cases) - len(live) == 3 and cases[2] is None
    keys = {tuple(sorted((k, v) for k, v in cases[i]["opt"].items() if k != "seed")) for i in live}
    assert len(keys) == 1 and len({cases[i]["opt"]["seed"] for i in live}) == len(live)
    assert len({len(cases[i]["src"]) for i in live}) >= 15 and any(len(cases[i]["src"]) != len(cases[i]["tgt"]) for i in live)
    tuples = [exp[i]["tuples"] for i in live]
    first, second = tuples[:16], tuples[16:]
    assert len(set(first)) >= 8 and first.count(1000) >= 2 and min(first) == 0 and len(second) >= 2 and len(set(second)) >= 2
    assert any(0 < 3 * t for t in tuples) and any(3 * t < 10 for t in tuples)                  # identity pairs beside optimised ones
    assert all(e["iterations"] == 64 for e in (exp[i] for i in live) if 3 * e["tuples"] >= 10)
    # where a pair stops adding to its list: the chunk in which it fills, or the one that holds its last trial
    stop = [C.chunk_index(int(exp[i]["kept"][-1]) + 1 if exp[i]["tuples"] == 1000 else max(100 * exp[i]["mutual"], 1)) for i in live]
    assert len(set(stop[:16])) >= 5 and max(stop) >= 5
    full = [s for s, t in zip(stop, tuples) if t == 1000]
    assert len(set(full)) >= 2                                                                # full lists that fill in different chunks
    for i in live:                                                                             # stable under another summation order
        c = cases[i]
        r = F.fgr(c["src"], c["tgt"], c["fs"], c["ft"], c["opt"], reverse=True)
        assert np.abs(r["T"] - exp[i]["T"]).max() <= C.REVERSE_ATOL

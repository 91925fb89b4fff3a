"""NDT pose search on the device (lsr_ndt_score_poses, lsr_ndt_search_pose, Localizer.relocalize; csrc/pose_search.hip).

The score of a pose is defined as what a derivative pass at that pose returns, so the scoring kernel is compared with
derivatives(T = pose) by np.array_equal — every neighbourhood, every table mode, sources around the 64-point chunk, pose lists around
the 16-candidate tile of a workgroup and its 8-candidate staging batch.  The whole search is compared member by member with single
aligns (array_equal again), with the restated selection on the device's own scores, with the CPU oracle started from the winner's
candidate, and with the truth — on the six inputs on which tests/test_pose_search_cpu.py shows that the procedure itself succeeds."""
import ctypes as C
import math

import numpy as np
import pytest

import pose_search_numpy as psn
from lidarslam_ros2_amd import (DIRECT1, DIRECT7, DIRECT26, KDTREE, GeneralizedIterativeClosestPoint, Localizer, LocalizerParams,
                                NormalDistributionsTransform, _capi, poseLattice, synth)
from lidarslam_ros2_amd._capi import RegistrationError
from lidarslam_ros2_amd.frontend import as_pc2_payload
from lidarslam_ros2_amd.posemath import pose_delta
from ndt_variants import POSE_R_TOL, POSE_T_TOL, SCORE_TOL

pytestmark = pytest.mark.gpu

TILE, BATCH = 16, 8       # csrc/pose_search.hpp: PS_TILE candidates per workgroup, PS_BATCH per trip through a wave's staging tile
P0 = np.zeros(6)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def make_ndt(neighborhood=DIRECT7, table_mode=None, target=None, source=None):
    ndt = NormalDistributionsTransform(device=0)
    ndt.setResolution(psn.RES)
    ndt.setTransformationEpsilon(psn.EPS)
    ndt.setNeighborhoodSearchMethod(neighborhood)
    if table_mode is not None:
        ndt.setTuning(table_mode=table_mode)
    if target is not None:
        ndt.setInputTarget(synth.as_pointxyzi(target))
    if source is not None:
        ndt.setInputSource(synth.as_pointxyzi(source))
    return ndt


def by_derivatives(ndt, poses):
    out = [ndt.derivatives(P0, T=T, compute_hessian=False, with_pairs=True) for T in poses]
    return np.array([o[0] for o in out]), np.array([o[3] for o in out])


def assert_same_bits(got, want, label=""):
    for g, w, what in zip(got, want, ("score", "pairs")):
        assert np.array_equal(np.asarray(g).view(np.uint64), np.asarray(w).view(np.uint64)), (label, what, np.flatnonzero(g != w)[:8])


def truth32(case):
    return np.asarray(case.truth, np.float32)


# ---- 1. bits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table_mode", [0, 1, 2], ids=["dense", "compact", "lds"])
@pytest.mark.parametrize("neighborhood", [DIRECT7, DIRECT1, DIRECT26], ids=["direct7", "direct1", "direct26"])
def test_scores_are_the_bits_of_a_derivative_pass(neighborhood, table_mode):
    case = psn.case(0)
    ndt = make_ndt(neighborhood, table_mode, case.target)
    info = ndt.gridInfo()
    T = truth32(case)
    far = T.copy()
    far[0, 3] += 500.0
    edge = T.copy()                                        # the sensor on the upper x face of the grid's bounding box
    edge[0, 3] = (int(info["max_b"][0]) + 1) * psn.RES
    poses = np.concatenate([poseLattice(T, (5, 5, 1), (0.5, 0.5, 1.0), 5, math.radians(3.0)), far[None], edge[None],
                            np.eye(4, dtype=np.float32)[None]])
    assert poses.shape[0] == 128
    for n in (1, 63, 64, 65, 129, 2000):
        ndt.setInputSource(synth.as_pointxyzi(case.source[:n]))
        got = ndt.scorePoses(poses)
        want = by_derivatives(ndt, poses)
        assert_same_bits(got, want, (n,))
        assert got[0][125] == 0.0 and got[1][125] == 0.0                    # 500 m away: no point meets a voxel
        if n == 2000:
            centre = 62                                                      # the truth itself: the middle of the lattice
            assert got[1][centre] > 1000                                     # most points of the scan meet a usable leaf there
            assert got[1][126] < got[1][centre]                              # on the face: part of the scan has no voxel
            print(f"pairs at the truth {got[1][centre]:.0f}, on the face {got[1][126]:.0f}, at the identity {got[1][127]:.0f}")


# ---- 2. the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, d", psn.INPUTS)
def test_lattice_scores_against_the_oracle(O, seed, d):
    """The 1053 poses of the search lattice: score within the project's 1e-5 of the oracle's — relative to the candidate's own score
    where that is at least 1 % of the lattice maximum, below that absolute (1e-5 of the maximum); pair counts equal to the count of
    (point, usable leaf) pairs on the oracle's grid."""
    case = psn.case(seed)
    ndt = make_ndt(DIRECT7, None, case.target, case.source)
    poses = poseLattice(psn.displaced_center(case.truth, d), **psn.LATTICE)
    assert poses.shape[0] == 1053
    score, pairs = ndt.scorePoses(poses)
    grid = O.VoxelGridCovariance(case.target, psn.RES)
    ref = np.array([O.ndt_derivatives(grid, case.source, P0, T=T, compute_hessian=False, resolution=psn.RES)[0] for T in poses])
    top = ref.max()
    bar = np.where(ref >= 0.01 * top, SCORE_TOL * ref, SCORE_TOL * top)
    err = np.abs(score - ref)
    print(f"seed {seed} displacement {d}: largest score error {np.max(err / bar):.3f} of the bar; maximum {top:.1f}")
    assert top > 0 and np.all(err <= bar), (np.argmax(err / bar), np.max(err / bar))
    assert np.array_equal(pairs, psn.pair_counts(grid, case.source, poses))


# ---- 3. counts -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored_lattice():
    case = psn.case(0)
    ndt = make_ndt(DIRECT7, None, case.target, case.source)
    poses = poseLattice(psn.displaced_center(case.truth, 0), **psn.LATTICE)
    return ndt, poses, ndt.scorePoses(poses)


def test_list_lengths_around_the_tile(scored_lattice):
    ndt, poses, full = scored_lattice
    rng = np.random.default_rng(3)
    spots = rng.choice(poses.shape[0], 64, replace=False)
    assert_same_bits((full[0][spots], full[1][spots]), by_derivatives(ndt, poses[spots]), "1053")
    for k in (1, 2, BATCH - 1, BATCH, BATCH + 1, TILE - 1, TILE, TILE + 1, 63, 64, 65, 1053):
        got = ndt.scorePoses(poses[:k])
        assert got[0].shape == (k,)
        assert_same_bits(got, (full[0][:k], full[1][:k]), k)
    for start in (5, 1040):               # a list that does not start on a tile of the long one
        got = ndt.scorePoses(poses[start:start + TILE + 1])
        assert_same_bits(got, (full[0][start:start + TILE + 1], full[1][start:start + TILE + 1]), start)


def test_repeated_and_permuted_lists(scored_lattice):
    ndt, poses, full = scored_lattice
    rng = np.random.default_rng(4)
    some = poses[:100].copy()
    some[3] = some[40] = some[97] = poses[500]
    got = ndt.scorePoses(some)
    for k in (3, 40, 97):
        assert got[0][k] == full[0][500] and got[1][k] == full[1][500] and full[1][500] > 0
    perm = rng.permutation(poses.shape[0])
    got = ndt.scorePoses(poses[perm])
    assert_same_bits(got, (full[0][perm], full[1][perm]), "permuted")


@pytest.mark.parametrize("count", [70000, 70000 + TILE - 1, 70000 + TILE + 1])
def test_seventy_thousand_poses(count):
    """More candidates than a grid's y or z dimension holds (65 535): a 64-point source, the whole list against the same list scored in
    slices of 1000, and 64 spot checks against derivatives."""
    case = psn.case(0)
    ndt = make_ndt(DIRECT7, None, case.target, case.source[:64])
    poses = poseLattice(truth32(case), (51, 50, 1), (0.2, 0.2, 1.0), 28, math.radians(2.0))[:count]
    assert poses.shape[0] == count
    got = ndt.scorePoses(poses)
    if count == 70000:
        parts = [ndt.scorePoses(poses[a:a + 1000]) for a in range(0, count, 1000)]
        assert_same_bits(got, (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), "slices")
    spots = np.concatenate([np.random.default_rng(count).choice(count, 60, replace=False), [0, 65535, 65536, count - 1]])
    assert_same_bits((got[0][spots], got[1][spots]), by_derivatives(ndt, poses[spots]), "spots")
    assert np.count_nonzero(got[1]) > count // 2


# ---- 4. no side effects --------------------------------------------------------------------------------------------------------------
def test_scoring_leaves_the_object_as_it_was(scored_lattice):
    ndt, poses, _ = scored_lattice
    case = psn.case(0)
    ndt.align(case.guess)
    before, r_before = ndt.getFinalTransformation(), dict(ndt.last_result)
    fit = ndt.getFitnessScore()
    ndt.scorePoses(poses[:200])
    assert np.array_equal(ndt.getFinalTransformation(), before) and ndt.hasConverged() == r_before["converged"]
    assert ndt.getFitnessScore() == fit
    ndt.align(case.guess)
    r_after = dict(ndt.last_result)
    assert np.array_equal(ndt.getFinalTransformation(), before)
    for key in ("converged", "iterations", "score", "n_evaluations", "n_correspondences"):
        assert r_before[key] == r_after[key]


# ---- 5. the search -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, d", psn.INPUTS)
def test_search_pose(O, seed, d):
    case = psn.case(seed)
    ndt = make_ndt(DIRECT7, None, case.target, case.source)
    center = psn.displaced_center(case.truth, d)
    pose, result, rep = ndt.searchPose(center, top_k=psn.TOP_K, min_sep_m=psn.SEP_M, min_sep_rad=psn.SEP_RAD, **psn.LATTICE)
    assert rep["n_candidates"] == 1053 and rep["n_kept"] == psn.TOP_K
    # the object answers as after align
    assert np.array_equal(ndt.getFinalTransformation(), pose) and ndt.hasConverged() == result["converged"]
    # the selection: the restatement on the device's own scores
    poses = poseLattice(center, **psn.LATTICE)
    score, _ = ndt.scorePoses(poses)
    kept = psn.select(score, poses, psn.TOP_K, psn.SEP_M, psn.SEP_RAD)
    assert np.array_equal(rep["kept"], kept) and np.array_equal(rep["coarse_score"], score[kept])
    # every member: the bits of a single align from its candidate
    single = make_ndt(DIRECT7, None, case.target, case.source)
    for e, c in enumerate(kept):
        single.align(poses[c])
        assert np.array_equal(single.getFinalTransformation(), rep["refined"][e]), (e, c)
        for key in ("converged", "iterations", "score", "n_evaluations"):
            assert single.last_result[key] == rep["results"][e][key], (e, key)
    # the winner: the largest trans_probability, ties to the lower rank
    tp = [r["score"] for r in rep["results"]]
    w = rep["winner"]
    assert w == int(np.argmax(tp)) and np.array_equal(pose, rep["refined"][w]) and result["score"] == tp[w]
    # ... against the oracle from the same candidate (north-star bars), and against the truth
    grid = O.VoxelGridCovariance(case.target, psn.RES)
    ref = O.ndt_align(grid, case.source, poses[kept[w]], resolution=psn.RES, trans_eps=psn.EPS)
    dt, dr = pose_delta(pose, ref["final"])
    tt, tr = pose_delta(pose, case.truth)
    print(f"seed {seed} displacement {d}: winner rank {w} (tp {tp[w]:.6f}); {dt:.2e} m {dr:.2e} rad from the oracle, {tt:.4f} m {tr:.2e} rad from the truth")
    assert dt < POSE_T_TOL and dr < POSE_R_TOL
    assert tt < 0.05 and tr < 0.005


def test_search_with_nothing_kept():
    """A lattice 500 m off the map: no point meets a voxel, every score is 0 — LSR_OK, nothing kept, the object's last result stays."""
    case = psn.case(0)
    ndt = make_ndt(DIRECT7, None, case.target, case.source)
    ndt.align(case.guess)
    before = ndt.getFinalTransformation()
    far = truth32(case)
    far[1, 3] += 500.0
    pose, result, rep = ndt.searchPose(far, (3, 3, 1), (1.0, 1.0, 1.0), 3, 0.1, top_k=4)
    assert pose is None and rep["n_kept"] == 0 and rep["winner"] == -1 and rep["n_candidates"] == 27 and not result["converged"]
    assert np.array_equal(ndt.getFinalTransformation(), before)


# ---- 6. Localizer.relocalize ---------------------------------------------------------------------------------------------------------
def test_relocalize_then_track():
    case = psn.case(0)
    ndt = make_ndt(DIRECT7)
    loc = Localizer(ndt, LocalizerParams(scan_min_range=0.1, scan_max_range=100.0, vg_size_for_input=0.2, reach=(60.0, 60.0, 20.0),
                                         slack=(6.0, 6.0, 6.0)))
    loc.set_map(synth.as_pointxyzi(case.target))
    center = psn.displaced_center(case.truth, 0)
    loc.set_initial_pose(center)
    loc.lost = True
    payload = as_pc2_payload(case.source)
    pose = loc.relocalize(payload, case.source.shape[0], half_extent=(4.0, 4.0, 0.0), yaw_half_range=math.radians(30.0))
    assert loc.last_search["n_candidates"] == 1053 and loc.last_search["n_kept"] == 16
    tt, tr = pose_delta(pose, case.truth)
    assert tt < 0.05 and tr < 0.005 and not loc.lost and np.array_equal(loc.pose, pose)
    # the window: cut around the found pose (it left the search centre by more than slack / 2 = 3 m on no axis? then around the centre)
    moved = np.abs(pose[:3, 3].astype(np.float64) - center[:3, 3]) > 3.0
    want_center = pose[:3, 3] if moved.any() else center[:3, 3]
    assert np.allclose(loc.center, want_center) and loc.window.contains(pose[:3, 3]) and loc.n_target > 0
    assert loc.n_recuts == (1 if moved.any() else 0)
    # and the tracker goes on from there
    again = loc.receive_cloud(payload, case.source.shape[0])
    ta, ra = pose_delta(again, case.truth)
    assert ta < 0.05 and ra < 0.005 and not loc.lost
    # nothing kept: raises, the state stays
    far = center.copy()
    far[1, 3] += 500.0
    state = (loc.pose.copy(), loc.window, loc.center.copy(), loc.lost)
    with pytest.raises((RuntimeError, RegistrationError)):
        loc.relocalize(payload, case.source.shape[0], center=far, half_extent=(1.0, 1.0, 0.0), yaw_half_range=math.radians(10.0))
    assert np.array_equal(loc.pose, state[0]) and loc.window == state[1] and np.array_equal(loc.center, state[2]) and loc.lost == state[3]


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def _raw_score(reg, poses16, count, score, pairs=None):
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    return _capi.load().lsr_ndt_score_poses(reg._h, None if poses16 is None else poses16.ctypes.data_as(fp), count,
                                            None if score is None else score.ctypes.data_as(dp),
                                            None if pairs is None else pairs.ctypes.data_as(dp))


def _raw_derivatives(reg, T16):
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    s = C.c_double()
    return _capi.load().lsr_ndt_derivatives_pairs(reg._h, P0.ctypes.data_as(dp), T16.ctypes.data_as(fp), 0, C.byref(s), None, None, None)


def test_errors():
    case = psn.case(0)
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (4, 1))
    score, pairs = np.full(4, 7.0), np.full(4, 7.0)
    untouched = lambda: np.all(score == 7.0) and np.all(pairs == 7.0)
    # no target, no source: as lsr_ndt_derivatives
    ndt = make_ndt(DIRECT7)
    assert _raw_score(ndt, eye, 4, score, pairs) == _raw_derivatives(ndt, eye[0]) == -4 and untouched()
    ndt.setInputTarget(synth.as_pointxyzi(case.target))
    assert _raw_score(ndt, eye, 4, score, pairs) == _raw_derivatives(ndt, eye[0]) == -5 and untouched()
    with pytest.raises(RegistrationError):
        ndt.searchPose(np.eye(4), (1, 1, 1), (1, 1, 1), 1, 0.0)
    ndt.setInputSource(synth.as_pointxyzi(case.source[:100]))
    # arguments
    assert _raw_score(ndt, None, 4, score, pairs) == -1 and _raw_score(ndt, eye, 4, None, pairs) == -1
    assert _raw_score(ndt, eye, 0, score, pairs) == -1 and _raw_score(ndt, eye, (1 << 20) + 1, score, pairs) == -1
    for bad in (np.nan, np.inf, -np.inf):
        p = eye.copy()
        p[2, 13] = bad
        assert _raw_score(ndt, p, 4, score, pairs) == -1 and untouched()
    assert _raw_score(ndt, eye, 4, score, None) == 0 and np.all(pairs == 7.0) and not np.any(score == 7.0)      # pairs is optional
    for k in (0, 17):
        with pytest.raises(RegistrationError) as e:
            ndt.searchPose(np.eye(4), (1, 1, 1), (1, 1, 1), 1, 0.0, top_k=k)
        assert e.value.status == -1
    with pytest.raises(RegistrationError) as e:
        ndt.searchPose(np.eye(4), (0, 1, 1), (1, 1, 1), 1, 0.0)
    assert e.value.status == -1
    # KDTREE stays out
    ndt.setNeighborhoodSearchMethod(KDTREE)
    score[:] = 7.0
    assert _raw_score(ndt, eye, 4, score, pairs) == _capi.ERR_NOT_IMPLEMENTED and untouched()
    with pytest.raises(RegistrationError) as e:
        ndt.searchPose(np.eye(4), (1, 1, 1), (1, 1, 1), 1, 0.0)
    assert e.value.status == _capi.ERR_NOT_IMPLEMENTED
    # a GICP object: scoring answers what lsr_ndt_derivatives answers on it; the search is refused
    gicp = GeneralizedIterativeClosestPoint(device=0)
    assert _raw_score(gicp, eye, 4, score, pairs) == _raw_derivatives(gicp, eye[0]) != 0 and untouched()
    best, res = np.zeros(16, np.float32), _capi.Result()
    prm = _capi.PoseSearchParams(_capi.PoseLattice((C.c_int32 * 3)(1, 1, 1), (C.c_double * 3)(1, 1, 1), 1, 0.0), 4, 1.0, 0.1)
    assert _capi.load().lsr_ndt_search_pose(gicp._h, eye.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm),
                                            best.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res), None) == -1


def test_search_lets_go_of_the_target():
    """The workers share the object's target only for the length of the call: afterwards the object alone holds it again — a new
    resolution rebuilds its grid in place (refused for a shared target), and the search can be repeated with the same answer."""
    case = psn.case(0)
    ndt = make_ndt(DIRECT7, None, case.target, case.source)
    center = psn.displaced_center(case.truth, 0)
    first, _, rep1 = ndt.searchPose(center, (5, 5, 1), (1.0, 1.0, 1.0), 5, math.radians(5.0), top_k=4)
    again, _, rep2 = ndt.searchPose(center, (5, 5, 1), (1.0, 1.0, 1.0), 5, math.radians(5.0), top_k=4)
    assert rep1["n_kept"] == 4 and np.array_equal(first, again) and np.array_equal(rep1["kept"], rep2["kept"])
    ndt.setResolution(3.0)
    ndt.align(case.guess)
    assert ndt.hasConverged() and ndt.gridInfo()["n_valid"] > 0

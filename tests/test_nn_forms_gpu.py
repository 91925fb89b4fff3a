"""GPU: every form of the nearest-neighbour search against brute force (tests/nn_numpy.py), reached BY SHAPE —
  a. nn1_wave_kernel on adversarial clouds, over the refined, the sort-built and the bucket-built grid of an NDT object;
  b. more than 262 144 queries: nn1_kernel capped at two fine shells + nn1_coop_kernel over the work list, and getFitnessScore on top;
  c. fitness_score_batch: nn1_ball_group_kernel + nn1_list_group_kernel, members that fill the work list included;
  d. a target hundreds of metres wide (the sort builder chosen by the key count) and LSR_ERR_INDEX_OVERFLOW for one too wide.
(index, d2) comparisons are np.array_equal: same fp32 arithmetic, exact search.  tests/test_nn_numpy_cpu.py asserts on the CPU that
the inputs have the properties that take these paths."""
import functools

import numpy as np
import pytest

import nn_numpy as N

pytestmark = pytest.mark.gpu

F = np.float32
RANGES = (N.DBL_MAX, 1.0, 0.25)
PARKED = np.float32([[5000, 5000, 5000], [5001, 5000, 5000], [5000, 5001, 5000], [5000, 5000, 5001]])


def make_ndt(res=4.0, builder=0):
    from lidarslam_ros2_amd import NormalDistributionsTransform

    r = NormalDistributionsTransform(device=0)
    r.setResolution(res)
    r.setTransformationEpsilon(0.01)
    if builder:
        r.setTuning(grid_builder=builder)
    return r


def park_pose(r, T):
    """Put the pose T into the object.  setMaximumIterations(0) alone does not: NDT's `iterations > max` test is strict, two Newton
    steps are still taken.  A source kilometres away touches no voxel, the Newton step is zero and align() leaves the guess as the
    final transformation; setInputSource afterwards does not touch it."""
    r.setMaximumIterations(0)
    r.setInputSource(PARKED)
    r.align(T)
    assert np.array_equal(r.getFinalTransformation(), np.asarray(T, F))


def same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "d2", int((got[1] != want[1]).sum()))
    assert np.array_equal(got[0], want[0]), (what, "index", int((got[0] != want[0]).sum()))


# ---- a. the wave form on adversarial clouds ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["refined", "sort_built", "nan_in_target"])
@pytest.mark.parametrize("name", [n for n, _ in N.clouds()])
def test_wave_form_on_adversarial_clouds(name, variant):
    pts = N.cloud(name)
    tgt = np.vstack([pts, np.full((1, 3), np.nan, F)]) if variant == "nan_in_target" else pts
    for res in (4.0, 3.7, 2.96):
        q = N.query_mix(pts, res / 8)
        r = make_ndt(res, 1 if variant == "sort_built" else 0)
        r.setInputTarget(tgt)
        r.setInputSource(q)
        for T in (None, N.yaw_pose()):
            same(r.nearestNeighbors(T), N.brute_nn(pts, q, T), (name, variant, res, T is None))   # indices of the ORIGINAL cloud


# ---- b. more than 262 144 queries ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_large_query_set_neighbours(builder):
    n = N.NN_WAVE_MAX_QUERIES + 1
    r = make_ndt(4.0, builder)
    r.setInputTarget(N.large_target())
    for posed in (False, True):
        r.setInputSource(N.large_source(n, posed))
        same(r.nearestNeighbors(N.yaw_pose() if posed else None), N.large_brute(n, posed), (builder, posed))


@pytest.mark.parametrize("builder", [0, 1])
def test_large_query_set_ragged_last_workgroup(builder):
    n = N.NN_WAVE_MAX_QUERIES + 4096 + 3
    r = make_ndt(4.0, builder)
    r.setInputTarget(N.large_target())
    r.setInputSource(N.large_source(n))
    same(r.nearestNeighbors(None), N.large_brute(n), builder)


@pytest.mark.parametrize("builder", [0, 1])
def test_large_query_set_fitness(builder):
    """getFitnessScore over the capped walk + work list, its gate included; 102 queries sit exactly ON max_range = 0.25 (T = identity)."""
    n = N.NN_WAVE_MAX_QUERIES + 1
    tgt = N.large_target()
    r = make_ndt(4.0, builder)
    r.setInputTarget(tgt)
    for posed in (False, True):
        T = N.yaw_pose() if posed else np.eye(4, dtype=F)
        park_pose(r, T)
        src = N.large_source(n, posed)
        r.setInputSource(src)
        assert np.array_equal(r.getFinalTransformation(), T)
        for max_range in RANGES:
            got, want = r.getFitnessScore(max_range), N.brute_fitness(tgt, src, T, max_range, N.large_brute(n, posed))
            print("large fitness", builder, posed, max_range, got, want)
            assert got == pytest.approx(want, rel=N.fitness_rel_tol(n), abs=0), (builder, posed, max_range)


def test_large_query_set_all_deferred():
    """Every finite query 1 000 m outside the grid: the work list is written to its last slots, every answer comes from coop_knn."""
    n = N.NN_WAVE_MAX_QUERIES + 1
    r = make_ndt(4.0)
    r.setInputTarget(N.large_target())
    r.setInputSource(N.large_source(n) + np.float32([1000.0, 0, 0]))
    same(r.nearestNeighbors(None), N.large_brute(n, False, 1000.0), "shifted")


# ---- c. the group fitness form -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_brute():
    tgt = N.group_target()
    return tuple(N.brute_nn(tgt, src, T) for _, T, src in N.group_members())


@pytest.mark.parametrize("which", [tuple(range(13)), (2, 5, 7)], ids=["B13", "B3"])
def test_group_fitness_against_brute_force(which):
    """B = 13: a group of twelve (256 workgroups walk the lists) and a group of one (1 024); B = 3: half_out, ball and the empty source."""
    from lidarslam_ros2_amd.registration import fitness_score_batch, set_input_source_batch, set_input_target_batch

    tgt = N.group_target()
    members = [N.group_members()[k] for k in which]
    refs = [group_brute()[k] for k in which]
    regs = [make_ndt(4.0) for _ in members]
    set_input_target_batch(regs, [tgt] * len(regs))
    for r, (_, T, _) in zip(regs, members):
        park_pose(r, T)
    set_input_source_batch(regs, [src for _, _, src in members])
    for r, (_, T, _) in zip(regs, members):
        assert np.array_equal(r.getFinalTransformation(), T)
    for max_range in RANGES:
        fits = fitness_score_batch(regs, max_range)
        for b, (name, T, src) in enumerate(members):
            want = N.brute_fitness(tgt, src, T, max_range, refs[b])
            single = regs[b].getFitnessScore(max_range)
            print("group fitness", len(regs), name, max_range, fits[b], single, want)
            assert fits[b] == pytest.approx(want, rel=N.fitness_rel_tol(len(src)), abs=0), (name, max_range)
            assert fits[b] == single, (name, max_range)             # same partial-sum layout: the same bits
            if name == "empty":
                assert fits[b] == N.DBL_MAX and single == N.DBL_MAX
    # and the neighbours themselves, through the single object's search (the batch entry returns nothing but the score)
    for b, (name, T, src) in enumerate(members):
        if len(src):
            same(regs[b].nearestNeighbors(T), refs[b], name)


# ---- d. a wide target: the sort builder chosen by the key count, and the overflow error ---------------------------------------------------
@pytest.mark.parametrize("builder", [0, 1])
def test_wide_target_and_index_overflow(builder):
    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint, _capi

    tgt, q = N.wide_target(600.0), N.wide_queries(600.0)
    want = N.brute_nn(tgt, q)
    g = GeneralizedIterativeClosestPoint(device=0)
    if builder:
        g.setTuning(grid_builder=builder)
    g.setInputTarget(tgt)
    g.setInputSource(q)
    same(g.nearestNeighbors(None), want, ("wide", builder))
    same(g.nearestNeighbors(N.yaw_pose(0.5, (0.1, -0.1, 0.05))), N.brute_nn(tgt, q, N.yaw_pose(0.5, (0.1, -0.1, 0.05))), ("wide, posed", builder))
    with pytest.raises(_capi.RegistrationError) as ei:      # >= 3 000 x 3 000 coarse cells: ccells * 512 >= 2^32, found before any launch
        g.setInputTarget(N.wide_target(12000.0))
        g.nearestNeighbors(None)
    assert ei.value.status == -7                             # LSR_ERR_INDEX_OVERFLOW
    g.setInputTarget(tgt)
    same(g.nearestNeighbors(None), want, ("wide, after the error", builder))

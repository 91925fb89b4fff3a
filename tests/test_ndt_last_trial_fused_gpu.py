"""The fused pass of a line search's tenth trial (csrc/ndt.hip: PH_MT_LAST, NDT_PASS_FUSED): trial number max_step_iterations
ends the search whatever it returns, so the Hessian the search recomputes at its last step rides along in the trial's launch.
Score, gradient and pair count of the fused pass must be the bits of a gradient-only pass, its Hessian the bits of a pass with
Hessian; an align must walk the schedule of the CPU oracle with one launch less per search that runs to the cap."""
import numpy as np
import pytest

from lidarslam_ros2_amd import synth
from lidarslam_ros2_amd.posemath import pose_delta

pytestmark = pytest.mark.gpu

from ndt_variants import POSE_R_TOL, POSE_T_TOL  # noqa: E402  (tolerances: north_star)
from ndt_variants import tune as _tune  # noqa: E402

RES = 5.0
# quad kernel: automatic / 64 points per workgroup, LDS and compact global table; lane kernel: 512 / 1024 threads, split form
PASS_VARIANTS = [(1, 0, 2), (1, 64, 2), (1, 0, 1), (0, 512, 2), (0, 1024, 0), (0, 512, 2, 1)]
# a partial chunk, exactly one chunk, the second chunk of a 128-point batch, several workgroups of the quad kernel (300) and of
# the lane kernel (1100)
SIZES = [1, 63, 64, 65, 127, 128, 129, 300, 1100]


def make_ndt(eps=0.01, max_iter=None):
    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform

    ndt = NormalDistributionsTransform(device=0)
    ndt.setResolution(RES)
    ndt.setTransformationEpsilon(eps)
    ndt.setNeighborhoodSearchMethod(DIRECT7)
    if max_iter is not None:
        ndt.setMaximumIterations(max_iter)
    return ndt


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def pass_case():
    c = synth.small_case(n_source=1100, n_keyframes=3)
    return c, np.ascontiguousarray(c.target[::4])   # a few thousand target points: the table fits LDS at this resolution


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.mark.parametrize("variant", PASS_VARIANTS)
def test_fused_pass_has_the_bits_of_both_plain_passes(O, pass_case, variant):
    case, target = pass_case
    ndt = make_ndt()
    _tune(ndt, variant)
    ndt.setInputTarget(synth.as_pointxyzi(target))
    if variant[2] == 2:
        assert ndt.gridInfo()["n_valid"] > 0
    p0 = O.matrix_to_pose(case.guess)
    poses = [p0 + np.r_[0.3, -0.2, 0.05, 0.01, -0.015, 0.02], p0 + np.r_[-0.1, 0.25, 0.0, -0.02, 0.01, 0.03]]
    saw_pairs = False
    for n in SIZES:
        ndt.setInputSource(synth.as_pointxyzi(case.source[:n]))
        for p in poses:
            s0, g0, _, n0 = ndt.derivatives(p, compute_hessian=False, with_pairs=True)
            s1, g1, H1, n1 = ndt.derivatives(p, compute_hessian=True, with_pairs=True)
            s2, g2, H2, n2 = ndt.derivatives(p, compute_hessian=2, with_pairs=True)
            assert np.array_equal(bits(s2), bits(s0)) and np.array_equal(bits(g2), bits(g0)) and np.array_equal(bits(n2), bits(n0)), (n, variant)
            assert np.array_equal(bits(H2), bits(H1)), (n, variant)
            assert n1 == n0
            saw_pairs = saw_pairs or (n0 > 0 and np.any(H1 != 0))
    assert saw_pairs, "the poses must put source points into target voxels"


# ---- align level ------------------------------------------------------------------------------------------------------
# Chosen on the CPU: of 200 random (seed, size, guess offset) draws of synth.small_case, one whose oracle registration has searches
# that run to the tenth trial AND searches that stop earlier, and for which the oracle's controller walks the same schedule of
# evaluations on the oracle's arithmetic and on the kernels' fp32 operation order (tests/ndt_host_emu.py).
ALIGN_SEED, ALIGN_N, ALIGN_OFFSET, ALIGN_ITERS = 17, 3000, (0.036, -0.032, -0.0018), 12
MAX_STEP_ITERATIONS = 10


@pytest.fixture(scope="module")
def align_case(O):
    case = synth.small_case(n_source=ALIGN_N, n_keyframes=4, seed=ALIGN_SEED, guess_perturb=ALIGN_OFFSET)
    ref = O.ndt_align(O.VoxelGridCovariance(case.target, RES), case.source, case.guess, resolution=RES, trans_eps=0.0,
                      max_iterations=ALIGN_ITERS, trace=True)
    # evaluations per Newton iteration: 1 = step accepted at once, 2 + k = k trials and the Hessian recomputation
    per_iter = np.diff(np.r_[1.0, ref["trace"][:, 8]]).astype(int)
    capped = int((per_iter == 2 + MAX_STEP_ITERATIONS).sum())
    early = int(((per_iter > 1) & (per_iter < 2 + MAX_STEP_ITERATIONS)).sum())
    return case, ref, capped, early


def test_align_folds_the_hessian_into_the_tenth_trial(align_case):
    from lidarslam_ros2_amd import align_batch

    case, ref, capped, early = align_case
    assert capped >= 3 and early >= 1, (capped, early)   # the oracle alone: the fused path and the plain recomputation both run
    total = ref["n_evals"] + ref["n_evals_grad"] + ref["n_hessian_recompute"]
    tgt, src = synth.as_pointxyzi(case.target), synth.as_pointxyzi(case.source)

    ndt = make_ndt(eps=0.0, max_iter=ALIGN_ITERS)
    ndt.setInputTarget(tgt)
    ndt.setInputSource(src)
    ndt.setProfiling(True)
    ndt.getProfile(reset=True)
    ndt.align(case.guess)
    prof = ndt.getProfile(reset=True)
    ndt.setProfiling(False)
    T, r = ndt.getFinalTransformation().copy(), ndt.last_result
    dt, ang = pose_delta(T, ref["final"])
    print("fused align: dt %.3g ang %.3g iterations %d/%d score %.17g/%.17g n_evaluations %d/%d launches %d capped %d early %d"
          % (dt, ang, r["iterations"], ref["iterations"], r["score"], ref["trans_probability"], r["n_evaluations"], total,
             prof["deriv_launches"], capped, early))
    assert dt <= POSE_T_TOL and ang <= POSE_R_TOL
    assert r["iterations"] == ref["iterations"]
    assert abs(r["score"] - ref["trans_probability"]) <= 1e-5 * abs(ref["trans_probability"])
    assert r["n_evaluations"] == total
    assert prof["deriv_launches"] == r["n_evaluations"] - capped   # one launch less per search that ran to the cap

    # the same registration twice in one set (lane kernel): the same bits, the same counts
    peer = make_ndt(eps=0.0, max_iter=ALIGN_ITERS)
    peer.shareTargetOf(ndt)
    peer.setInputSource(src)
    finals, results = align_batch([ndt, peer], [case.guess, case.guess])
    for b in range(2):
        assert np.array_equal(finals[b], T), (b, pose_delta(finals[b], T))
        assert results[b]["iterations"] == r["iterations"] and results[b]["n_evaluations"] == r["n_evaluations"], b

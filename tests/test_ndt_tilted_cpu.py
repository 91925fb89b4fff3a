"""NDT on tilted attitudes, the part that needs no GPU (tests/tilted_cases.py has the frames).

1. The guess decomposition of the library (lsr_debug_guess_pose: the p that ndt_fill_initial_state stores; csrc/ndt.hip euler012_f)
   against the oracle's (O.matrix_to_pose), bit for bit, on both branches of Eigen's eulerAngles(0,1,2).
2. The guard for the inputs of tests/test_ndt_tilted_gpu.py: on every input the GPU file uses, the kernels' arithmetic evaluated
   on the host (tests/ndt_host_emu.py) agrees with the oracle ten times closer than the bars the device is held to, and a
   registration driven by it takes the oracle's iterations — a GPU failure there is then the device's, not the input's.
All six frames of tilted_cases.FRAMES pass the guard; one input was replaced (frame "far", 65 points: tilted_cases.REPLACED_SIZES)."""
import ctypes as C

import numpy as np
import pytest

from lidarslam_ros2_amd import synth
from lidarslam_ros2_amd.posemath import pose_delta

import ndt_host_emu as E
import tilted_cases as TC
from ndt_variants import POSE_R_TOL, POSE_T_TOL


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def guess_pose(M):
    """lsr_debug_guess_pose of a 4x4 (None: the null guess)."""
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    p = np.zeros(6)
    gp = None
    if M is not None:
        g = np.ascontiguousarray(np.asarray(M, np.float32).T).reshape(-1)
        gp = g.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.lsr_debug_guess_pose(gp, p.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return p


def _attitudes():
    """(label, 4x4 fp32) guesses: >= 2000 random attitudes, the six guesses of the frames, and the edges of the decomposition."""
    rng = np.random.default_rng(2024)
    out = []
    for k in range(2400):
        t = rng.uniform(-50, 50, 3)
        out.append(("random%d" % k, synth.pose_matrix(t[0], t[1], t[2], rng.uniform(-3.1, 3.1), roll=rng.uniform(-3.1, 3.1),
                                                       pitch=rng.uniform(-1.5, 1.5))))
    edges = [(0.0, 0.3, 0.2), (0.0, -0.3, -2.9), (0.0, 0.0, 1.0),                       # roll exactly 0
             (1e-7, 0.2, 0.5), (-1e-7, 0.2, 0.5), (1e-7, 0.0, 0.0), (-1e-7, 0.0, 0.0),  # roll = +-1e-7
             (0.05, 0.04, np.pi), (0.05, 0.04, -np.pi), (-0.05, 0.04, np.pi), (-0.05, -0.04, -np.pi), (0.0, 0.0, np.pi), (0.0, 0.0, -np.pi),
             (0.3, np.pi / 2 - 1e-3, 0.4), (0.3, -(np.pi / 2 - 1e-3), 0.4), (-0.3, np.pi / 2 - 1e-3, -2.0), (-0.3, -(np.pi / 2 - 1e-3), 2.0)]
    for roll, pitch, yaw in edges:
        out.append(("edge(%g,%g,%g)" % (roll, pitch, yaw), synth.pose_matrix(1.5, -2.5, 0.5, yaw, roll=roll, pitch=pitch)))
    for name in TC.FRAME_NAMES:
        out.append(("frame " + name, TC.tilted(name).guess))
    out.append(("identity", np.eye(4)))
    return [(label, np.asarray(M, np.float32)) for label, M in out]


def test_guess_decomposition_equals_the_oracle_bit_for_bit(O):
    """lsr_debug_guess_pose == O.matrix_to_pose, equal bits (both restate Eigen 3.4's eulerAngles(0,1,2) in fp32 on one libm), over
    2400 random attitudes (roll, yaw over +-3.1, pitch over +-1.5), the guesses of the six frames, roll = 0 and +-1e-7, yaw = +-pi,
    pitch = +-(pi/2 - 1e-3), the identity and the null guess.  Both branches are hit: between 0.3 and 0.7 of the random attitudes
    come back as the alias (second angle outside [-pi/2, pi/2]).  The matrix rebuilt from p is the guess to 2e-6."""
    flipped = n_random = 0
    for label, M in _attitudes():
        p, ref = guess_pose(M), O.matrix_to_pose(M)
        assert np.array_equal(p.view(np.uint64), ref.view(np.uint64)), (label, p, ref)
        assert np.array_equal(p, p.astype(np.float32).astype(np.float64))      # fp32 angles and translation, widened
        assert np.array_equal(p[:3], M[:3, 3].astype(np.float64))
        assert -1e-6 <= p[3] <= np.pi + 1e-6, (label, p)                        # Eigen's range of the first angle
        back = O.pose_to_matrix(p)
        dt, ang = pose_delta(back, M)
        assert dt < 1e-6 and ang < 2e-6, (label, dt, ang)
        assert np.allclose(back[:3, :3], M[:3, :3], atol=2e-6), label
        if label.startswith("random"):
            n_random += 1
            # the alias branch is taken when atan2(R[1,2], R[2,2]) > 0, i.e. R[1,2] = -sin(roll) cos(pitch) > 0; only there the
            # second angle leaves [-pi/2, pi/2]
            flipped += bool(abs(p[4]) > np.pi / 2)
            assert bool(abs(p[4]) > np.pi / 2) == bool(M[1, 2] > 0), (label, p)
    assert n_random >= 2000 and 0.3 <= flipped / n_random <= 0.7, (flipped, n_random)
    # the frames' own guesses: three on the alias branch, with all three angles near +-pi
    for name in TC.FRAME_NAMES:
        p = guess_pose(TC.tilted(name).guess)
        assert (abs(p[4]) > np.pi / 2) == (name in TC.FLIPPED) and (p[3] > 3.0) == (name in TC.FLIPPED), (name, p)
    assert np.array_equal(guess_pose(None), np.zeros(6)) and np.array_equal(guess_pose(np.eye(4)), O.matrix_to_pose(np.eye(4)))
    assert np.array_equal(guess_pose(None), guess_pose(np.eye(4)))
    from lidarslam_ros2_amd import _capi
    assert _capi.load().lsr_debug_guess_pose(None, None) == -1                  # LSR_ERR_INVALID_ARGUMENT


def test_repose_is_the_same_problem_in_another_frame():
    """target' = W target, guess' = W guess, truth' = W truth; the source is the base case's; blocks() takes each block over its own
    largest reference entry and refuses a non-zero value where the reference block is all zero."""
    c = TC.base_case()
    for name in TC.FRAME_NAMES:
        w, W = TC.tilted(name), TC.frame_matrix(name)
        assert w.source is c.source and w.target.dtype == np.float32 and w.guess.dtype == np.float32
        back = (w.target.astype(np.float64) - W[:3, 3]) @ W[:3, :3]
        assert np.abs(back - c.target).max() < 2e-5                             # fp32 rounding of coordinates below 200 m
        d0, a0 = pose_delta(c.guess, c.truth)
        d1, a1 = pose_delta(w.guess, w.truth)
        assert abs(d0 - d1) < 1e-5 and abs(a0 - a1) < 1e-6
    g, H = np.arange(1.0, 7.0), np.diag([1.0, 1, 1, 400, 400, 400])
    H2 = H.copy()
    H2[0, 0] += 0.0075                                                          # 0.75 % of a translation entry: under 2e-5 of the whole matrix
    d = TC.blocks((1.0, g, H2), (1.0, g, H))
    assert d["H_tt"] == pytest.approx(0.0075) and d["H_rr"] == 0.0 and np.abs(H2 - H).max() <= 2e-5 * np.abs(H).max()
    with pytest.raises(AssertionError):
        TC.assert_blocks((1.0, g, H2), (1.0, g, H))
    H3 = H.copy()
    H3[0, 4] = 1e-30                                                            # the reference's H_tr is all zero
    assert TC.blocks((1.0, g, H3), (1.0, g, H))["H_tr"] == float("inf") and TC.blocks((1.0, g, H), (1.0, g, H))["H_tr"] == 0.0
    with pytest.raises(AssertionError):
        TC.assert_blocks((1.0, g, H3), (1.0, g, H))
    assert TC.assert_blocks((1.0 + 5e-7, g, H), (1.0, g, H), margin=0.1)["score"] == pytest.approx(5e-7, rel=1e-3)
    with pytest.raises(AssertionError):
        TC.assert_blocks((1.0 + 2e-6, g, H), (1.0, g, H), margin=0.1)


@pytest.mark.parametrize("name", TC.FRAME_NAMES)
def test_emulation_meets_a_tenth_of_the_bars_on_every_gpu_input(O, name):
    """For every (frame, size, pose, Hessian form) of the GPU file: host emulation against O.ndt_derivatives, block by block, at
    margin 0.1 (score 1e-6, each other block 2e-6).  Largest values seen per frame (pytest -s prints them):
              score    g_t      g_r      H_tt     H_tr     H_rr
      flat    7.2e-08  2.5e-07  3.4e-07  2.3e-07  1.8e-07  1.1e-07
      roll+   8.8e-08  1.8e-07  9.4e-07  1.1e-07  8.8e-08  1.1e-07
      roll-   6.5e-08  1.3e-06  3.9e-07  5.7e-07  5.1e-07  4.1e-07
      far     1.4e-07  1.9e-06  6.4e-07  8.6e-07  8.1e-07  2.0e-06
      steep   2.1e-07  2.9e-07  7.8e-07  2.4e-07  2.9e-07  7.2e-07
      tiny-   1.6e-07  1.1e-07  1.4e-07  2.6e-07  9.8e-08  1.9e-07
    The large ones are pose-form rows of the flipped frames at 63 .. 65 points (few points, a small |g_t|; the pose-form transform is
    composed in fp32 from angles near pi).  One input did not pass and was replaced: frame "far", 65 points, pose form, g_t 2.19e-6
    (tilted_cases.REPLACED_SIZES: 193 points instead, 2.5e-7)."""
    w = TC.tilted(name)
    worst = {}
    for n in TC.sizes(name):
        emu = E.Emu(O, w.grid(O), w.source[:n], TC.RES)
        for pname, p, T in w.poses(O):
            for form in TC.HESSIAN_FORMS:
                ref = TC.oracle_pass(O, w, n, p, T, form)
                TC.assert_blocks(TC.emu_pass(emu, p, T, form), ref, margin=0.1, label=(name, n, pname, form), worst=worst)
        emu.close()
    print("\n[tilted cpu] %-6s emulation vs oracle: %s" % (name, TC.fmt(worst)))


def test_emulation_meets_a_tenth_of_the_bars_on_the_snap_grid(O):
    """Frame "flat", 2000 points, pose form, each angle on or off the 1e-4 small-angle snap of the angle tables
    (tilted_cases.SNAP_ANGLES: 14 combinations, all snapped, none, one axis only): the same guard.  Largest values seen:
    score 3.0e-09  g_t 1.4e-08  g_r 5.4e-08  H_tt 8.2e-09  H_tr 2.9e-08  H_rr 6.0e-08."""
    assert len(TC.SNAP_ANGLES) >= 12 and len(set(TC.SNAP_ANGLES)) == len(TC.SNAP_ANGLES)
    snapped = [tuple(abs(a) < 1e-4 for a in ang) for ang in TC.SNAP_ANGLES]
    assert (True, True, True) in snapped and (False, False, False) in snapped
    assert {(False, True, True), (True, False, True), (True, True, False)} <= set(snapped)      # one axis only off the snap
    assert {(True, False, False), (False, True, False), (False, False, True)} <= set(snapped)   # one axis only on it
    w = TC.tilted("flat")
    emu = E.Emu(O, w.grid(O), w.source, TC.RES)
    worst = {}
    for p in TC.snap_poses(O):
        for form in TC.HESSIAN_FORMS:
            TC.assert_blocks(TC.emu_pass(emu, p, None, form), TC.oracle_pass(O, w, TC.N_SOURCE, p, None, form), margin=0.1,
                             label=(tuple(p[3:]), form), worst=worst)
    emu.close()
    print("\n[tilted cpu] snap grid emulation vs oracle: %s" % TC.fmt(worst))


@pytest.mark.parametrize("name", TC.FRAME_NAMES)
def test_emulation_driven_registration_follows_the_oracle(O, name):
    """Both schedules (eps 0.01 / 35 iterations, eps 1e-6 / 30) on every frame: the oracle converges within 0.1 m of truth', and the
    registration driven by the host emulation ends within a tenth of the north-star bars of it; at eps 0.01 with the same iteration count and the
    same evaluation schedule (trace[:, 8]: derivative passes so far).  Iteration counts, oracle / emulation, eps 0.01 and eps 1e-6:
    flat 7/7, 8/8; roll+ 7/7, 8/8; roll- 6/6, 25/25; far 7/7, 7/7; steep 7/7, 8/8; tiny- 7/7, 8/8.  Final poses apart by at most
    4.6e-6 m / 1.8e-6 rad (frame "steep")."""
    w = TC.tilted(name)
    line, worst_pose = [], (0.0, 0.0)
    for eps, max_iter in TC.SCHEDULES:
        ref = w.oracle_align(O, eps, max_iter, trace=True)
        emu = E.ndt_align(O, w.grid(O), w.source, w.guess, TC.RES, trans_eps=eps, max_iterations=max_iter, trace=True)
        line.append("eps %g: %d / %d" % (eps, ref["iterations"], emu["iterations"]))
        assert ref["converged"] and emu["converged"]
        gt, _ = pose_delta(ref["final"], w.truth)
        assert gt < 0.1, (name, eps, gt)
        dt, ang = pose_delta(ref["final"], emu["final"])
        assert dt <= 0.1 * POSE_T_TOL and ang <= 0.1 * POSE_R_TOL, (name, eps, dt, ang)
        worst_pose = (max(worst_pose[0], dt), max(worst_pose[1], ang))
        if eps == 0.01:
            assert emu["iterations"] == ref["iterations"]
            assert np.array_equal(ref["trace"][:, 8], emu["trace"][:, 8])
            assert TC.n_passes(emu) == TC.n_passes(ref), name      # what the GPU file asserts of n_evaluations
    print("\n[tilted cpu] %-6s iterations oracle / emulation: %s; final poses apart by %.1e m %.1e rad" % ((name, ", ".join(line)) + worst_pose))
    assert sum(n in TC.FLIPPED for n in TC.FRAME_NAMES) >= 3 and len(TC.FRAME_NAMES) >= 5


def _same_run(emu, ref, label):
    """The guard for what the GPU file asserts of a truncated registration beyond the pose: the number of derivative passes, and the
    score of the last pass at a tenth of the score bar.  (Not asserted of the full registrations: in frame "steep" the emulation's
    last score is 1.1e-5 from the oracle's, the last step there being 4.6e-6 m apart on a slope.)"""
    assert TC.n_passes(emu) == TC.n_passes(ref), label
    rel = abs(emu["trans_probability"] - ref["trans_probability"]) / abs(ref["trans_probability"])
    assert rel <= 0.1 * TC.SCORE_TOL, (label, rel)
    return rel


@pytest.mark.parametrize("name", TC.TRUNCATED_FRAMES)
def test_emulation_driven_truncated_registrations_follow_the_oracle(O, name):
    """max_iterations = 0 .. the full count on "roll-" and "roll+" (the reference checks its limit before it counts: k gives k + 2
    iterations): the emulation-driven registration takes the oracle's iterations and passes and ends on its score (largest relative
    difference 1.5e-8) and, to a tenth of the north-star bars, on its pose."""
    w = TC.tilted(name)
    full = w.oracle_align(O, 0.01, 35, trace=True)["iterations"]
    worst = 0.0
    for k in range(full + 1):
        ref = w.oracle_align(O, 0.01, k)
        emu = E.ndt_align(O, w.grid(O), w.source, w.guess, TC.RES, trans_eps=0.01, max_iterations=k)
        assert emu["iterations"] == ref["iterations"] == min(k + 2, full), (name, k)
        dt, ang = pose_delta(ref["final"], emu["final"])
        assert dt <= 0.1 * POSE_T_TOL and ang <= 0.1 * POSE_R_TOL, (name, k, dt, ang)
        worst = max(worst, _same_run(emu, ref, (name, k)))
    print("\n[tilted cpu] %-6s truncated 0 .. %d: largest relative score difference %.1e" % (name, full, worst))

"""NDT (and GICP) on tilted attitudes on the device, against the CPU oracle on the same inputs (tests/tilted_cases.py has the frames,
tests/test_ndt_tilted_cpu.py the guard that shows the kernels' arithmetic meets a tenth of these bars on every input used here).

Every other GPU test of the NDT path runs yaw-only: most of the 72 j_ang / h_ang entries then vanish or sit at +-1, and the guess
never leaves Eigen's eulerAngles(0,1,2) on its alias branch.  Here the guess carries roll and pitch, in three of six frames on the
alias branch (all three angles near +-pi), and one derivative pass is compared block by block — translation and rotation parts of
the gradient and of the Hessian each over their own largest entry — so that the rotation block (~400 times the translation block)
cannot hide an error in the other entries.  Bars: the project's existing ones (ndt_variants.py), per block.
`pytest -s` prints the largest value seen per block.
Checked once on a scratch build: with the sx*sy entry of j_ang (entry 11) mis-signed in the scalar formulas and in LSR_ANGLE_ENTRIES, the
nine derivative tests here fail by 50 to 500 times the bar.  Mis-signed in LSR_ANGLE_ENTRIES alone (which only align()'s request builder
on the device reads; derivatives() takes its tables from the host), nothing here fails: the registrations still end within the bars
("Tilted attitudes").  tests/test_host_cpu.py and the guard in tests/test_ndt_tilted_cpu.py see that one."""
import dataclasses

import numpy as np
import pytest

from lidarslam_ros2_amd import synth
from lidarslam_ros2_amd.posemath import pose_delta

import tilted_cases as TC
from ndt_variants import POSE_R_TOL, POSE_T_TOL

pytestmark = pytest.mark.gpu

KERNELS = ("quad", "lane")          # the automatic quad kernel; setTuning(quad=0, workgroup=512)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def make_ndt(kernel="quad", eps=0.01, max_iter=35, neighborhood="DIRECT7"):
    import lidarslam_ros2_amd as L

    ndt = L.NormalDistributionsTransform(device=0)
    ndt.setResolution(TC.RES)
    ndt.setTransformationEpsilon(eps)
    ndt.setMaximumIterations(max_iter)
    ndt.setNeighborhoodSearchMethod(getattr(L, neighborhood))
    if kernel == "lane":
        ndt.setTuning(quad=0, workgroup=512)
    return ndt


def _pair_of_kernels(w, neighborhood="DIRECT7"):
    regs = [make_ndt(k, neighborhood=neighborhood) for k in KERNELS]
    for r in regs:
        r.setInputTarget(synth.as_pointxyzi(w.target))
    return regs


def _both_kernels_against(regs, p, T, form, ref, label, worst):
    """One pass through both kernels: equal bits and equal pair counts between them, the oracle's blocks at margin 1."""
    a = regs[0].derivatives(p, T=T, compute_hessian=form, with_pairs=True)
    b = regs[1].derivatives(p, T=T, compute_hessian=form, with_pairs=True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), label
    assert a[3] == b[3], (label, a[3], b[3])
    TC.assert_blocks(a[:3], ref, label=label, worst=worst)
    return a


@pytest.mark.parametrize("name", TC.FRAME_NAMES)
def test_derivative_pass_block_by_block(O, name):
    """DIRECT7, source prefixes of 1, 63, 64, 65, 129 and 2000 points (tilted_cases.sizes: 193 for 65 in frame "far"), the guess in
    matrix form and an offset pose in pose form, compute_hessian True / False / 2, through the quad kernel and the 512-thread lane
    kernel."""
    w = TC.tilted(name)
    regs = _pair_of_kernels(w)
    worst, hit = {}, 0
    for n in TC.sizes(name):
        for r in regs:
            r.setInputSource(synth.as_pointxyzi(w.source[:n]))
        for pname, p, T in w.poses(O):
            refs = {h: TC.oracle_pass(O, w, n, p, T, h) for h in (True, False)}
            for form in TC.HESSIAN_FORMS:
                a = _both_kernels_against(regs, p, T, form, refs[bool(form)], (name, n, pname, form), worst)
                hit += a[3] > 0
    assert hit >= 30                                      # the prefixes do meet voxels: not a comparison of zeros
    print("\n[tilted gpu] %-6s DIRECT7 device vs oracle: %s" % (name, TC.fmt(worst)))


@pytest.mark.parametrize("neighborhood,search", [("DIRECT1", 1), ("DIRECT26", 26), ("KDTREE", 0)])
def test_derivative_pass_block_by_block_other_neighbourhoods(O, neighborhood, search):
    """Frames "roll-" (alias branch) and "steep" at 2000 points, both poses, with and without Hessian, both kernels."""
    worst = {}
    for name in ("roll-", "steep"):
        w = TC.tilted(name)
        regs = _pair_of_kernels(w, neighborhood)
        for r in regs:
            r.setInputSource(synth.as_pointxyzi(w.source))
        for pname, p, T in w.poses(O):
            for form in (True, False):
                ref = TC.oracle_pass(O, w, TC.N_SOURCE, p, T, form, search=search)
                a = _both_kernels_against(regs, p, T, form, ref, (name, neighborhood, pname, form), worst)
                assert a[3] > 0
    print("\n[tilted gpu] %-8s device vs oracle: %s" % (neighborhood, TC.fmt(worst)))


def test_derivative_pass_on_the_snap_grid(O):
    """Frame "flat", 2000 points, pose form, each angle on or off the 1e-4 small-angle snap (tilted_cases.SNAP_ANGLES)."""
    w = TC.tilted("flat")
    regs = _pair_of_kernels(w)
    for r in regs:
        r.setInputSource(synth.as_pointxyzi(w.source))
    worst = {}
    for p in TC.snap_poses(O):
        refs = {h: TC.oracle_pass(O, w, TC.N_SOURCE, p, None, h) for h in (True, False)}
        for form in TC.HESSIAN_FORMS:
            _both_kernels_against(regs, p, None, form, refs[bool(form)], (tuple(p[3:]), form), worst)
    print("\n[tilted gpu] snap grid device vs oracle: %s" % TC.fmt(worst))


@pytest.mark.parametrize("eps,max_iter", TC.SCHEDULES)
def test_registration_in_every_frame(O, eps, max_iter):
    """Every frame through the quad kernel, the lane kernel and all six as one align_batch: the three forms return equal bits and
    equal evaluation counts; against the oracle the north-star bars, equal hasConverged, equal iteration counts at eps 0.01 (the CPU
    guard shows the emulation-driven registration agrees there), under 0.1 m from truth'."""
    from lidarslam_ros2_amd import align_batch

    worlds = [TC.tilted(name) for name in TC.FRAME_NAMES]
    singles, quads = [], []
    for w in worlds:
        per_kernel = []
        for k in KERNELS:
            r = make_ndt(k, eps, max_iter)
            r.setInputTarget(synth.as_pointxyzi(w.target))
            r.setInputSource(synth.as_pointxyzi(w.source))
            r.align(w.guess)
            per_kernel.append((r.getFinalTransformation().copy(), r.getFinalNumIteration(), r.last_result["n_evaluations"], r.hasConverged()))
            if k == "quad":
                quads.append(r)
        assert np.array_equal(per_kernel[0][0], per_kernel[1][0]) and per_kernel[0][1:] == per_kernel[1][1:], w.name
        singles.append(per_kernel[0])
    finals, results = align_batch(quads, [w.guess for w in worlds])
    worst_t = worst_r = 0.0
    for b, w in enumerate(worlds):
        T, iters, n_evals, conv = singles[b]
        assert np.array_equal(finals[b], T), (w.name, pose_delta(finals[b], T))
        assert results[b]["iterations"] == iters and results[b]["n_evaluations"] == n_evals and results[b]["converged"] == conv, w.name
        ref = w.oracle_align(O, eps, max_iter, trace=True)
        dt, ang = pose_delta(T, ref["final"])
        worst_t, worst_r = max(worst_t, dt), max(worst_r, ang)
        print("\n[tilted gpu] %-6s eps %g: %d iterations (oracle %d), %.1e m %.1e rad from the oracle" % (w.name, eps, iters, ref["iterations"], dt, ang), end="")
        assert dt <= POSE_T_TOL and ang <= POSE_R_TOL, (w.name, dt, ang, iters, ref["iterations"])
        assert conv == ref["converged"], w.name
        if eps == 0.01:
            assert iters == ref["iterations"] and n_evals == TC.n_passes(ref), (w.name, iters, n_evals)
        gt, _ = pose_delta(T, w.truth)
        assert gt < 0.1, (w.name, gt)
    print("\n[tilted gpu] eps %g: largest distance to the oracle %.1e m %.1e rad" % (eps, worst_t, worst_r))


@pytest.mark.parametrize("name", TC.TRUNCATED_FRAMES)
def test_truncated_registrations_step_by_step(O, name):
    """setMaximumIterations(k) for k = 0 .. the full count on both branches of the decomposition, each against
    O.ndt_align(max_iterations=k): the controller's pose update, the device's request builder and the stale-h_ang rule one Newton
    step at a time.  North-star bars, equal iteration counts."""
    w = TC.tilted(name)
    full = w.oracle_align(O, 0.01, 35, trace=True)["iterations"]
    ndt = make_ndt()
    ndt.setInputTarget(synth.as_pointxyzi(w.target))
    ndt.setInputSource(synth.as_pointxyzi(w.source))
    worst_t = worst_r = worst_s = 0.0
    for k in range(full + 1):
        ref = w.oracle_align(O, 0.01, k)
        ndt.setMaximumIterations(k)
        ndt.align(w.guess)
        dt, ang = pose_delta(ndt.getFinalTransformation(), ref["final"])
        worst_t, worst_r = max(worst_t, dt), max(worst_r, ang)
        assert dt <= POSE_T_TOL and ang <= POSE_R_TOL, (name, k, dt, ang)
        assert ndt.getFinalNumIteration() == ref["iterations"] == min(k + 2, full), (name, k)   # the reference counts after its check
        assert ndt.hasConverged() == ref["converged"], (name, k)
        # the passes so far and the score of the last one (the guard shows 1.5e-8 for the kernels' arithmetic): a step taken with a
        # wrong j_ang / h_ang entry ends on another slope long before it moves the pose by the north-star bar
        assert ndt.last_result["n_evaluations"] == TC.n_passes(ref), (name, k)
        rel = abs(ndt.last_result["score"] - ref["trans_probability"]) / abs(ref["trans_probability"])
        worst_s = max(worst_s, rel)
        assert rel <= TC.SCORE_TOL, (name, k, rel)
    print("\n[tilted gpu] %-6s truncated at 0 .. %d iterations: largest distance to the oracle %.1e m %.1e rad, score %.1e" %
          (name, full, worst_t, worst_r, worst_s))


@pytest.fixture(scope="module")
def gicp_base():
    c = TC.base_case()
    # the GICP frontend re-filters the target at vg_size_for_input (as tests/test_gicp_gpu.py does)
    return dataclasses.replace(c, target=synth.voxel_downsample(c.target, 0.4))


@pytest.mark.parametrize("name", ["flat", "roll-", "far", "steep"])
def test_gicp_align_in_tilted_frames(O, gicp_base, name):
    """GICP's pose extraction (csrc/gicp.hip) has only run yaw-only: both inner solvers against O.gicp_align with the matching solver,
    settings of tests/test_gicp_gpu.py::test_align_matches_oracle (correspondence distance 5, epsilon 1e-8), north-star bars, under
    0.1 m from truth'."""
    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint

    target, guess, truth = TC.repose(gicp_base, TC.frame_matrix(name))
    source = gicp_base.source
    nt, ns = O.NearestNeighbour(target, 1.0), O.NearestNeighbour(source, 1.0)
    ct, cs = O.gicp_covariances(nt, target), O.gicp_covariances(ns, source)
    for optimizer, solver in (("gauss_newton", 1), ("bfgs", 0)):
        g = GeneralizedIterativeClosestPoint(device=0)
        g.setMaxCorrespondenceDistance(5.0)
        g.setTransformationEpsilon(1e-8)
        g.setOptimizer(optimizer)
        g.setInputTarget(synth.as_pointxyzi(target))
        g.setInputSource(synth.as_pointxyzi(source))
        g.align(guess)
        T = g.getFinalTransformation()
        ref = O.gicp_align(nt, target, ct, source, cs, guess, max_corr_dist=5.0, trans_eps=1e-8, solver=solver)
        dt, ang = pose_delta(T, ref["final"])
        print("\n[tilted gpu] %-6s GICP %-12s %.1e m %.1e rad from the oracle (%d iterations, oracle %d)" %
              (name, optimizer, dt, ang, g.last_result["iterations"], ref["iterations"]), end="")
        assert dt <= POSE_T_TOL and ang <= POSE_R_TOL, (name, optimizer, dt, ang)
        assert g.hasConverged() and ref["converged"], (name, optimizer)
        gt, _ = pose_delta(T, truth)
        assert gt < 0.1, (name, optimizer, gt)

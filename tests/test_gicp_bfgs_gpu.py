"""GPU parity of the BFGS inner optimiser of GICP (LSR_GICP_SOLVER = LSR_GICP_BFGS, csrc/gicp.hip: gicp_bfgs_step_kernel +
csrc/gicp_bfgs.hpp): the 13-sum cost/gradient pass against the oracle's functor, one inner loop against the host build of the
same automaton fed by the oracle's functor, the align against the oracle's BFGS align, and the launch chain's guarantees."""
import numpy as np
import pytest

import gicp_bfgs_cases as K
import gicp_numpy as GN
from lidarslam_ros2_amd import synth
from lidarslam_ros2_amd.posemath import pose_delta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def case():
    c = synth.small_case(n_source=4000, n_keyframes=3)
    c.target = synth.voxel_downsample(c.target, 0.4)     # the case tests/test_gicp_gpu.py uses
    return c


@pytest.fixture(scope="module")
def oracle_cov(O, case):
    nt, ns = O.NearestNeighbour(case.target, 1.0), O.NearestNeighbour(case.source, 1.0)
    return nt, O.gicp_covariances(nt, case.target), O.gicp_covariances(ns, case.source)


def make_gicp(solver="bfgs", corr=5.0, eps=1e-8):
    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint

    g = GeneralizedIterativeClosestPoint(device=0)
    g.setMaxCorrespondenceDistance(corr)
    g.setTransformationEpsilon(eps)
    g.setOptimizer(solver)
    return g


def _pairs(lin):
    v = lin["valid"] != 0
    return lin["out"][v], lin["q"][v], GN.sym6_to_33(lin["M6"][v])


def test_solver_key_round_trip():
    from lidarslam_ros2_amd import _capi

    g = make_gicp("gauss_newton")
    assert g.getOptimizer() == "gauss_newton"
    g.setOptimizer("bfgs")
    assert g.getOptimizer() == "bfgs" and g._geti(_capi.GICP_SOLVER) == _capi.GICP_BFGS
    for bad in (-1, 2, 51):
        with pytest.raises(_capi.RegistrationError) as ei:
            g._seti(_capi.GICP_SOLVER, bad, "set")
        assert ei.value.status == -1           # LSR_ERR_INVALID_ARGUMENT
    assert g.getOptimizer() == "bfgs"
    with pytest.raises(ValueError):
        g.setOptimizer("lbfgs")


# ---- 5. the pass --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,box", [(100, 10.0), (4000, 40.0), (131072 + 300, 40.0)])
def test_pass_matches_the_oracles_functor(O, n, box):
    """One partly filled workgroup; sixteen workgroups; more than 512 x 256 points (the grid-stride loop).  f and g of the first
    record of the trace against oracle.gicp_cost on the same pairs at the same x: fp64 sums of up to ~1e5 terms in another order —
    rel 1e-12 on f, 1e-11 max|g| on g (the argument of the 1e-10 bar of test_covariances_match_oracle)."""
    rng = np.random.default_rng(n)
    target = rng.uniform(-box / 2, box / 2, (n, 3)).astype(np.float32)
    a = 0.01
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    source = ((target.astype(np.float64) - [0.05, -0.03, 0.02]) @ Rz).astype(np.float32)   # target moved by a small pose
    g = make_gicp()
    g.setInputTarget(target)
    g.setInputSource(source)
    lin = g.linearize()
    tr = g.bfgs_trace(capacity=4)
    assert tr["m"] == lin["m"] >= n - n // 50 and tr["n_evals"] >= 2
    src, tgt, M = _pairs(lin)
    assert src.shape[0] == tr["m"]
    assert np.array_equal(tr["x"][0], lin["x6"]) and tr["inner"][0] == 0
    f, grad = O.gicp_cost(src, tgt, M, tr["x"][0])
    ef, eg = abs(tr["f"][0] - f) / abs(f), np.abs(tr["g"][0] - grad).max() / np.abs(grad).max()
    print("n = %d: m = %d, f %.17g rel %.2e, max|g| %.3e rel %.2e" % (n, tr["m"], f, ef, np.abs(grad).max(), eg))
    assert ef <= 1e-12
    assert eg <= 1e-11
    # the trace held four records of more: the count is the whole loop's
    assert tr["x"].shape[0] == min(4, tr["n_evals"])


# ---- 6. the inner loop ----------------------------------------------------------------------------------------------------------------
INNER_LOOP_BAR = 10 * 1.2e-12    # ten times the worst |dx| of the first run on an MI355X


def test_inner_loop_replays_on_the_host_automaton(O, case):
    """The first outer iteration's whole inner loop on the device against the SAME automaton on the host (tools/gicp_bfgs_host_emu)
    fed by the oracle's functor on the device's pairs: the same decisions (steps, evaluations, ending reason) and every evaluated x
    within INNER_LOOP_BAR (m, rad) — measured 1.2e-12 on the first run (51 evaluations, 13 steps, ends on no progress): f and g
    differ in the last bits (another summation order), the interpolations carry that on.  Above 1e-6 would be a bug."""
    g = make_gicp()
    g.setInputTarget(synth.as_pointxyzi(case.target))
    g.setInputSource(synth.as_pointxyzi(case.source))
    lin = g.linearize(case.guess)
    tr = g.bfgs_trace(case.guess)
    src, tgt, M = _pairs(lin)
    emu = K.run_automaton(lambda x: O.gicp_cost(src, tgt, M, x), tr["x"][0], 20)
    assert tr["n_inner"] == emu["n_inner"]
    assert tr["reason"] == emu["reason"], (tr["reason_name"], K.REASONS[emu["reason"]])
    assert tr["n_evals"] == emu["n_evals"] == tr["x"].shape[0]
    assert np.array_equal(tr["inner"], emu["inner"])
    worst = float(np.abs(tr["x"] - emu["points"]).max())
    print("inner loop: %d evaluations, %d steps, ends on %s, worst |dx| %.3e, final |dx| %.3e" %
          (tr["n_evals"], tr["n_inner"], tr["reason_name"], worst, float(np.abs(tr["x_final"] - emu["x"]).max())))
    assert worst <= INNER_LOOP_BAR
    assert np.abs(tr["x_final"] - emu["x"]).max() <= INNER_LOOP_BAR
    assert tr["n_evals"] > 20          # a real line-search workload: tens of passes in the first outer iteration
    # the inspection leaves no trace: the align that follows is the align without it
    g.align(case.guess)
    T1 = g.getFinalTransformation().copy()
    h = make_gicp()
    h.setInputTarget(synth.as_pointxyzi(case.target))
    h.setInputSource(synth.as_pointxyzi(case.source))
    h.align(case.guess)
    assert np.array_equal(T1, h.getFinalTransformation()) and g.last_result["n_evaluations"] == h.last_result["n_evaluations"]


# ---- 7. the align -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", [5.0, 30.0])
def test_bfgs_align_matches_the_oracles_bfgs_align(O, case, oracle_cov, corr):
    nt, ct, cs = oracle_cov
    ref = O.gicp_align(nt, case.target, ct, case.source, cs, case.guess, max_corr_dist=corr, trans_eps=1e-8, solver=0)
    g = make_gicp("bfgs", corr)
    g.setInputTarget(synth.as_pointxyzi(case.target))
    g.setInputSource(synth.as_pointxyzi(case.source))
    out = g.align(case.guess, output=True)
    T = g.getFinalTransformation()
    gn = make_gicp("gauss_newton", corr)
    gn.setInputTarget(synth.as_pointxyzi(case.target))
    gn.setInputSource(synth.as_pointxyzi(case.source))
    gn.align(case.guess)
    dt, ang = pose_delta(T, ref["final"])
    dt_gn, ang_gn = pose_delta(gn.getFinalTransformation(), ref["final"])
    print("corr %.0f: distance to the BFGS oracle  BFGS device %.3e m %.3e rad (%d passes)   Gauss-Newton device %.3e m %.3e rad" %
          (corr, dt, ang, g.last_result["n_evaluations"], dt_gn, ang_gn))
    assert g.last_result["iterations"] == ref["iterations"] == g.getFinalNumIteration()
    assert g.last_result["n_correspondences"] == ref["n_correspondences"]
    assert g.hasConverged() and ref["converged"]
    assert dt <= 1e-4 and ang <= 1e-5, (dt, ang, g.last_result, ref)       # the same-algorithm bar (tests/test_gicp_gpu.py)
    assert np.abs(out - (case.source @ T[:3, :3].T + T[:3, 3])).max() < 1e-4
    assert g.getFitnessScore() < 0.5
    assert abs(g.last_result["score"] - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
    assert g.last_result["n_evaluations"] > g.last_result["iterations"]


# ---- 8. the chain's guarantees under BFGS -----------------------------------------------------------------------------------------------
def test_two_aligns_and_a_solver_round_trip_give_the_same_bits(case):
    g = make_gicp("bfgs")
    g.setInputTarget(synth.as_pointxyzi(case.target))
    g.setInputSource(synth.as_pointxyzi(case.source))
    g.align(case.guess)
    Tb, rb = g.getFinalTransformation().copy(), dict(g.last_result)
    g.align(case.guess)
    assert np.array_equal(Tb, g.getFinalTransformation())
    assert (g.last_result["iterations"], g.last_result["n_evaluations"], g.last_result["score"]) == (rb["iterations"], rb["n_evaluations"], rb["score"])
    ref = make_gicp("gauss_newton")
    ref.setInputTarget(synth.as_pointxyzi(case.target))
    ref.setInputSource(synth.as_pointxyzi(case.source))
    ref.align(case.guess)
    Tg, rg = ref.getFinalTransformation().copy(), dict(ref.last_result)
    g.setOptimizer("gauss_newton")
    g.align(case.guess)
    assert np.array_equal(Tg, g.getFinalTransformation())
    assert (g.last_result["iterations"], g.last_result["n_evaluations"], g.last_result["score"]) == (rg["iterations"], rg["n_evaluations"], rg["score"])
    g.setOptimizer("bfgs")
    g.align(case.guess)
    assert np.array_equal(Tb, g.getFinalTransformation())
    assert (g.last_result["iterations"], g.last_result["n_evaluations"], g.last_result["score"]) == (rb["iterations"], rb["n_evaluations"], rb["score"])
    assert not np.array_equal(Tb, Tg)       # two schedules, two roundings of the same minimum


def test_mixed_batch_equals_the_single_aligns(case):
    """Six objects, three with their own target and three sharing the first one's, objects 1 and 4 left on Gauss-Newton: every member of
    the batch ends bit for bit where its own align() puts it."""
    from lidarslam_ros2_amd import align_batch

    rng = np.random.default_rng(9)
    regs, guesses, singles = [], [], []
    for b in range(6):
        g = make_gicp("gauss_newton" if b in (1, 4) else "bfgs")
        if b < 3:
            shift = np.float32([0.4 * b, -0.3 * b, 0.0])
            g.setInputTarget(case.target + shift)
            g.setInputSource(case.source[: 3900 - 150 * b] + shift)
            G = case.guess.copy(); G[:3, 3] += shift - G[:3, :3] @ shift
        else:
            g.shareTargetOf(regs[0])
            g._n_target = case.target.shape[0]
            g.setInputSource(case.source[: 3800 - 211 * b])
            G = case.guess.copy(); G[:3, 3] += rng.uniform(-0.1, 0.1, 3).astype(np.float32)
        regs.append(g); guesses.append(G)
    for g, G in zip(regs, guesses):
        g.align(G)
        singles.append((g.getFinalTransformation().copy(), dict(g.last_result)))
    finals, results = align_batch(regs, guesses)
    for b in range(6):
        assert np.array_equal(finals[b], singles[b][0]), b
        assert results[b]["iterations"] == singles[b][1]["iterations"] and results[b]["n_evaluations"] == singles[b][1]["n_evaluations"], b
        assert results[b]["converged"]
    assert min(results[b]["n_evaluations"] for b in (0, 2, 3, 5)) > 3 * max(results[b]["n_evaluations"] for b in (1, 4))


def test_too_few_correspondences_and_collinear_clouds(case):
    g = make_gicp("bfgs", corr=0.5)
    g.setInputTarget(case.target)
    g.setInputSource(case.source + np.float32(500.0))
    g.align()                                   # < 4 correspondences: loop left, not converged, pose = guess
    assert not g.hasConverged()
    assert np.allclose(g.getFinalTransformation(), np.eye(4))
    assert g.last_result["n_evaluations"] == 0
    tr = g.bfgs_trace()
    assert tr["m"] < 4 and tr["n_evals"] == 0
    # the collinear clouds of test_rank_deficient_system_returns_a_finite_pose: the call returns, with a finite pose
    t = np.linspace(-20.0, 20.0, 400, dtype=np.float32)
    line = np.stack([t, np.zeros_like(t), np.zeros_like(t)], axis=1)
    src = line[::2] + np.float32([0.05, 0.0, 0.0])
    g = make_gicp("bfgs")
    g.setInputTarget(line)
    g.setInputSource(src)
    g.align(np.eye(4, dtype=np.float32))
    T = g.getFinalTransformation()
    assert np.all(np.isfinite(T)), T
    assert np.abs(T[:3, 3]).max() < 5.0

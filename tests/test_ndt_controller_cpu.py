"""The cases of the NDT controller tests, held to the oracle on the CPU (no GPU needed): the restatement in ndt_controller_numpy.py
reproduces the oracle's logged poses bit for bit on every case, the case set takes every branch at least twice with every deciding
comparison away from a tie, a one-ulp perturbation of every division and square root changes no branch, and the bars next to the cases
are the measured ones.  test_ndt_controller_gpu.py replays the same cases on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ndt_controller_cases as K
import ndt_controller_numpy as N
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(K.all_cases())
# every branch the restatement names that finite or NaN operands can reach (ndt_controller_cases.py: what is unreachable)
REQUIRED = ["tv1_cubic", "tv1_average", "tv2_cubic", "tv2_secant", "tv3_degenerate", "tv4_nan", "tv1_average_nan", "trial_nan",
            "ui_upper", "ui_lower", "ui_swap", "ui_converged", "interval_closed", "cap_ten_trials", "exit_after_trials",
            "exit_first_evaluation", "reversed", "first_clamped_up", "first_clamped_down", "trial_clamped_up", "end_by_trans_eps",
            "end_by_max_iterations", "small_step_at_iteration_0", "zero_slope", "newton_zero_step", "newton_nan_step"]


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b, equal_nan=True))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_oracle(name):
    b = K.build(name, O)
    log, res, rp, rows = b["log"], b["result"], b["replay"], b["rows"]
    assert 1 <= len(rows) <= 40 and rows.shape[1] == 29
    assert rp.n_used == len(rows) and len(rp.trace) == len(rows)
    assert len(rp.poses) == len(log)
    for k, (mine, e) in enumerate(zip(rp.poses, log)):
        assert _same(mine, e["p"]), (name, k)                     # the pose of every evaluation, bit for bit
    assert rp.converged == int(res["converged"]) and rp.iterations == res["iterations"]
    assert np.array_equal(rp.p, res["p"], equal_nan=True)
    assert np.array_equal(np.float64(rp.trans_probability), np.float64(res["trans_probability"]), equal_nan=True)
    assert rp.n_evals == res["n_evals"] + res["n_evals_grad"] + res["n_hessian_recompute"]
    # the phase in which the device consumes row r is the one the trace row before it asked for
    asked = [N.PH_INIT] + [int(t[N.COL["phase"]]) for t in rp.trace[:-1]]
    assert asked == b["kinds"]
    assert rp.trace[-1][N.COL["done"]] == 1 and not rp.trace[:-1, N.COL["done"]].any()


@pytest.mark.parametrize("name", CASES)
def test_rows_poison_what_the_device_must_not_read(name):
    b = K.build(name, O)
    for row, kind in zip(b["rows"], b["kinds"]):
        if kind == N.PH_MT_TRIAL:
            assert np.all(np.isnan(row[8:29]))
        if kind == N.PH_MT_HESS:
            assert np.all(np.isnan(row[0:7])) and not np.isnan(row[7])
        if kind in (N.PH_INIT, N.PH_MT_FIRST, N.PH_MT_LAST, N.PH_MT_HESS) and "nan_hessian" not in name and "nan_in_hessian" not in name:
            assert not np.any(np.isnan(row[8:29]))
    if not any("nan" in t for t in b["replay"].branches):   # no NaN of the case's own making: any NaN would be a poisoned field read
        assert np.all(np.isfinite(b["replay"].trace)), "the restatement read a poisoned field"


def test_every_branch_is_taken_by_two_cases():
    count = {r: 0 for r in REQUIRED}
    seen = set()
    for name in CASES:
        br = K.build(name, O)["replay"].branches
        seen |= br
        for r in REQUIRED:
            count[r] += r in br
    assert all(v >= 2 for v in count.values()), {k: v for k, v in count.items() if v < 2}
    assert not ({"tv3_proper", "tv4_proper"} & seen)


@pytest.mark.parametrize("name", CASES)
def test_no_comparison_is_near_a_tie(name):
    worst = min(K.build(name, O)["replay"].margins, key=lambda m: m[1], default=("none", 1.0))
    assert worst[1] >= 1e-9, worst


@pytest.mark.parametrize("name", CASES)
def test_one_ulp_perturbation_changes_no_branch_and_gives_the_bar(name):
    b = K.build(name, O)
    bar, stable = N.measure_bar(b["rows"], b["replay"], b["p0"], b["step_size"], b["trans_eps"], b["max_iterations"], b["n_points"])
    assert stable or name in K.EXACT_TIE_CASES
    assert b["bar"] == pytest.approx(bar, rel=5e-3), (name, bar)
    assert b["bar"] >= 0.999 * N.ULP64 and b["bar"] < 1e-10


def test_reachability_of_case_3_and_4():
    """Random scripted profiles (the search that picked the cases ran 10 000 of them) reach neither the proper case 3 nor case 4 with
    finite operands; the degenerate case 3 they do reach."""
    seen = set()
    for seed in range(600):
        c = K.random_scripted_case(seed)
        log, _res = N.run_oracle(O, c["objective"], c["p_start"], c["step_size"], c["trans_eps"], c["max_iterations"], K.N_POINTS)
        rows, _kinds = N.rows_from_log(log)
        seen |= N.replay(rows, log[0]["p"], c["step_size"], c["trans_eps"], c["max_iterations"], K.N_POINTS).branches
    assert "tv3_degenerate" in seen and not ({"tv3_proper", "tv4_proper"} & seen)


def test_hand_made_cases_end_as_described():
    r = K.build("exact_zero_slope", O)
    assert r["result"]["converged"] and r["result"]["iterations"] == 2 and len(r["rows"]) == 1
    assert np.array_equal(r["result"]["p"], r["p0"]) and "zero_slope" in r["replay"].branches
    r = K.build("zero_gradient", O)
    assert r["result"]["converged"] and r["result"]["iterations"] == 0 and "newton_zero_step" in r["replay"].branches
    r = K.build("nan_in_hessian", O)
    assert not r["result"]["converged"] and "newton_nan_step" in r["replay"].branches
    r = K.build("small_step_at_iteration_0", O)
    first = r["replay"].trace[1]                      # after the first line search: a_t below trans_eps, not converged, iteration 1 begun
    assert r["result"]["iterations"] == 2 and first[N.COL["nr_iterations"]] == 1 and first[N.COL["done"]] == 0
    assert K.build("small_step_then_large", O)["result"]["iterations"] == 3
    r = K.build("nan_trial_value", O)
    assert "tv1_average_nan" in r["replay"].branches and np.all(np.isnan(r["result"]["p"]))
    assert np.all(np.isfinite(r["rows"][:, 0:7][~np.isnan(r["rows"][:, 0])]))          # from finite operands
    for name in ("nan_score_case_4", "nan_score_and_slope_case_4"):
        assert "tv4_nan" in K.build(name, O)["replay"].branches


def test_svd6_restatement_and_the_elimination_agree_with_longdouble():
    """The 6x6 systems of the GPU test on the CPU: float64 numpy.linalg.solve stays within a tenth of the bar 16 cond(H) 2^-53, and so
    does the device's elimination restated in float64; svd6_solve as restated here meets the same bar."""
    for name, kind, H, g in K.solve6_systems():
        ref = N.reference_solve6(H, g)
        with np.errstate(all="ignore"):
            gj = N.gauss_jordan6(H, g)
            if kind == "nan":
                assert ref is None and np.all(np.isnan(gj))
                continue
            scale = max(float(np.max(np.abs(ref))), 1e-300)
            bar = N.solve6_bar(H)
            if kind == "regular":
                assert float(np.max(np.abs(np.linalg.solve(H, -g) - ref))) / scale <= 0.1 * bar, name
            if kind in ("regular", "singular"):
                assert float(np.max(np.abs(gj - ref))) / scale <= 0.1 * bar, name
                assert float(np.max(np.abs(N.svd6_solve(H, -g) - ref))) / scale <= bar, name
            if kind == "residual":
                assert float(np.max(np.abs(H @ gj + g))) <= bar * float(np.max(np.abs(g))), name
            if kind == "bounded":
                # the rotated unobserved direction: the restated elimination drops unknown 5 and solves equations 0, 1, 2, 4, 5 -
                # pinned here, and held to a longdouble solve of exactly those five equations in the five kept unknowns
                x, dropped, order = N.gauss_jordan6(H, g, details=True)
                assert dropped == [5] and sorted(order[:5]) == [0, 1, 2, 4, 5] and x[5] == 0.0
                sub, rhs = H[np.ix_(order[:5], range(5))], g[order[:5]]
                x5 = np.asarray(N.longdouble_solve(sub, -rhs), np.float64)
                assert float(np.max(np.abs(x[:5] - x5))) / float(np.max(np.abs(x5))) <= 0.1 * 16.0 * np.linalg.cond(sub) * 2.0 ** -53
    a, b = K.mt_operands()
    assert a.shape == b.shape == (4096,)
    assert N.mt_div_takes_ieee_path(a, b).sum() > 500 and (~N.mt_div_takes_ieee_path(a, b)).sum() > 1500
    assert N.mt_sqrt_takes_ieee_path(a).sum() > 500 and (~N.mt_sqrt_takes_ieee_path(a)).sum() > 1500


def test_ulp_distance_counts_in_integers():
    """neighbours 1, 2 and 3 ulp away are 1, 2 and 3 apart at every magnitude (the ordered bit patterns of normal doubles are far
    above 2^53: a distance formed in float64 would round them away), across zero and the denormals, and against the infinities"""
    for v in (1.0, 1.5, 3.0, 1e10, 1e-5, -2.0, 1e290, 1e-290, 2.2250738585072014e-308, 5e-324, 0.0, -0.0, -1e300):
        up = down = np.float64(v)
        for k in (1, 2, 3):
            up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
            assert N.ulp_distance([v], [up])[0] == k and N.ulp_distance([up], [v])[0] == k, (v, k)
            assert N.ulp_distance([v], [down])[0] == k and N.ulp_distance([down], [v])[0] == k, (v, k)
    d = N.ulp_distance([-0.0, np.nan, np.nan, 1.0, -5e-324, np.inf, 1.0], [0.0, np.nan, 1.0, np.nan, 5e-324, 1.7976931348623157e308, 1.0 + 2.0 ** -44])
    assert d.tolist() == [0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 2, 1, 256]
    assert N.ulp_distance([-np.inf], [np.inf])[0] == 2 * 0x7FF0000000000000
    assert N.same_bits([0.0, np.nan, 1.0], [-0.0, np.nan, 1.0]).tolist() == [False, True, True]


def test_inspection_entries_are_declared_and_check_their_arguments():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    lib.lsr_last_error.restype = C.c_char_p
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name in ("lsr_debug_ndt_controller_replay", "lsr_debug_ndt_solve6", "lsr_debug_mt_math"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes and re.search(r"\bint " + name + r"\(", hdr)
    assert int(re.search(r"#define LSR_NDT_REPLAY_TRACE (\d+)", hdr).group(1)) == N.TRACE_WIDTH == _capi.NDT_REPLAY_TRACE
    assert int(re.search(r"#define LSR_NDT_REPLAY_MAX_ROWS (\d+)", hdr).group(1)) == _capi.NDT_REPLAY_MAX_ROWS == 512
    dp = C.POINTER(C.c_double)
    buf = np.zeros(512 * 47)
    d = buf.ctypes.data_as(dp)
    used = C.c_int(-1)
    # a null handle with every bad argument in turn: the argument checks come first and touch nothing; a live handle with the same bad
    # arguments is test_ndt_controller_gpu.py's
    for rows in (0, -1, 513):
        assert lib.lsr_debug_ndt_controller_replay(None, d, 0.1, 0.01, 35, 10, d, rows, d, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(None, d, 0.1, 0.01, 35, 10, d, 1, d, C.byref(used)) == -1
    assert b"null handle" in lib.lsr_last_error()
    assert lib.lsr_debug_ndt_controller_replay(None, d, 0.1, 0.01, 35, 0, d, 1, d, C.byref(used)) == -1
    assert b"null handle" not in lib.lsr_last_error()
    assert lib.lsr_debug_ndt_controller_replay(None, None, 0.1, 0.01, 35, 10, d, 1, d, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(None, d, 0.1, 0.01, 35, 10, None, 1, d, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(None, d, 0.1, 0.01, 35, 10, d, 1, None, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(None, d, 0.1, 0.01, 35, 10, d, 1, d, None) == -1
    assert used.value == -1
    assert lib.lsr_debug_ndt_solve6(None, d, d, 1, d) == -1
    assert lib.lsr_debug_ndt_solve6(None, None, d, 1, d) == -1 and lib.lsr_debug_ndt_solve6(None, d, None, 1, d) == -1
    assert lib.lsr_debug_ndt_solve6(None, d, d, 1, None) == -1 and lib.lsr_debug_ndt_solve6(None, d, d, 0, d) == -1
    assert lib.lsr_debug_ndt_solve6(None, d, d, _capi.DEBUG_MAX_COUNT + 1, d) == -1
    assert lib.lsr_debug_mt_math(None, d, d, 1, d, d) == -1
    assert lib.lsr_debug_mt_math(None, None, d, 1, d, d) == -1 and lib.lsr_debug_mt_math(None, d, None, 1, d, d) == -1
    assert lib.lsr_debug_mt_math(None, d, d, 1, None, d) == -1 and lib.lsr_debug_mt_math(None, d, d, 1, d, None) == -1
    assert lib.lsr_debug_mt_math(None, d, d, 0, d, d) == -1 and lib.lsr_debug_mt_math(None, d, d, _capi.DEBUG_MAX_COUNT + 1, d, d) == -1
    assert not buf.any()

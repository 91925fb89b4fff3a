"""The on-device NDT controller (csrc/ndt.hip: ndt_controller_mt, mt_trial_value, mt_update_interval, mt_div / mt_sqrt, solve6_wave,
ndt_newton_begin / ndt_newton_end, ndt_controller_wave0) against the oracle, apart from the derivative pass: the three inspection
entries run the device functions on one wave as the derivative kernels call them.

* replay: every case of ndt_controller_cases.py (the oracle's own loop on a synthetic objective, its evaluations turned into rows).
  Phases, flags, request flags and counters equal the restatement's, which test_ndt_controller_cpu.py holds to the oracle's logged
  poses bit for bit; a_t, the interval, phi_0, d_phi_0, dir, x_t, p and trans_probability within the case's measured bar; the result
  equals the oracle's.
* solve6: the one-wave elimination against a longdouble elimination / minimum-norm answer, bar 16 cond(H) 2^-53.
* mt_math: the fast division and square root within 1 ulp of the correctly rounded results, equal bits on the IEEE path."""
import ctypes as C

import numpy as np
import pytest

import ndt_controller_cases as K
import ndt_controller_numpy as N

pytestmark = pytest.mark.gpu
CASES = sorted(K.all_cases())
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def handle():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    h = C.c_void_p()
    _capi.check(lib.lsr_create(_capi.METHOD_NDT, 0, None, C.byref(h)), "lsr_create")
    yield lib, h
    lib.lsr_destroy(h)


def _replay(handle, b):
    from lidarslam_ros2_amd import _capi

    lib, h = handle
    rows = np.ascontiguousarray(b["rows"], np.float64)
    trace = np.full((len(rows), N.TRACE_WIDTH), -7.0)
    used = C.c_int(-1)
    p0 = np.ascontiguousarray(b["p0"], np.float64)
    _capi.check(lib.lsr_debug_ndt_controller_replay(h, p0.ctypes.data_as(DP), b["step_size"], b["trans_eps"], b["max_iterations"],
                                                    b["n_points"], rows.ctypes.data_as(DP), len(rows), trace.ctypes.data_as(DP),
                                                    C.byref(used)), "lsr_debug_ndt_controller_replay")
    return trace, used.value


@pytest.mark.parametrize("name", CASES)
def test_controller_replay_follows_the_oracle(handle, O, name):
    b = K.build(name, O)
    ref, res = b["replay"].trace, b["result"]
    got, used = _replay(handle, b)
    assert used == len(b["rows"]) == len(ref)
    for col in N.EXACT_COLS:      # phase, pass form, request flags, done, converged, counters, the interval's flags; score, g, pairs
        assert np.array_equal(got[:, col], ref[:, col], equal_nan=True), (name, N.TRACE_FIELDS[col], got[:, col], ref[:, col])
    dev = N.trace_deviation(got, ref, b["trans_eps"] / 2)
    print(f"{name}: {used} rows, deviation {dev:.3g}, bar {b['bar']:.3g}")
    assert dev <= b["bar"], (name, dev, b["bar"])
    if not any("nan" in t for t in b["replay"].branches):
        assert np.all(np.isfinite(got)), "the controller read a poisoned field"
    # the end of the align, against the oracle itself
    last = got[-1]
    assert last[N.COL["done"]] == 1 and last[N.COL["converged"]] == int(res["converged"])
    assert last[N.COL["nr_iterations"]] == res["iterations"]
    assert last[N.COL["n_evals"]] == res["n_evals"] + res["n_evals_grad"] + res["n_hessian_recompute"]
    p = last[N.COL["p0"]:N.COL["p0"] + 6]
    assert np.array_equal(np.isnan(p), np.isnan(res["p"]))
    if np.all(np.isfinite(res["p"])):
        assert np.max(np.abs(p - res["p"])) <= b["bar"] * max(np.max(np.abs(res["p"])), b["trans_eps"] / 2)
    tp = res["trans_probability"]
    assert (np.isnan(tp) and np.isnan(last[N.COL["trans_probability"]])) or abs(last[N.COL["trans_probability"]] - tp) <= b["bar"] * abs(tp)


def test_replay_stops_at_done_and_leaves_the_rest_untouched(handle, O):
    """rows past the end of the align are not consumed: n_used stays, their trace rows are zero"""
    b = dict(K.build("small_step_at_iteration_0", O))
    n = len(b["rows"])
    b["rows"] = np.concatenate([b["rows"], np.full((5, 29), np.nan)])
    got, used = _replay(handle, b)
    assert used == n and np.all(got[n:] == 0.0)
    assert np.array_equal(got[:n, :len(N.INT_FIELDS)], b["replay"].trace[:, :len(N.INT_FIELDS)])


def test_solve6_against_longdouble(handle):
    from lidarslam_ros2_amd import _capi

    lib, h = handle
    systems = K.solve6_systems()
    Hu = np.ascontiguousarray([N.upper21(H) for _n, _k, H, _g in systems], np.float64)
    g6 = np.ascontiguousarray([g for _n, _k, _H, g in systems], np.float64)
    out = np.full((len(systems), 6), -7.0)
    _capi.check(lib.lsr_debug_ndt_solve6(h, Hu.ctypes.data_as(DP), g6.ctypes.data_as(DP), len(systems), out.ctypes.data_as(DP)),
                "lsr_debug_ndt_solve6")
    for (name, kind, H, g), x in zip(systems, out):
        ref = N.reference_solve6(H, g)
        if kind == "nan":
            assert np.all(np.isnan(x)), (name, x)
            continue
        assert np.all(np.isfinite(x)), (name, x)
        bar = N.solve6_bar(H)
        scale = max(float(np.max(np.abs(ref))), 1e-300)
        err = float(np.max(np.abs(x - ref))) / scale
        print(f"{name}: error {err:.3g}, bar {bar:.3g}")
        if kind in ("regular", "singular"):
            assert err <= bar, (name, err, bar, x)
        elif kind == "residual":   # a consistent singular system: H delta = -g, the minimum-norm answer is not promised
            assert float(np.max(np.abs(H @ x + g))) <= bar * float(np.max(np.abs(g))), (name, x)
        else:
            # "bounded" (finding 2 with the unobserved direction coupled to the rest): the vanishing pivot's unknown is dropped and the
            # other five solve five of the six equations.  Which unknown and which equations: the float64 restatement of the
            # elimination, which test_ndt_controller_cpu.py pins and holds to a longdouble solve of those five equations.  The
            # minimum-norm answer is promised for decoupled systems only; the step is of the reference's size, not 1e16 times it.
            gj, dropped, order = N.gauss_jordan6(H, g, details=True)
            kept = [k for k in range(6) if k not in dropped]
            assert list(np.flatnonzero(x == 0.0)) == dropped, (name, x)
            bar5 = 16.0 * np.linalg.cond(H[np.ix_([order[k] for k in kept], kept)]) * 2.0 ** -53
            err5 = float(np.max(np.abs(x - gj))) / float(np.max(np.abs(gj)))
            print(f"{name}: against the restated elimination {err5:.3g}, bar {bar5:.3g}")
            assert err5 <= bar5, (name, x, gj)
            assert np.linalg.norm(x) <= 10.0 * np.linalg.norm(np.asarray(ref, np.float64)), (name, x)


def test_inspection_entries_check_their_arguments_with_a_real_handle(handle):
    """bad pointers and counts with a live object: LSR_ERR_INVALID_ARGUMENT, nothing launched (test_ndt_controller_cpu.py: null handle)"""
    lib, h = handle
    buf = np.zeros(64)
    d = buf.ctypes.data_as(DP)
    used = C.c_int(-1)
    for rows in (0, -1, 513):
        assert lib.lsr_debug_ndt_controller_replay(h, d, 0.1, 0.01, 35, 10, d, rows, d, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(h, d, 0.1, 0.01, 35, 0, d, 1, d, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(h, None, 0.1, 0.01, 35, 10, d, 1, d, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(h, d, 0.1, 0.01, 35, 10, None, 1, d, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(h, d, 0.1, 0.01, 35, 10, d, 1, None, C.byref(used)) == -1
    assert lib.lsr_debug_ndt_controller_replay(h, d, 0.1, 0.01, 35, 10, d, 1, d, None) == -1
    assert used.value == -1 and not buf.any()
    assert lib.lsr_debug_ndt_solve6(h, None, d, 1, d) == -1 and lib.lsr_debug_ndt_solve6(h, d, None, 1, d) == -1
    assert lib.lsr_debug_ndt_solve6(h, d, d, 1, None) == -1 and lib.lsr_debug_ndt_solve6(h, d, d, 0, d) == -1
    assert lib.lsr_debug_ndt_solve6(h, d, d, (1 << 20) + 1, d) == -1
    assert lib.lsr_debug_mt_math(h, None, d, 1, d, d) == -1 and lib.lsr_debug_mt_math(h, d, None, 1, d, d) == -1
    assert lib.lsr_debug_mt_math(h, d, d, 1, None, d) == -1 and lib.lsr_debug_mt_math(h, d, d, 1, d, None) == -1
    assert lib.lsr_debug_mt_math(h, d, d, 0, d, d) == -1 and lib.lsr_debug_mt_math(h, d, d, (1 << 20) + 1, d, d) == -1
    assert not buf.any()


def test_mt_div_and_sqrt_within_one_ulp(handle):
    from lidarslam_ros2_amd import _capi

    lib, h = handle
    a, b = K.mt_operands()
    quot, root = np.full(a.shape, -7.0), np.full(a.shape, -7.0)
    _capi.check(lib.lsr_debug_mt_math(h, a.ctypes.data_as(DP), b.ctypes.data_as(DP), len(a), quot.ctypes.data_as(DP),
                                      root.ctypes.data_as(DP)), "lsr_debug_mt_math")
    with np.errstate(all="ignore"):
        q_ref, r_ref = a / b, np.sqrt(a)
    dq, dr = N.ulp_distance(quot, q_ref), N.ulp_distance(root, r_ref)
    wq, wr = int(np.argmax(dq)), int(np.argmax(dr))
    print(f"division: worst {dq[wq]} ulp at {a[wq]!r} / {b[wq]!r}; square root: worst {dr[wr]} ulp at {a[wr]!r}")
    fast_q, fast_r = ~N.mt_div_takes_ieee_path(a, b), ~N.mt_sqrt_takes_ieee_path(a)
    print(f"fast path: division {np.bincount(np.minimum(dq[fast_q], 3).astype(np.int64), minlength=4)} results at 0, 1, 2, 3+ ulp; "
          f"square root {np.bincount(np.minimum(dr[fast_r], 3).astype(np.int64), minlength=4)}")
    assert dq[wq] <= 1, (a[wq], b[wq], quot[wq], q_ref[wq])
    assert dr[wr] <= 1, (a[wr], root[wr], r_ref[wr])
    ieee_q, ieee_r = N.mt_div_takes_ieee_path(a, b), N.mt_sqrt_takes_ieee_path(a)
    assert np.all(N.same_bits(quot, q_ref)[ieee_q]), "the guard sends these divisors to the IEEE division"
    assert np.all(N.same_bits(root, r_ref)[ieee_r]), "the guard sends these radicands to the IEEE square root"

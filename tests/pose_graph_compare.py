"""TEST INFRASTRUCTURE of tests/test_pose_graph_long_gpu.py: the device's pose-graph optimiser against the dense numpy restatement
tests/pose_graph_numpy.py over the oracle's decisive iterations, with the tolerances as parameters; the raw C call with sentinel-filled
outputs for either entry point; the graphs with many loop edges."""
import ctypes as C

import numpy as np

import pose_graph_cases as PC
import pose_graph_numpy as O
from lidarslam_ros2_amd import _capi, pose_graph
from lidarslam_ros2_amd.posemath import pose_delta

STOPS = {O.STOP_MAX_ITERATIONS: "max_iterations", O.STOP_TRIALS: "trials", O.STOP_RHO_ZERO: "rho_zero", O.STOP_LAMBDA: "lambda"}


def oracle(X, E, max_iterations=10):
    """-> (poses, trace, result, poses after every iteration)"""
    hist = []
    Y, trace, res = O.optimize(X, E, max_iterations, history=hist)
    return Y, trace, res, hist


def pose_diff(A, B):
    d = [pose_delta(a, b) for a, b in zip(A, B)]
    return max(v[0] for v in d), max(v[1] for v in d)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def decisive_iterations(trace, decisive, floor=0.0):
    """How many leading iterations of the oracle's trace a second fp64 implementation can be held to: accept or reject is the sign of
    cur - tmp, and two implementations whose chi2 agree within the tolerance take the same decision while the oracle's gains stay above
    `decisive` (ten times that tolerance) and chi2 above `floor`."""
    keep = 0
    for t in trace:
        if t["chi2"] <= floor or min(abs(g) for g in t["gains"]) < decisive:
            break
        keep += 1
    return keep


def loop_heavy_graph(N, L, seed=7):
    """N vertices two laps round a radius-15 circle, drift N(0, 0.03 m) / N(0, 0.002) composed per step, the odometry edges of the
    drifted poses (k = 5) and L distinct loop edges with |from - to| > 5 that miss vertex 0, in sorted order, measured from the truth:
    all L of them lie outside a band of 5.  -> (truth, start, edges)"""
    rng = np.random.default_rng(seed)
    GT = PC.circle(N, 15.0, N // 2, 0.03)
    X = PC.drifted(GT, 0.03, 0.002, rng)
    E = O.adjacent_edges(X, 5)
    pairs = set()
    while len(pairs) < L:
        a, b = sorted(int(v) for v in rng.integers(1, N, 2))
        if b - a > 5:
            pairs.add((a, b))
    return GT, X, E + [(a, b, O.inv(GT[a]) @ GT[b]) for a, b in sorted(pairs)]


def run_and_compare(name, reg, X, E, ora, tol_rel, tol_pose, band=5, max_iterations=10, floor=0.0):
    """The device against the oracle over the decisive iterations: the device runs exactly that many, and its trace entry by entry
    (trials equal, chi2 and lambda within tol_rel), its result record and its poses (tol_pose, metres and radians) are the oracle's at
    that iteration.  Prints every figure before it asserts.  Where the oracle's run goes on past its decisive iterations the device's
    full run is held to what does not depend on rounding: it does not end above the decisive prefix's chi2.
    -> (poses of the full run, its result, number of decisive iterations, dict of the measured differences)"""
    Y, trace, ores, hist = ora
    trace, hist = trace[:max_iterations], hist[:max_iterations]
    keep = decisive_iterations(trace, 10 * tol_rel, floor)
    assert keep >= 1
    dev, res = pose_graph.optimize(reg, X, E, max_iterations=keep, band=band)
    dt, dr = pose_diff(dev, hist[keep - 1])
    rc = max(rel(t["chi2"], o["chi2"]) for t, o in zip(res.trace, trace))
    rl = max(rel(t["lam"], o["lam"]) for t, o in zip(res.trace, trace))
    trials = [t["trials"] for t in res.trace]
    measured = dict(chi2_rel=rc, lambda_rel=rl, pose_m=dt, pose_rad=dr)
    print(f"{name}: {keep} of {len(trace)} iterations decisive, trials {trials} chi2 {res.chi2_before:.6g} -> {res.chi2_after:.6g} | vs oracle: "
          f"chi2 rel {rc:.3g} lambda rel {rl:.3g} poses {dt:.3g} m {dr:.3g} rad | device_ms {res.device_ms:.3f}")
    assert trials == [o["trials"] for o in trace[:keep]] and res.iterations == keep and res.trials == sum(trials)
    assert rc <= tol_rel and rl <= tol_rel
    assert rel(res.chi2_before, ores["chi2_before"]) <= tol_rel
    assert res.chi2_after == res.trace[-1]["chi2"] and res.lam == res.trace[-1]["lam"]
    assert dt <= tol_pose and dr <= tol_pose
    assert res.device_ms > 0
    if keep == len(trace) == ores["iterations"]:
        assert res.stop_reason == STOPS[ores["stop"]]
        return dev, res, keep, measured
    full, fres = pose_graph.optimize(reg, X, E, max_iterations=max_iterations, band=band)
    print(f"{name}: full run trials {[t['trials'] for t in fres.trace]} chi2 -> {fres.chi2_after:.6g}")
    assert np.isfinite(full).all() and fres.chi2_after <= res.chi2_after * (1 + tol_rel)
    assert [t["trials"] for t in fres.trace[:keep]] == trials
    return full, fres, keep, measured


def edge_array(edges):
    """(from, to[, Z]) -> lsr_pose_edge array; a missing measurement is the identity"""
    arr = (_capi.PoseEdge * max(len(edges), 1))()
    eye = np.eye(4).reshape(16).tolist()
    for i, e in enumerate(edges):
        arr[i].from_, arr[i].to = int(e[0]), int(e[1])
        arr[i].measurement[:] = eye if len(e) < 3 else np.asarray(e[2], np.float64).reshape(4, 4).T.reshape(16).tolist()
    return arr


def raw_call(entry, reg, P, edges, params=(10, 5)):
    """`entry` (lsr_optimize_pose_graph or lsr_optimize_pose_graph_long) on col-major poses P (n, 16) with sentinel-filled outputs
    -> (status, outputs untouched?, poses out, result record, trace array)"""
    fn = getattr(_capi.load(), entry)
    P = np.ascontiguousarray(P, np.float64)
    arr = edge_array(edges)
    out = np.full((max(len(P), 1), 16), -7.0)
    res = _capi.PoseGraphResult(-7, -7, -7.0, -7.0, -7.0, -7, -7, -7.0)
    tr = (_capi.PoseGraphTrace * max(params[0], 1))()
    for t in tr:
        t.trials, t.chi2 = -7, -7.0
    dp = C.POINTER(C.c_double)
    st = fn(reg._h, P.ctypes.data_as(dp), len(P), arr, len(edges), C.byref(_capi.PoseGraphParams(*params)), out.ctypes.data_as(dp),
            C.byref(res), tr)
    untouched = bool((out == -7.0).all()) and res.iterations == -7 and res.device_ms == -7.0 and all(t.trials == -7 and t.chi2 == -7.0 for t in tr)
    return st, untouched, out, res, tr

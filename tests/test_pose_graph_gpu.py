"""'Next' row N6: the optimiser half of GraphBasedSlamComponent::doPoseAdjustment (graph_based_slam_component.cpp:267-319)
on the device through `lsr_optimize_pose_graph`, against the dense numpy restatement tests/pose_graph_numpy.py: traces entry by entry,
poses, the band / Woodbury split at its limits, refusals, and the chain search_loop -> pose_adjustment -> modified_map.

Tolerance (DESIGN.md 4 "Pose-graph optimisation"): both sides are fp64 and cond(H + lambda I) <~ 1e6, so differences near 1e-10 or
below are expected.  Measured on an MI355X, the largest over every graph of this file: chi2 1.88e-11 relative, lambda 3.31e-12 relative,
poses 1.12e-12 m / 9.9e-14 rad.  The tolerance is 100 x the measured value, below the 1e-8 the specification allows at most:
TOL_REL = 2e-9 for chi2 and lambda (relative), TOL_POSE = 1.2e-10 for poses (metres and radians)."""
import ctypes as C

import numpy as np
import pytest

import map_numpy
import pose_graph_cases as PC
import pose_graph_numpy as O
from lidarslam_ros2_amd import LoopClosureParams, MapArray, NormalDistributionsTransform, SubMap, _capi, pose_graph, search_loop, synth
from lidarslam_ros2_amd.posemath import pose_delta

pytestmark = pytest.mark.gpu

TOL_REL = 2e-9       # chi2, lambda: 100 x the largest measured difference (1.88e-11)
TOL_POSE = 1.2e-10   # metres and radians: 100 x the largest measured difference (1.12e-12 m; 9.9e-14 rad)
DECISIVE = 10 * TOL_REL
STOPS = {O.STOP_MAX_ITERATIONS: "max_iterations", O.STOP_TRIALS: "trials", O.STOP_RHO_ZERO: "rho_zero", O.STOP_LAMBDA: "lambda"}


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(0)


@pytest.fixture(scope="module")
def reference():
    """the 200-vertex graph and the oracle's run on it, computed once: (start, edges, (oracle poses, trace, result, poses per iteration))"""
    _, X, E = PC.reference_graph()
    return X, E, _oracle(X, E)


def _oracle(X, E, max_iterations=10):
    hist = []
    Y, trace, res = O.optimize(X, E, max_iterations, history=hist)
    return Y, trace, res, hist


def _pose_diff(A, B):
    d = [pose_delta(a, b) for a, b in zip(A, B)]
    return max(v[0] for v in d), max(v[1] for v in d)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _decisive_iterations(trace, floor=0.0):
    """How many leading iterations of the oracle's trace a second fp64 implementation can be held to.  Accept or reject is the sign of
    cur - tmp; two implementations whose chi2 agree within TOL_REL take the same decision when |cur - tmp| / cur exceeds 2 TOL_REL
    (DECISIVE is 10 TOL_REL).  Past that — a run that has converged and still iterates — the decisions are rounding on both sides, and
    so is everything that follows from them.  `floor`: chi2 itself loses its relative accuracy near zero: an error component carries
    an absolute rounding of ~1e-15 (eps x coordinates of a few metres), so chi2 = sum e^2 over E edges keeps 2e-15 sqrt(E / chi2)
    relative — worse than TOL_REL below chi2 ~ 1e-10; only the graph whose minimum is exactly zero gets there."""
    keep = 0
    for t in trace:
        if t["chi2"] <= floor or min(abs(g) for g in t["gains"]) < DECISIVE:
            break
        keep += 1
    return keep


def _run_and_compare(name, reg, X, E, oracle=None, band=5, max_iterations=10, floor=0.0):
    """The device against the oracle over the decisive iterations (all of them on most graphs): the device runs exactly that many,
    and its trace entry by entry (trials equal, chi2 and lambda within TOL_REL), its result record and its poses (TOL_POSE) are the
    oracle's at that iteration.  Prints every figure before it asserts.  Where the oracle's run goes on past its decisive iterations the
    device's full run is held to what does not depend on rounding: it does not end above the decisive prefix's chi2.
    -> (poses of the full run, its result, number of decisive iterations)"""
    Y, trace, ores, hist = oracle if oracle is not None else _oracle(X, E, max_iterations)
    trace, hist = trace[:max_iterations], hist[:max_iterations]
    keep = _decisive_iterations(trace, floor)
    assert keep >= 1
    dev, res = pose_graph.optimize(reg, X, E, max_iterations=keep, band=band)
    dt, dr = _pose_diff(dev, hist[keep - 1])
    rc = max(_rel(t["chi2"], o["chi2"]) for t, o in zip(res.trace, trace))
    rl = max(_rel(t["lam"], o["lam"]) for t, o in zip(res.trace, trace))
    trials = [t["trials"] for t in res.trace]
    print(f"{name}: {keep} of {len(trace)} iterations decisive, trials {trials} chi2 {res.chi2_before:.6g} -> {res.chi2_after:.6g} | vs oracle: "
          f"chi2 rel {rc:.3g} lambda rel {rl:.3g} poses {dt:.3g} m {dr:.3g} rad | device_ms {res.device_ms:.3f}")
    assert trials == [o["trials"] for o in trace[:keep]] and res.iterations == keep and res.trials == sum(trials)
    assert rc <= TOL_REL and rl <= TOL_REL
    assert _rel(res.chi2_before, ores["chi2_before"]) <= TOL_REL
    assert res.chi2_after == res.trace[-1]["chi2"] and res.lam == res.trace[-1]["lam"]
    assert dt <= TOL_POSE and dr <= TOL_POSE
    assert res.device_ms > 0
    if keep == len(trace) == ores["iterations"]:
        assert res.stop_reason == STOPS[ores["stop"]]
        return dev, res, keep
    full, fres = pose_graph.optimize(reg, X, E, max_iterations=max_iterations, band=band)
    print(f"{name}: full run trials {[t['trials'] for t in fres.trace]} chi2 -> {fres.chi2_after:.6g}")
    assert np.isfinite(full).all() and fres.chi2_after <= res.chi2_after * (1 + TOL_REL)
    assert [t["trials"] for t in fres.trace[:keep]] == trials
    return full, fres, keep


def test_known_answer_device_returns_the_truth(reg):
    """12 vertices, consistent edges, perturbed start: the device reaches the true poses within 1e-9 (the oracle reaches 4e-15,
    tests/test_pose_graph_cpu.py).  The minimum is exactly zero and chi2 ends at rounding level (1e-29), so the trace is compared while
    chi2 > 1e-9 (_decisive_iterations); the full run's poses are compared with the truth."""
    GT, X, E = PC.known_answer_graph()
    dev, res, keep = _run_and_compare("known answer", reg, X, E, floor=1e-9)
    dt, dr = _pose_diff(dev, GT)
    print(f"known answer: |device - truth| {dt:.3g} m {dr:.3g} rad, chi2 {res.chi2_before:.6g} -> {res.chi2_after:.3g}")
    assert dt <= 1e-9 and dr <= 1e-9 and res.iterations >= 5
    assert np.array_equal(dev[0], GT[0])                       # the fixed vertex is returned as it came


def test_reference_shaped_graph_matches_the_oracle_trace(reg, reference):
    """200 vertices, k = 5, 976 edges (four workgroups of edges, 1194 band columns), loop edges (0,100), (3,104) twice, (50,151),
    (97,199), (195,199): an edge into the fixed vertex, a duplicate pair, a loop edge inside the band, four slots of U.  chi2 ends at
    6e-3 and every trial changes it by more than 1e-4 of itself: no accept / reject decision is marginal, all ten iterations count."""
    X, E, ora = reference
    assert len(E) == 976 and min(abs(g) for t in ora[1] for g in t["gains"]) > 1e-4 and ora[2]["chi2_after"] > 1e-3
    dev, res, keep = _run_and_compare("reference graph", reg, X, E, ora)
    assert keep == 10 and res.iterations == 10 and res.stop_reason == "max_iterations"
    assert np.array_equal(dev[0], X[0])
    assert res.chi2_after < 0.05 * res.chi2_before


def test_one_iteration_pins_one_linearise_solve_update(reg, reference):
    X, E, ora = reference
    dev, res, keep = _run_and_compare("reference graph, one iteration", reg, X, E, ora, max_iterations=1)
    assert keep == 1 and res.iterations == 1 and res.stop_reason == "max_iterations"
    moved = max(pose_delta(a, b)[0] for a, b in zip(dev, X))
    assert moved > 0.05                                        # the step is far above the tolerance it is compared within


def test_two_runs_are_bit_identical(reg, reference):
    X, E = reference[0], reference[1]
    a, ra = pose_graph.optimize(reg, X, E)
    b, rb = pose_graph.optimize(reg, X, E)
    assert np.array_equal(a, b) and ra.trace == rb.trace
    assert (ra.chi2_before, ra.chi2_after, ra.lam, ra.trials) == (rb.chi2_before, rb.chi2_after, rb.lam, rb.trials)


def test_vertices_up_to_k_have_no_odometry_edge(reg):
    """The reference adds odometry edges for i > k only (:289), so vertices 1 .. k hang on lambda and on whatever loop edge touches
    them: with one loop edge 1 -> 39 vertex 1 is dragged by more than a metre.  The oracle's moves it too, and the device agrees."""
    _, X, E = PC.quirk_graph()
    ora = _oracle(X, E)
    assert np.linalg.norm(ora[0][1][:3, 3] - X[1][:3, 3]) > 0.1
    dev, res, _ = _run_and_compare("i > k quirk", reg, X, E, ora)
    moved = float(np.linalg.norm(dev[1][:3, 3] - X[1][:3, 3]))
    print("vertex 1 moved by", moved, "m")
    assert moved > 0.1


def test_rejected_steps_follow_the_oracle(reg):
    """16 vertices with a start error of N(0, 5 m) / N(0, 0.45): the oracle's own trace has an iteration with more than one trial while
    chi2 is far above rounding, inside its decisive iterations; the device takes the same trials."""
    _, X, E = PC.rejected_step_graph()
    ora = _oracle(X, E)
    trace = ora[1]
    keep = _decisive_iterations(trace)
    assert any(t["trials"] > 1 and t["chi2"] > 1e-6 for t in trace[:keep]), [t["trials"] for t in trace]
    dev, res, _ = _run_and_compare("rejected step", reg, X, E, ora)
    assert res.trials > res.iterations


def test_low_rank_part_at_its_limit_and_widest_band(reg):
    """(a) 20 vertices, k = 5, solved with band = 1: every edge with |from - to| > 1 that does not touch vertex 0 goes through the
    Woodbury correction — with the extra loop edges exactly LSR_POSE_GRAPH_MAX_OFFBAND_EDGES of them, a 384 x 384 dense system — and
    the answer is the oracle's, as with band = 5.  (b) 60 vertices, k = 8, band = 8: the widest band (half-width 53)."""
    rng = np.random.default_rng(5)
    GT = PC.circle(20, 8.0, 20, 0.05)
    X = PC.drifted(GT, 0.03, 0.002, rng)
    E = O.adjacent_edges(X, 5) + [(a, b, O.inv(GT[a]) @ GT[b]) for a, b in ((0, 12), (2, 17), (19, 4), (3, 18), (5, 16), (1, 19), (6, 11), (7, 15), (9, 2))]
    off = [e for e in E if e[0] != 0 and e[1] != 0 and abs(e[0] - e[1]) > 1]
    assert len(off) == _capi.POSE_GRAPH_MAX_OFFBAND_EDGES
    ora = _oracle(X, E)
    _run_and_compare("64 off-band edges, band 1", reg, X, E, ora, band=1)
    _run_and_compare("same graph, band 5", reg, X, E, ora, band=5)
    GT = PC.circle(60, 20.0, 30, 0.02)
    X = PC.drifted(GT, 0.03, 0.002, rng)
    E = O.adjacent_edges(X, 8) + [(a, b, O.inv(GT[a]) @ GT[b]) for a, b in ((0, 30), (2, 33), (25, 56), (40, 9))]
    _run_and_compare("k = 8, band 8", reg, X, E, band=8)


def test_largest_documented_size_runs(reg):
    """4096 vertices, k = 8, band 8, 64 loop edges, two iterations: the sizes the header promises, where an index past a buffer would
    show.  No oracle at this size (its matrix is dense); the run has to lower chi2 and return finite, orthonormal poses."""
    rng = np.random.default_rng(6)
    n = 4096
    GT = PC.circle(n, 300.0, 2048, 0.002)
    X = np.stack(PC.drifted(GT, 0.01, 0.0005, rng))
    E = pose_graph.adjacent_edges(X, 8)
    E += [(a, a + 2048 - 7, O.inv(GT[a]) @ GT[a + 2048 - 7]) for a in range(10, 10 + 32 * 64, 32)]
    assert len(E) == (n - 9) * 8 + 64
    dev, res = pose_graph.optimize(reg, X, E, max_iterations=2, band=8)
    print(f"4096 vertices: chi2 {res.chi2_before:.6g} -> {res.chi2_after:.6g}, trials {res.trials}, device_ms {res.device_ms:.1f}")
    assert np.isfinite(dev).all() and res.iterations == 2
    assert res.chi2_after < 0.5 * res.chi2_before
    R = dev[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12


def _raw_call(reg, P, edges, n=None, n_edges=None, params=(10, 5), null=()):
    """lsr_optimize_pose_graph with sentinel-filled outputs -> (status, outputs untouched?)"""
    lib = _capi.load()
    P = np.ascontiguousarray(P, np.float64)
    n = len(P) if n is None else n
    arr = (_capi.PoseEdge * max(len(edges), 1))()
    for i, (a, b) in enumerate(edges):
        arr[i].from_, arr[i].to = a, b
        arr[i].measurement[:] = np.eye(4).reshape(16).tolist()
    out = np.full((max(len(P), 1), 16), -7.0)
    res = _capi.PoseGraphResult(-7, -7, -7.0, -7.0, -7.0, -7, -7, -7.0)
    tr = (_capi.PoseGraphTrace * 10)()
    for t in tr:
        t.trials, t.chi2 = -7, -7.0
    dp = C.POINTER(C.c_double)
    st = lib.lsr_optimize_pose_graph(reg._h, None if "poses" in null else P.ctypes.data_as(dp), n, None if "edges" in null else arr,
                                     len(edges) if n_edges is None else n_edges, C.byref(_capi.PoseGraphParams(*params)),
                                     None if "out" in null else out.ctypes.data_as(dp), None if "result" in null else C.byref(res), tr)
    untouched = bool((out == -7.0).all()) and res.iterations == -7 and res.device_ms == -7.0 and all(t.trials == -7 and t.chi2 == -7.0 for t in tr)
    return st, untouched, out, res


def test_limits_and_bad_edges_are_refused_with_outputs_untouched(reg):
    I = np.tile(np.eye(4).T.reshape(16), (30, 1))
    I[:, 12] = np.arange(30)
    chain = [(i, i + 1) for i in range(29)]
    bad = [
        dict(edges=chain, null=("poses",)), dict(edges=chain, null=("edges",)), dict(edges=chain, null=("out",)),
        dict(edges=chain, null=("result",)), dict(edges=chain, n=0), dict(edges=chain, n_edges=-1),
        dict(edges=chain + [(4, 4)]), dict(edges=chain + [(-1, 3)]), dict(edges=chain + [(3, 30)]),
        dict(edges=chain, params=(0, 5)), dict(edges=chain, params=(10, 0)), dict(edges=chain, params=(10, _capi.POSE_GRAPH_MAX_BAND + 1)),
        dict(edges=chain + [(1, 20)] * (_capi.POSE_GRAPH_MAX_OFFBAND_EDGES + 1)),
    ]
    for kw in bad:
        st, untouched, _, _ = _raw_call(reg, I, **kw)
        assert st == -1 and untouched, kw
    big = np.tile(np.eye(4).reshape(16), (_capi.POSE_GRAPH_MAX_VERTICES + 1, 1))
    st, untouched, _, _ = _raw_call(reg, big, [(0, 1)])
    assert st == -1 and untouched
    assert b"pose graph" in _capi.load().lsr_last_error()
    # exactly the limit of off-band edges is served
    st, untouched, out, res = _raw_call(reg, I, chain + [(1, 20)] * _capi.POSE_GRAPH_MAX_OFFBAND_EDGES)
    assert st == 0 and not untouched and res.iterations >= 1
    # one vertex, or no edge: the input poses, zero iterations
    st, _, out, res = _raw_call(reg, I[:1], [])
    assert st == 0 and np.array_equal(out[0], I[0]) and res.iterations == 0 and res.trials == 0
    st, _, out, res = _raw_call(reg, I, [])
    assert st == 0 and np.array_equal(out, I) and res.iterations == 0


def test_chain_search_loop_pose_adjustment_modified_map(reg):
    """search_loop -> MapArray.pose_adjustment -> MapArray.modified_map through one object (`ndt`; `reg` only re-runs the graph): the
    accepted edge of a small synthetic drive closes the loop; the poses agree with the oracle on the same stored poses and edge, and the map equals tests/map_numpy.py moved by
    the device's own poses, bit for bit."""
    from lidarslam_ros2_amd import DIRECT7

    route = synth.make_loop_route()
    ma = MapArray()
    ma.submaps = [SubMap(synth.as_pointxyzi(sm["cloud"]), sm["position"], sm["orientation"], sm["distance"]) for sm in route]
    ndt = NormalDistributionsTransform(0)   # graph_based_slam_component.cpp:64-72
    ndt.setMaximumIterations(100)
    ndt.setResolution(5.0)
    ndt.setTransformationEpsilon(0.01)
    ndt.setNeighborhoodSearchMethod(DIRECT7)
    found = search_loop(ndt, ma.submaps, LoopClosureParams(threshold_loop_closure_score=1.0, distance_loop_closure=20.0,
                                                          range_of_searching_loop_closure=10.0, search_submap_num=2, voxel_leaf_size=0.2))
    accepted = [e for e in found if e.accepted]
    assert len(accepted) == 1 and accepted[0].pair_id[1] == len(route) - 1
    stored = list(ma.stored_poses())
    E = O.adjacent_edges(stored, 5) + [(accepted[0].pair_id[0], accepted[0].pair_id[1], accepted[0].relative_pose)]
    ora = _oracle(stored, E)
    # a 21-vertex graph converges in a few iterations and the oracle's later accept / reject decisions are rounding: the chain runs the
    # decisive ones, and the ten-iteration default is held to ending no higher (_run_and_compare)
    full, fres, keep = _run_and_compare("chain graph", reg, stored, E, ora)
    results = []
    poses = ma.pose_adjustment(ndt, accepted, max_iterations=keep, result=results)
    res = results[0]
    dt, dr = _pose_diff(poses, ora[3][keep - 1])
    print(f"chain: {keep} iterations, poses vs oracle {dt:.3g} m {dr:.3g} rad, chi2 {res.chi2_before:.6g} -> {res.chi2_after:.6g}")
    assert res.iterations == keep and dt <= TOL_POSE and dr <= TOL_POSE
    assert _rel(res.chi2_after, ora[1][keep - 1]["chi2"]) <= TOL_REL and res.chi2_after < res.chi2_before
    default = ma.pose_adjustment(ndt, accepted)                         # the default: ten iterations
    assert np.isfinite(default).all() and np.array_equal(default, ma.pose_adjustment(ndt, accepted))
    assert max(pose_delta(a, b)[0] for a, b in zip(default, full)) < 1e-6   # its own odometry edges (C helper) against numpy's: rounding
    # the loop edge pulls: its residual shrinks — to what the oracle leaves of it, not to zero: one edge of identity information against
    # five odometry edges per vertex spreads the correction over the graph
    a, b = accepted[0].pair_id
    Yk = ora[3][keep - 1]
    before = pose_delta(np.linalg.inv(stored[a]) @ stored[b], accepted[0].relative_pose)[0]
    after = pose_delta(np.linalg.inv(poses[a]) @ poses[b], accepted[0].relative_pose)[0]
    want = pose_delta(np.linalg.inv(Yk[a]) @ Yk[b], accepted[0].relative_pose)[0]
    print("loop residual", before, "->", after, "m; oracle", want)
    assert after < before and abs(after - want) <= 2 * TOL_POSE
    rec, first = ma.modified_map(ndt, poses)
    want, want_first = map_numpy.assemble_map(ma.submaps, poses)
    assert np.array_equal(first, want_first) and np.array_equal(np.asarray(rec), want)

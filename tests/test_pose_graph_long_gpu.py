"""Pose-graph optimisation past 64 edges outside the band (`lsr_optimize_pose_graph_long`, csrc/pose_graph_dense.hip): a drive of
ordinary length keeps every accepted loop edge (graph_based_slam_component.cpp:247, :308-315), so the dense part of the Woodbury split
is a blocked Cholesky over many workgroups.  Against the dense numpy restatement tests/pose_graph_numpy.py on three graphs whose
6L = 390, 576 and 1200 leave a remainder of 6, none and 48 over the 64-wide tile; bit-identical runs; the bits of the old entry within
its limit; limits and refusals; the documented size; MapArray.pose_adjustment with 70 accepted loop edges.

Tolerance (DESIGN.md 4 "Pose-graph optimisation"): 100 x the largest difference measured on an MI355X over the three oracle graphs, the
project's convention.  Measured (8, 10 and 5 decisive iterations): chi2 2.11e-13 relative, lambda 4.09e-12 relative, poses 1.98e-14 m /
1.44e-15 rad — below what the old path measures on its graphs (tests/test_pose_graph_gpu.py), and five orders below the parity bar of
1e-3 m / 1e-4 rad.  TOL_REL = 4.1e-10 for chi2 and lambda (relative), TOL_POSE = 2.0e-12 for poses (metres and radians)."""
import numpy as np
import pytest

import pose_graph_cases as PC
import pose_graph_compare as PCMP
import pose_graph_numpy as O
from lidarslam_ros2_amd import MapArray, NormalDistributionsTransform, _capi, pose_graph
from lidarslam_ros2_amd.loop_closure import LoopEdge

pytestmark = pytest.mark.gpu

TOL_REL = 4.1e-10    # chi2, lambda (relative): 100 x the largest measured difference (lambda, 4.09e-12)
TOL_POSE = 2.0e-12   # metres and radians: 100 x the largest measured difference (1.98e-14 m; 1.44e-15 rad)
LONG = "lsr_optimize_pose_graph_long"
CASES = {"60-65": (60, 65), "120-96": (120, 96), "160-200": (160, 200)}   # vertices, loop edges: 6L mod 64 = 6, 0, 48


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(0)


@pytest.fixture(scope="module")
def graphs():
    """the three graphs and the oracle's run on each, computed once: name -> (start, edges, oracle)"""
    out = {}
    for name, (N, L) in CASES.items():
        _, X, E = PCMP.loop_heavy_graph(N, L)
        out[name] = (X, E, PCMP.oracle(X, E))
    return out


def _off_band(E, band=5):
    return sum(1 for e in E if e[0] != 0 and e[1] != 0 and abs(e[0] - e[1]) > band)


@pytest.mark.parametrize("name", list(CASES))
def test_trace_and_poses_match_the_oracle(reg, graphs, name):
    """Band 5, every loop edge outside it.  The oracle's decisive iterations (8, 10 and 5 of ten at 10 x TOL_REL) have one trial each
    and chi2 goes 0.56 -> 0.49, 0.97 -> 0.57, 1.87 -> 1.25; the device's trace, result record and poses are the oracle's there."""
    X, E, ora = graphs[name]
    N, L = CASES[name]
    assert _off_band(E) == L > _capi.POSE_GRAPH_MAX_OFFBAND_EDGES and len(X) == N
    dev, res, keep, measured = PCMP.run_and_compare(name, reg, X, E, ora, TOL_REL, TOL_POSE)
    print(name, "measured", measured)
    assert keep >= 5 and all(t["trials"] == 1 for t in ora[1][:keep])
    assert np.array_equal(dev[0], X[0])
    assert res.chi2_after < res.chi2_before


def test_two_runs_are_bit_identical(reg, graphs):
    X, E, _ = graphs["160-200"]
    a, ra = pose_graph.optimize(reg, X, E)
    b, rb = pose_graph.optimize(reg, X, E)
    assert np.array_equal(a, b) and ra.trace == rb.trace
    assert (ra.chi2_before, ra.chi2_after, ra.lam, ra.trials, ra.iterations) == (rb.chi2_before, rb.chi2_after, rb.lam, rb.trials, rb.iterations)


def test_same_bits_as_the_old_entry_within_its_limit(reg):
    """PC.reference_graph() (four edges outside the band) through both entries: the long one runs the old path."""
    _, X, E = PC.reference_graph()
    P = np.ascontiguousarray(np.asarray(X).transpose(0, 2, 1).reshape(len(X), 16))
    got = {}
    for entry in ("lsr_optimize_pose_graph", LONG):
        st, untouched, out, res, tr = PCMP.raw_call(entry, reg, P, E)
        assert st == 0 and not untouched and res.iterations == 10
        got[entry] = (out, [(t.trials, t.chi2, t.lam, t.rho) for t in tr[:res.iterations]],
                      (res.iterations, res.trials, res.chi2_before, res.chi2_after, res.lam, res.stop_reason))
    old, new = got["lsr_optimize_pose_graph"], got[LONG]
    assert np.array_equal(old[0], new[0]) and old[1] == new[1] and old[2] == new[2]
    dev, pres = pose_graph.optimize(reg, X, E)                          # the package calls the long entry
    assert np.array_equal(dev.transpose(0, 2, 1).reshape(len(X), 16), old[0]) and pres.chi2_after == old[2][3]


def test_limits_and_refusals(reg):
    lib = _capi.load()
    I = np.tile(np.eye(4).T.reshape(16), (30, 1))
    I[:, 12] = np.arange(30)
    chain = [(i, i + 1) for i in range(29)]
    assert _capi.POSE_GRAPH_MAX_OFFBAND_EDGES == 64 and _capi.POSE_GRAPH_LONG_MAX_OFFBAND_EDGES == 1024
    st, untouched, out, res, _ = PCMP.raw_call(LONG, reg, I, chain + [(1, 20)] * 65)
    assert st == 0 and not untouched and res.iterations >= 1 and np.isfinite(out).all()
    st, untouched, _, _, _ = PCMP.raw_call("lsr_optimize_pose_graph", reg, I, chain + [(1, 20)] * 65)
    assert st == -1 and untouched and b"LSR_POSE_GRAPH_MAX_OFFBAND_EDGES" in lib.lsr_last_error()
    st, untouched, _, _, _ = PCMP.raw_call(LONG, reg, I, chain + [(1, 20)] * 1025)
    assert st == -1 and untouched
    assert b"pose graph" in lib.lsr_last_error() and b"LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES" in lib.lsr_last_error()
    # exactly the limit is served: 1024 duplicate rows of U, C = I + U B^-1 U^T stays positive definite because of the I
    st, untouched, out, res, _ = PCMP.raw_call(LONG, reg, I, chain + [(1, 20)] * 1024)
    assert st == 0 and not untouched and res.iterations >= 1 and np.isfinite(out).all()
    assert res.chi2_after <= res.chi2_before


def test_documented_size_runs(reg):
    """2048 vertices, k = 5, band 5, 1024 loop edges one lap apart, two iterations: W is 12282 x 6145 doubles (0.6 GB), C 6144 x 6144,
    96 block columns.  No oracle at this size; the run has to halve chi2 and return finite, orthonormal poses."""
    rng = np.random.default_rng(6)
    n, L = 2048, 1024
    GT = PC.circle(n, 300.0, 1024, 0.002)
    X = np.stack(PC.drifted(GT, 0.01, 0.0005, rng))
    E = pose_graph.adjacent_edges(X, 5)
    E += [(a, a + 1024 - 7, O.inv(GT[a]) @ GT[a + 1024 - 7]) for a in range(1, 1 + L)]
    assert len(E) == (n - 6) * 5 + L and _off_band(E) == L == _capi.POSE_GRAPH_LONG_MAX_OFFBAND_EDGES
    dev, res = pose_graph.optimize(reg, X, E, max_iterations=2, band=5)
    print(f"2048 vertices, 1024 loop edges: chi2 {res.chi2_before:.6g} -> {res.chi2_after:.6g}, trials {res.trials}, device_ms {res.device_ms:.1f}")
    assert np.isfinite(dev).all() and res.iterations == 2
    assert res.chi2_after < 0.5 * res.chi2_before
    R = dev[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12


def test_map_array_pose_adjustment_with_70_loop_edges(reg):
    """A MapArray of 48 two-point submaps and 70 accepted loop edges (plus one rejected, which is skipped): pose_adjustment no longer
    raises, and its poses are pose_graph.optimize's on the same edges, bit for bit."""
    rng = np.random.default_rng(11)
    GT = PC.circle(48, 10.0, 24, 0.02)
    X = PC.drifted(GT, 0.03, 0.002, rng)
    ma = MapArray()
    for i, T in enumerate(X):
        ma.append(np.zeros((2, 8), np.float32), T, float(i))
    pairs = set()
    while len(pairs) < 70:
        a, b = sorted(int(v) for v in rng.integers(1, 48, 2))
        if b - a > 5:
            pairs.add((a, b))
    loops = [LoopEdge((a, b), O.inv(GT[a]) @ GT[b], 0.1, True) for a, b in sorted(pairs)]
    results = []
    poses = ma.pose_adjustment(reg, loops + [LoopEdge((2, 40), np.eye(4), 9.0, False)], result=results)
    stored = ma.stored_poses()
    E = pose_graph.adjacent_edges(stored, 5) + [(e.pair_id[0], e.pair_id[1], e.relative_pose) for e in loops]
    assert _off_band(E) == 70
    want, wres = pose_graph.optimize(reg, stored, E)
    assert np.array_equal(poses, want) and results[0].trace == wres.trace
    assert np.isfinite(poses).all() and results[0].chi2_after < results[0].chi2_before

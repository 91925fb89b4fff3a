"""Pose-graph optimisation: the optimiser half of GraphBasedSlamComponent::doPoseAdjustment
(graph_based_slam_component.cpp:267-319) behind `lsr_optimize_pose_graph_long` — g2o's VertexSE3 / EdgeSE3 graph with identity information,
vertex 0 fixed, ten Levenberg-Marquardt iterations, solved on the device; no g2o.  Up to 1024 edges outside the band (every loop edge a
node has accepted over a few laps); within the 64 of `lsr_optimize_pose_graph` the result is that entry's, bit for bit.

An edge is `(from, to, Z)` with Z the 4x4 fp64 measurement from^-1 * to — what `LoopEdge.relative_pose` holds.  `adjacent_edges` makes
the odometry edges the reference adds (:289-303), `optimize` runs the optimiser; `MapArray.pose_adjustment` chains both behind the
accepted edges of `search_loop` and returns the poses `MapArray.modified_map` takes.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

from . import _capi

NUM_ADJACENT_POSE_CONSTRAINTS = 5    # graph_based_slam_component.cpp:40
STOP_REASONS = ("max_iterations", "trials", "rho_zero", "lambda")


@dataclass
class PoseGraphResult:
    iterations: int
    trials: int
    chi2_before: float
    chi2_after: float
    lam: float
    stop_reason: str
    device_ms: float
    trace: List[dict] = field(default_factory=list)   # per iteration: trials, chi2, lam, rho


def _col16(poses) -> np.ndarray:
    P = np.asarray(poses, np.float64)
    if P.ndim != 3 or P.shape[1:] != (4, 4):
        raise ValueError("poses: (n, 4, 4)")
    return np.ascontiguousarray(P.transpose(0, 2, 1).reshape(len(P), 16))


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def adjacent_edges(poses, k: int = NUM_ADJACENT_POSE_CONSTRAINTS) -> List[Tuple[int, int, np.ndarray]]:
    """The odometry edges of :289-303 through lsr_pose_graph_edges (host only): for i > k (strictly), j = 0 .. k-1, the edge
    (i - k + j -> i) measured from `poses`."""
    lib = _capi.load()
    P = _col16(poses)
    n = len(P)
    cap = max(0, n - k - 1) * k
    out = (_capi.PoseEdge * max(cap, 1))()
    n_out = C.c_size_t()
    _capi.check(lib.lsr_pose_graph_edges(_dp(P), n, int(k), out, cap, C.byref(n_out)), "poseGraphEdges")
    return [(e.from_, e.to, np.array(e.measurement[:], np.float64).reshape(4, 4, order="F")) for e in out[:n_out.value]]


def optimize(registration, poses, edges: Sequence[Tuple[int, int, np.ndarray]], max_iterations: int = 10,
             band: int = NUM_ADJACENT_POSE_CONSTRAINTS, entry: str = "lsr_optimize_pose_graph_long"):
    """optimizer.optimize(max_iterations) (:317-318) on the device of `registration`, through lsr_optimize_pose_graph_long: up to
    _capi.POSE_GRAPH_LONG_MAX_OFFBAND_EDGES edges with |from - to| > band.  `entry`: the C entry point; "lsr_optimize_pose_graph" keeps
    its limit of _capi.POSE_GRAPH_MAX_OFFBAND_EDGES (the same bits within it).  -> ((n, 4, 4) fp64 poses, PoseGraphResult)."""
    if entry not in ("lsr_optimize_pose_graph_long", "lsr_optimize_pose_graph"):
        raise ValueError("entry: lsr_optimize_pose_graph_long or lsr_optimize_pose_graph")
    lib = _capi.load()
    P = _col16(poses)
    n, m = len(P), len(edges)
    arr = (_capi.PoseEdge * max(m, 1))()
    for i, (a, b, Z) in enumerate(edges):
        arr[i].from_, arr[i].to = int(a), int(b)
        arr[i].measurement[:] = np.asarray(Z, np.float64).reshape(4, 4).T.reshape(16).tolist()
    params = _capi.PoseGraphParams(int(max_iterations), int(band))
    out = np.zeros((n, 16), np.float64)
    res = _capi.PoseGraphResult()
    trace = (_capi.PoseGraphTrace * max(int(max_iterations), 1))()
    _capi.check(getattr(lib, entry)(registration._h, _dp(P), n, arr, m, C.byref(params), _dp(out), C.byref(res), trace),
                "optimizePoseGraph")
    tr = [dict(trials=t.trials, chi2=t.chi2, lam=t.lam, rho=t.rho) for t in trace[:res.iterations]]
    return (out.reshape(n, 4, 4).transpose(0, 2, 1).copy(),
            PoseGraphResult(res.iterations, res.trials, res.chi2_before, res.chi2_after, res.lam, STOP_REASONS[res.stop_reason],
                            res.device_ms, tr))

#!/usr/bin/env python3
"""Pose-graph optimisation (lsr_optimize_pose_graph_long) against the machine: `device_ms` — the hipEvent time of a whole
call on the object's stream, uploads, the host controller's read-backs and the final download included — for reference-shaped graphs
(laps round a circle, drift composed per step, k = 5 odometry edges per vertex, 6 loop edges, ten iterations).  Standalone: reads
nothing outside the repository, generates its graphs from a seed.

    python tools/pose_graph_probe.py [--sizes 200 1000 4000] [--loops 6 0] [--reps 5] [--warmup 1] [--out profiles/pose_graph_rows.json]
    python tools/pose_graph_probe.py --sizes 1000 4000 --loops 64 65 256 1024 --reps 3 --stages --append --out profiles/pose_graph_rows.json
    python tools/pose_graph_probe.py --sizes 1000 4000 --loops 64 65 256 1024 --reps 3 --entry old     (the 64-edge rows through lsr_optimize_pose_graph)

One JSON row per size and loop-edge count (without a loop edge the solve is the band alone: one right-hand side, one active lane): vertices, edges, iterations, trials, chi2 before / after, device_ms (median / min / max of `reps` after
`warmup`), the host clock around the call, and device_ms per trial.  From 7 loop edges on they are distinct pairs whole laps apart, spread evenly
over the drive; past 64 of them the dense part of the solve is the blocked Cholesky of csrc/pose_graph_dense.hip.  With --stages
one more call per row runs with the library's own event brackets (lsr_set_i32(LSR_PROFILE)) and the row also carries
`stage_ms`: band solve (right-hand sides included), dense part, row combine, each summed over the call's trials, and their share of that
call's device_ms.  The share of each kernel (the band factor is the only long
dependent chain) comes from a run of its own under the profiler, which slows the host and is not mixed with the figures above:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/pose_graph_probe.py --sizes 4000 --reps 1 --warmup 0
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _rot_z(th):
    T = np.eye(4)
    T[0, 0] = T[1, 1] = np.cos(th)
    T[0, 1], T[1, 0] = -np.sin(th), np.sin(th)
    return T


def _small_motion(rng, sigma_t, sigma_r):
    """a rigid motion close to the identity: rotation vector ~ N(0, sigma_r) by Rodrigues, translation ~ N(0, sigma_t)"""
    w = rng.normal(size=3) * sigma_r
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + (np.sin(a) / a) * K + ((1 - np.cos(a)) / (a * a)) * (K @ K) if a > 0 else np.eye(3)
    T[:3, 3] = rng.normal(size=3) * sigma_t
    return T


def make_graph(n, k=5, n_loops=6, seed=3):
    """-> (start poses (n, 4, 4), edges): 100 vertices per lap of a radius-30 circle, loop edges one lap apart measured from the truth"""
    from lidarslam_ros2_amd import pose_graph

    rng = np.random.default_rng(seed)
    truth = []
    for i in range(n):
        T = _rot_z(2 * np.pi * i / 100)
        T[:3, 3] = [30 * np.cos(2 * np.pi * i / 100) - 30, 30 * np.sin(2 * np.pi * i / 100), 0.02 * i]
        truth.append(T)
    X = [truth[0]]
    for i in range(1, n):
        X.append(X[-1] @ np.linalg.inv(truth[i - 1]) @ truth[i] @ _small_motion(rng, 0.03, 0.004))
    X = np.stack(X)
    edges = pose_graph.adjacent_edges(X, k)
    starts = np.linspace(0, n - 101, n_loops).astype(int) if n_loops else []
    if n_loops > 6:   # the rows with many loop edges: none into the fixed vertex, no pair twice — every one of them a slot of U —,
        # whole laps apart (one lap alone has room for n - 101 of them), picked evenly from all such pairs
        cand = [(a, a + 100 * j) for j in range(1, (n - 2) // 100 + 1) for a in range(1, n - 100 * j)]
        if len(cand) < n_loops:
            raise SystemExit(f"pose_graph_probe: {n} vertices have no room for {n_loops} distinct loop edges whole laps apart")
        pick = sorted(cand[i] for i in np.linspace(0, len(cand) - 1, n_loops).astype(int))
        edges += [(a, b, np.linalg.inv(truth[a]) @ truth[b]) for a, b in pick]
        assert len(set(pick)) == n_loops
        return X, edges
    edges += [(int(a), int(a) + 100, np.linalg.inv(truth[a]) @ truth[a + 100]) for a in starts]
    return X, edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[200, 1000, 4000])
    ap.add_argument("--loops", type=int, nargs="+", default=[6, 0], help="loop edges per graph; 0: the band solve alone, one right-hand side")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep the rows already in --out and add these")
    ap.add_argument("--stages", action="store_true", help="one more call per row under LSR_PROFILE: band solve, dense part, row combine")
    ap.add_argument("--entry", choices=("long", "old"), default="long",
                    help="old: lsr_optimize_pose_graph for the rows within its 64 edges outside the band (the others are skipped)")
    a = ap.parse_args()
    import torch

    from lidarslam_ros2_amd import NormalDistributionsTransform, _capi, pose_graph

    if not torch.cuda.is_available():
        raise SystemExit("pose_graph_probe: no GPU visible (there is no CPU path to time)")
    reg = NormalDistributionsTransform(device=0)
    entry = "lsr_optimize_pose_graph" if a.entry == "old" else "lsr_optimize_pose_graph_long"
    rows = []
    for n, loops in [(n, l) for n in a.sizes for l in a.loops]:
        if a.entry == "old" and loops > _capi.POSE_GRAPH_MAX_OFFBAND_EDGES:
            continue
        X, edges = make_graph(n, n_loops=loops)
        ms, wall, res = [], [], None
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            _, res = pose_graph.optimize(reg, X, edges, entry=entry)
            t1 = time.perf_counter()
            if r >= a.warmup:
                ms.append(res.device_ms)
                wall.append((t1 - t0) * 1e3)
        ms.sort()
        row = dict(vertices=n, loop_edges=loops, edges=len(edges), iterations=res.iterations, trials=res.trials, chi2_before=res.chi2_before,
                   chi2_after=res.chi2_after, device_ms_median=ms[len(ms) // 2], device_ms_min=ms[0], device_ms_max=ms[-1],
                   call_wall_ms_median=sorted(wall)[len(wall) // 2], device_ms_per_trial=ms[len(ms) // 2] / max(res.trials, 1), reps=len(ms),
                   entry=entry)
        if a.stages:   # a call of its own: the brackets add four event records per trial
            reg._seti(_capi.PROFILE, 1, "setProfile")
            _, pres = pose_graph.optimize(reg, X, edges, entry=entry)
            reg._seti(_capi.PROFILE, 0, "setProfile")
            parts = [reg._getf(k) for k in (_capi.POSE_GRAPH_BAND_SOLVE_MS, _capi.POSE_GRAPH_DENSE_MS, _capi.POSE_GRAPH_COMBINE_MS)]
            row["stage_ms"] = dict(zip(("band_solve", "dense", "combine"), parts), device_ms=pres.device_ms)
            row["stage_share"] = dict(zip(("band_solve", "dense", "combine"), [p / pres.device_ms for p in parts]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        if a.append and os.path.exists(a.out):
            with open(a.out) as f:
                rows = json.load(f) + rows
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

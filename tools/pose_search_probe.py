#!/usr/bin/env python
"""Times the NDT pose search (lsr_ndt_score_poses, lsr_ndt_search_pose; csrc/pose_search.hip) on one MI355X: the scores of the
21 x 21 x 1 x 72 = 31 752-pose lattice (+-10 m at 1 m, the whole circle at 5 degrees) of the cfg-1/2 scan (30 000 points) against its
submap at resolution 2.0 — hipEvents through LSR_POSE_SEARCH_MS, warmed up, repeated to show the spread —, the same scan thinned to
vg 1.0, what the call costs around the launch (pose upload, score download, the host's finiteness check), the whole searchPose with
top_k = 16, and the same scores the only way the library offered before: one lsr_ndt_derivatives call per pose, on a 512-pose subset.

    python tools/pose_search_probe.py [--reps 7] [--warmup 2] [--table-mode -1] [--out profiles/pose_search.md]
    python tools/pose_search_probe.py --counters       # three scoring launches and nothing else: the run to put under the profiler

Prints one JSON line; --out writes the note (the counters of a profiler run are added by hand: kernel resources and VALU share)."""
import argparse
import json
import math
import multiprocessing as mp
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _cache import cached  # noqa: E402
from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform, poseLattice, synth  # noqa: E402

RES = 2.0
LATTICE = dict(n=(21, 21, 1), step=(1.0, 1.0, 1.0), n_yaw=72, yaw_step=math.radians(5.0))


def _make():
    with mp.get_context("fork").Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
        return synth.cfg_ndt_30k(pool=pool)


def _ndt(case, source, table_mode):
    ndt = NormalDistributionsTransform(device=0)
    ndt.setResolution(RES)
    ndt.setTransformationEpsilon(0.01)
    ndt.setNeighborhoodSearchMethod(DIRECT7)
    if table_mode >= 0:
        ndt.setTuning(table_mode=table_mode)
    ndt.setInputTarget(synth.as_pointxyzi(case.target))
    ndt.setInputSource(synth.as_pointxyzi(source))
    ndt.setProfiling(True)
    return ndt


def _spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def _score_times(ndt, poses, warmup, reps):
    kernel, wall = [], []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        score, pairs = ndt.scorePoses(poses)
        t1 = time.perf_counter()
        if k >= warmup:
            kernel.append(ndt.poseSearchMs())
            wall.append(1e3 * (t1 - t0))
    return _spread(kernel), _spread(wall), score, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--table-mode", type=int, default=-1)
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("pose_search_probe.py measures on the GPU: none is visible")
    case = cached("probe_cfg_ndt_30k", _make)
    truth = np.asarray(case.truth, np.float32)
    center = synth.pose_matrix(truth[0, 3] + 3.4, truth[1, 3] - 2.7, 0.0, 2.0).astype(np.float32)   # off the truth, heading unknown
    poses = poseLattice(center, **LATTICE)
    ndt = _ndt(case, case.source, a.table_mode)
    if a.counters:
        for _ in range(3):
            ndt.scorePoses(poses)
        print(json.dumps(dict(tool="pose_search_probe", counters_run=True, poses=int(poses.shape[0]), points=int(case.source.shape[0]))))
        return
    row = dict(poses=int(poses.shape[0]), points=int(case.source.shape[0]), target_points=int(case.target.shape[0]),
               n_valid_leaves=int(ndt.gridInfo()["n_valid"]), table_mode=a.table_mode, reps=a.reps, warmup=a.warmup)
    k_ms, w_ms, score, pairs = _score_times(ndt, poses, a.warmup, a.reps)
    row["score_kernel_ms"], row["score_call_ms"] = k_ms, w_ms
    row["pairs_total"] = float(pairs.sum())
    row["ns_per_pair"] = 1e6 * k_ms["median"] / max(1.0, float(pairs.sum()))
    # the scan thinned to vg 1.0
    thin = ndt.voxelGridFilter(synth.as_pointxyzi(case.source), 1.0)[:, :3]
    ndt_thin = _ndt(case, thin, a.table_mode)
    kt, wt, _, _ = _score_times(ndt_thin, poses, a.warmup, a.reps)
    row["thin_points"], row["thin_kernel_ms"], row["thin_call_ms"] = int(thin.shape[0]), kt, wt
    # the whole search
    t = []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        pose, result, rep = ndt.searchPose(center, top_k=16, min_sep_m=0.9, min_sep_rad=math.radians(7.5), **LATTICE)
        if k >= a.warmup:
            t.append(1e3 * (time.perf_counter() - t0))
    row["search_call_ms"] = _spread(t)
    from lidarslam_ros2_amd.posemath import pose_delta

    row["search_error_m_rad"] = [float(v) for v in pose_delta(pose, case.truth)]
    row["search_winner_rank"] = int(rep["winner"])
    # the only way before: one derivative pass per pose
    sub = np.random.default_rng(0).choice(poses.shape[0], 512, replace=False)
    p0 = np.zeros(6)
    for T in poses[sub[:16]]:
        ndt.derivatives(p0, T=T, compute_hessian=False)
    t0 = time.perf_counter()
    ref = [ndt.derivatives(p0, T=T, compute_hessian=False)[0] for T in poses[sub]]
    row["derivatives_ms_per_pose"] = 1e3 * (time.perf_counter() - t0) / 512
    row["derivatives_equal_bits"] = bool(np.array_equal(np.array(ref), score[sub]))
    row["ratio_per_pose"] = row["derivatives_ms_per_pose"] / (w_ms["median"] / poses.shape[0])
    print(json.dumps(dict(tool="pose_search_probe", row=row)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# NDT pose search: scoring a pose lattice in one launch\n\n")
            f.write(f"`python tools/pose_search_probe.py --reps {a.reps} --warmup {a.warmup} --table-mode {a.table_mode}` on one MI355X; "
                    "times in ms as min / median / max over the repetitions.\n\n")
            f.write("| what | ms |\n|---|---|\n")
            fmt = lambda s: f"{s['min']:.3f} / {s['median']:.3f} / {s['max']:.3f}"
            f.write(f"| {row['poses']} poses x {row['points']} points, scoring launch (hipEvents, LSR_POSE_SEARCH_MS) | {fmt(k_ms)} |\n")
            f.write(f"| the same, whole scorePoses call (finiteness check, upload, launch, download) | {fmt(w_ms)} |\n")
            f.write(f"| scan thinned to vg 1.0 ({row['thin_points']} points), scoring launch | {fmt(kt)} |\n")
            f.write(f"| the same, whole call | {fmt(wt)} |\n")
            f.write(f"| whole searchPose, top_k = 16 | {fmt(row['search_call_ms'])} |\n")
            f.write(f"| one lsr_ndt_derivatives call per pose (512 of them), per pose | {row['derivatives_ms_per_pose']:.4f} |\n\n")
            f.write(f"Per pose: {row['ratio_per_pose']:.0f} times faster than one derivative call each "
                    f"({1e3 * w_ms['median'] / row['poses']:.3f} us against {1e3 * row['derivatives_ms_per_pose']:.1f} us); "
                    f"{row['pairs_total']:.3g} (point, voxel) pairs per list, {row['ns_per_pair']:.4f} ns per pair in the launch.  "
                    f"Scores equal to the derivative passes' bits: {row['derivatives_equal_bits']}.  searchPose ended "
                    f"{row['search_error_m_rad'][0]:.4f} m / {row['search_error_m_rad'][1]:.2e} rad from the truth (winner: rank {row['search_winner_rank']}).\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Times Scan Context and the appearance loop gate (csrc/scan_context.hip, lsr_search_loop_appearance) on one MI355X: the descriptor
of one new submap (18 k points, and a full-revolution one of the cfg_loop_route_full kind: that sensor and filter, 66 k points at the
route's start) and of 500 submaps in one call;
one query against 100, 1 000 and 10 000 stored descriptors; the whole appearance gate beside lsr_search_loop on the route both close;
and what the device finds on the drifted route of tests/scan_context_numpy.py.  Kernel times are hipEvents through
LSR_SCAN_CONTEXT_BUILD_MS / _MATCH_MS, call times the wall clock around the Python call; warmed up, repeated to show the spread.

    python tools/scan_context_probe.py [--reps 9] [--warmup 3] [--out profiles/scan_context.md]

Prints one JSON line; --out writes the note."""
import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _cache import cached  # noqa: E402
from lidarslam_ros2_amd import (DIRECT7, AppearanceLoopParams, LoopClosureParams, NormalDistributionsTransform, ScanContextParams,  # noqa: E402
                                SubMap, search_loop, search_loop_appearance, synth)

LOOP = dict(threshold_loop_closure_score=1.0, distance_loop_closure=20.0, range_of_searching_loop_closure=10.0, search_submap_num=2,
            voxel_leaf_size=0.2)


def _big_submaps():
    s = synth.vlp32()
    sensor = synth.Sensor(s.n_beams, s.elev_min_deg, s.elev_max_deg, s.n_azimuth * 3, s.range_noise, s.max_range, s.min_range)
    with mp.get_context("fork").Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
        return [sm["cloud"] for sm in synth.make_loop_route(spacing=3.0, length=3.0, sensor=sensor, vg_map=0.1, pool=pool)[:2]]


def _spread(v):
    v = sorted(v)
    return dict(min=v[0], median=v[len(v) // 2], max=v[-1])


def _backend():
    ndt = NormalDistributionsTransform(0)
    ndt.setMaximumIterations(100)
    ndt.setResolution(5.0)
    ndt.setTransformationEpsilon(0.01)
    ndt.setNeighborhoodSearchMethod(DIRECT7)
    return ndt


def _timed(fn, warmup, reps, kernel=None):
    wall, kern = [], []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if k >= warmup:
            wall.append(1e3 * (t1 - t0))
            if kernel:
                kern.append(kernel())
    return _spread(wall), (_spread(kern) if kernel else None), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("scan_context_probe.py measures on the GPU: none is visible")
    import scan_context_numpy as SC

    prm = ScanContextParams()
    route = synth.make_loop_route()
    big = cached("probe_sc_big_submaps", _big_submaps)
    reg = NormalDistributionsTransform(0)
    reg.setProfiling(True)
    row = dict(reps=a.reps, warmup=a.warmup)

    def dev(cloud):
        return torch.from_numpy(synth.as_pointxyzi(cloud)).cuda()

    def sub(cloud):
        return SubMap(cloud, (0.0, 0.0, 0.0))

    # ---- build
    small_h, small_d = synth.as_pointxyzi(route[0]["cloud"]), dev(route[0]["cloud"])
    big_h, big_d = synth.as_pointxyzi(big[0]), dev(big[0])
    row["small_points"], row["big_points"] = int(small_h.shape[0]), int(big_h.shape[0])
    for name, cloud in (("small_device", small_d), ("small_host", small_h), ("big_device", big_d), ("big_host", big_h)):
        w, k, _ = _timed(lambda: reg.scanContext([sub(cloud)], prm), a.warmup, a.reps, lambda: reg.scanContextMs()[0])
        row["build_" + name] = dict(call_ms=w, kernel_ms=k)
    many = [sub(dev(route[i % len(route)]["cloud"])) for i in range(len(route))]
    many = [many[i % len(many)] for i in range(500)]
    row["many_points"] = int(sum(int(s.cloud.shape[0]) for s in many))
    w, k, D500 = _timed(lambda: reg.scanContext(many, prm), a.warmup, a.reps, lambda: reg.scanContextMs()[0])
    row["build_500_device"] = dict(call_ms=w, kernel_ms=k)

    # ---- match: one query against N stored descriptors (device resident), distinct rolls of the route's
    base = D500[: len(route)]
    for n in (100, 1000, 10000):
        stored = torch.stack([torch.roll(base[i % len(route)], (i // len(route)) % 60, dims=1) for i in range(n)]).contiguous()
        q = base[len(route) - 1].contiguous()
        torch.cuda.synchronize()
        w, k, (d, s) = _timed(lambda: reg.matchScanContext(q, stored, prm), a.warmup, a.reps, lambda: reg.scanContextMs()[1])
        row["match_%d" % n] = dict(call_ms=w, kernel_ms=k, self_distance=float(d[0, len(route) - 1]), self_shift=int(s[0, len(route) - 1]))

    # ---- the gates on the route both close (submaps and descriptors resident)
    subs = [SubMap(dev(sm["cloud"]), sm["position"], sm["orientation"], sm["distance"]) for sm in route]
    ndt = _backend()
    D = ndt.scanContext(subs, prm)
    w_range, _, e_range = _timed(lambda: search_loop(ndt, subs, LoopClosureParams(**LOOP)), a.warmup, a.reps)
    app = AppearanceLoopParams(loop=LoopClosureParams(**LOOP))
    w_app, _, e_app = _timed(lambda: search_loop_appearance(ndt, subs, D, app), a.warmup, a.reps)
    guess_only = AppearanceLoopParams(loop=LoopClosureParams(**LOOP), lattice_n=(1, 1, 1), search_top_k=1)
    w_guess, _, e_guess = _timed(lambda: search_loop_appearance(ndt, subs, D, guess_only), a.warmup, a.reps)
    w_desc, _, _ = _timed(lambda: ndt.scanContext(subs[-1:], prm), a.warmup, a.reps)
    w_match, _, _ = _timed(lambda: ndt.matchScanContext(D[-1], D, prm), a.warmup, a.reps)
    from lidarslam_ros2_amd.posemath import pose_delta

    def err(e):
        truth = np.linalg.inv(route[e.pair_id[0]]["truth"]) @ route[-1]["truth"]
        return [float(v) for v in pose_delta(e.relative_pose, truth)]

    row["gate"] = dict(range_gate_ms=w_range, appearance_ms=w_app, appearance_guess_only_ms=w_guess, new_descriptor_ms=w_desc,
                       match_21_ms=w_match, range_pair=list(e_range[0].pair_id), appearance_pair=list(e_app[0].pair_id),
                       range_error=err(e_range[0]), appearance_error=err(e_app[0]), appearance_shift=e_app[0].shift,
                       appearance_sc_distance=e_app[0].sc_distance)

    # ---- the drifted route: what the device finds
    drifted = SC.drifted_route()
    dsubs = [SubMap(dev(sm["cloud"]), sm["position"], sm["orientation"], sm["distance"]) for sm in drifted]
    nd = _backend()
    DD = nd.scanContext(dsubs, prm)
    dist, shift = nd.matchScanContext(DD[-1], DD, prm)
    full = dict(LOOP, range_of_searching_loop_closure=20.0, search_submap_num=3)
    edges = search_loop_appearance(nd, dsubs, DD, AppearanceLoopParams(loop=LoopClosureParams(**full, top_k=2)))
    old = search_loop(_backend(), dsubs, LoopClosureParams(**full, top_k=16))

    def derr(e):
        truth = np.linalg.inv(drifted[e.pair_id[0]]["truth"]) @ drifted[-1]["truth"]
        return [float(v) for v in pose_delta(e.relative_pose, truth)]

    row["drifted"] = dict(distance=[float(v) for v in dist[0]], shift=[int(v) for v in shift[0]],
                          range_gate=[dict(pair=list(e.pair_id), fitness=e.fitness_score, accepted=e.accepted) for e in old],
                          appearance=[dict(pair=list(e.pair_id), sc_distance=e.sc_distance, shift=e.shift, fitness=e.fitness_score,
                                           accepted=e.accepted, error=derr(e), stored_distance=e.candidate_distance) for e in edges])
    print(json.dumps(dict(tool="scan_context_probe", row=row)))
    if a.out:
        fmt = lambda s: f"{s['min']:.3f} / {s['median']:.3f} / {s['max']:.3f}"   # noqa: E731
        with open(a.out, "w") as f:
            f.write("# Scan Context and the appearance loop gate\n\n")
            f.write(f"`python tools/scan_context_probe.py --reps {a.reps} --warmup {a.warmup}` on one MI355X, one session; times in ms as "
                    "min / median / max over the repetitions.  Launch: hipEvents around the kernel (`LSR_SCAN_CONTEXT_BUILD_MS`, "
                    "`LSR_SCAN_CONTEXT_MATCH_MS`); call: the wall clock around the Python call (table upload, zeroing of the output, "
                    "launch, copies, synchronisation).  20 rings x 60 sectors, 80 m.\n\n")
            f.write("## Descriptors\n\n| what | launch | call |\n|---|---|---|\n")
            for key, label in (("small_device", f"one submap, {row['small_points']} points, resident"),
                               ("small_host", f"one submap, {row['small_points']} points, host records (staged)"),
                               ("big_device", f"one submap, {row['big_points']} points, resident"),
                               ("big_host", f"one submap, {row['big_points']} points, host records (staged)"),
                               ("500_device", f"500 submaps in one call, {row['many_points']} points, resident")):
                r = row["build_" + key]
                f.write(f"| {label} | {fmt(r['kernel_ms'])} | {fmt(r['call_ms'])} |\n")
            b500 = row["build_500_device"]["kernel_ms"]["median"]
            f.write(f"\n500 submaps: {1e3 * b500 / 500:.2f} us per submap in the launch, {row['many_points'] * 32 / (b500 * 1e-3) / 1e12:.2f} TB/s "
                    "of 32-byte records read — the 500 entries repeat the route's 21 clouds (12 MB), so the reads are served by the caches: "
                    "this is the kernel's own rate (29 boundary tests and 19 ring tests per point, from LDS), not an HBM figure.  One submap "
                    "is bound by launch and call overhead: 5 to 17 workgroups of 4 096 points each, the same launch time for 18 k and 65 k points.\n\n")
            f.write("## One query against N stored descriptors\n\n| N | launch | call |\n|---|---|---|\n")
            for n in (100, 1000, 10000):
                r = row["match_%d" % n]
                f.write(f"| {n} | {fmt(r['kernel_ms'])} | {fmt(r['call_ms'])} |\n")
            m = row["match_10000"]["kernel_ms"]["median"]
            f.write(f"\n10 000 candidates: {1e3 * m / 10000:.3f} us per pair in the launch (72 000 multiply-adds each, one lane per shift, "
                    "sequential by definition); at 100 the launch latency dominates.  Brute force over every stored descriptor: no ring-key "
                    "tree is needed at these sizes.\n\n")
            g = row["gate"]
            f.write("## The gates on the route both close (21 submaps of ~18 k points, resident; NDT resolution 5.0)\n\n| what | call |\n|---|---|\n")
            f.write(f"| `search_loop` (range gate, align without guess) -> pair {tuple(g['range_pair'])} | {fmt(g['range_gate_ms'])} |\n")
            f.write(f"| `search_loop_appearance`, 7 x 7 lattice, 16 refined -> pair {tuple(g['appearance_pair'])} | {fmt(g['appearance_ms'])} |\n")
            f.write(f"| `search_loop_appearance`, the guess alone (1 x 1 lattice) | {fmt(g['appearance_guess_only_ms'])} |\n")
            f.write(f"| the new keyframe's descriptor (`scanContext` of one submap) | {fmt(g['new_descriptor_ms'])} |\n")
            f.write(f"| the comparison alone (`matchScanContext`, 1 x 21) | {fmt(g['match_21_ms'])} |\n\n")
            f.write(f"Extra cost of appearance over the range gate: {g['appearance_ms']['median'] - g['range_gate_ms']['median']:.3f} ms per call "
                    f"with the lattice, {g['appearance_guess_only_ms']['median'] - g['range_gate_ms']['median']:.3f} ms with the guess alone "
                    "(descriptor of the new keyframe not included: it is made once when the keyframe arrives).  The lattice's share is the "
                    "refinement of up to 16 starts as one candidate set, bound by the NDT launch chain; the comparison and the descriptor are "
                    f"bound by launch latency.  Error against the ground-truth relative pose: range gate {g['range_error'][0]:.4f} m / "
                    f"{g['range_error'][1]:.2e} rad, appearance {g['appearance_error'][0]:.4f} m / {g['appearance_error'][1]:.2e} rad "
                    f"(shift {g['appearance_shift']}, Scan Context distance {g['appearance_sc_distance']:.4f}).\n\n")
            d = row["drifted"]
            f.write("## The drifted route (tests/scan_context_numpy.py: drift to 25 m, -15 m, 0.3 m, 0.5 rad after the turn)\n\n")
            f.write("Scan Context distance and shift of the last submap to every submap, on the device:\n\n| submap | distance | shift |\n|---|---|---|\n")
            for i, (v, s) in enumerate(zip(d["distance"], d["shift"])):
                f.write(f"| {i} | {v:.7f} | {s} |\n")
            f.write("\nRange gate (`search_loop`, defaults, top_k 16): " +
                    ", ".join(f"{tuple(e['pair'])} fitness {e['fitness']:.3f} {'accepted' if e['accepted'] else 'rejected'}" for e in d["range_gate"]) + ".\n\n")
            f.write("Appearance gate: " +
                    "; ".join(f"{tuple(e['pair'])} distance {e['sc_distance']:.4f} shift {e['shift']} stored {e['stored_distance']:.1f} m away, fitness "
                              f"{e['fitness']:.4f} {'accepted' if e['accepted'] else 'rejected'}, {e['error'][0] * 1e3:.1f} mm / {e['error'][1]:.1e} rad from the truth"
                              for e in d["appearance"]) + ".\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times thinning the whole map on the device (lsr_voxel_grid_filter_map, lsr_assemble_map_filtered, lsr_save_map_pcd_filtered;
csrc/map_filter.hip).  A tool, not a test; it is not wired into bench.py.

    python tools/map_filter_profile.py [--keyframes 628] [--points 20000] [--leaf 0.1] [--reps 7] [--warmup 2] [--dir DIR]
                                       [--out profiles/map_filter.md]

The map: a synthetic drive once round a circle of --keyframes * 1.5 m, a keyframe of --points pcl::PointXYZI records every 1.5 m —
ground within 50 m of the sensor and two walls along the road, on a hill of +-20 m, so that every spot is seen from dozens of
keyframes —, the submaps resident in HBM, pose-local.  At 628 keyframes the map spans 400 m x 400 m x 53 m: 8.5e9 cells at a 0.1 m
leaf, beyond the int32 index.  A second, small drive (a quarter of the keyframes, flat) stays inside it and also takes the only route
there was before: lsr_assemble_map to the host, then lsr_voxel_grid_filter_pc2 host in / host out.

Timed legs (median, min - max over --reps after --warmup; the legs interleaved in one run): lsr_assemble_map alone (LSR_MAP_ASSEMBLY_MS,
hipEvents); lsr_assemble_map_filtered launch by launch (LSR_MAP_FILTER_*_MS, hipEvents) and as a whole (host clock: the call returns
synchronised); lsr_save_map_pcd against lsr_save_map_pcd_filtered for the three data kinds (host clock, file in --dir, default /dev/shm
when there is one) with the files' sizes.  Bytes/s of the key, sort and centroid launches: the bytes the algorithm moves, counted
from the shapes below, over the launch's time, against the 8 TB/s HBM peak.  Prints one JSON line and writes the table.  There is no
threshold."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KINDS = ("ascii", "binary", "binary_compressed")
HBM_PEAK = 8.0e12
LEGS = ("bbox", "key", "sort", "runs", "centroid", "write")


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _fmt(s, digits=2):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f} – {s['max']:.{digits}f}, n = {s['n']})"


def make_drive(np, keyframes, points, hill, seed):
    """-> (list of (points, 8) float32 pose-local PointXYZI records, (keyframes, 4, 4) fp64 poses)."""
    rng = np.random.default_rng(seed)
    R = keyframes * 1.5 / (2 * np.pi)
    clouds, poses = [], []
    n_ground = points * 6 // 10
    for k in range(keyframes):
        th = 2 * np.pi * k / keyframes
        c = np.array([R * np.cos(th), R * np.sin(th), hill * np.sin(th)])
        yaw = th + np.pi / 2
        P = np.eye(4)
        P[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1]]
        P[:3, 3] = c
        r, phi = 50.0 * np.sqrt(rng.uniform(0.002, 1.0, n_ground)), rng.uniform(0, 2 * np.pi, n_ground)
        gx, gy = c[0] + r * np.cos(phi), c[1] + r * np.sin(phi)
        ground = np.column_stack([gx, gy, hill * gy / R + rng.normal(0, 0.02, n_ground)])   # the hill's plane through the road
        n_wall = points - n_ground
        al = th + rng.uniform(-0.3, 0.3, n_wall) * min(1.0, 150.0 / R)
        rad = R + np.where(rng.random(n_wall) < 0.5, -10.0, 10.0) + rng.normal(0, 0.02, n_wall)
        wall = np.column_stack([rad * np.cos(al), rad * np.sin(al), hill * np.sin(al) + rng.uniform(0, 5, n_wall)])
        world = np.vstack([ground, wall])
        local = (world - c) @ P[:3, :3]          # R^T (w - c)
        rec = np.zeros((points, 8), np.float32)
        rec[:, :3] = local
        rec[:, 4] = rng.uniform(0, 255, points)
        clouds.append(rec)
        poses.append(P)
    return clouds, np.stack(poses)


def key_bytes(n, wide):
    return n * (32 + 4 + (8 if wide else 0))


def sort_bytes(n, bits):
    """Per pass: the histogram reads the keys, the scatter reads and writes (key, value); the first pass of a sort with implicit values
    reads none.  A wide index: two sorts and two gathers (order and a word read, a word written)."""
    def one(b, iota):
        passes = (b + 10) // 11
        return passes * (4 * n + 16 * n) - (4 * n if iota else 0)
    if bits <= 32:
        return one(bits, True)
    return one(32, True) + one(bits - 32, False) + 2 * 12 * n


def centroid_bytes(n, m, wide):
    return n * ((8 if wide else 4) + 4 + 32) + 16 * m


def profile_map(a, name, reg, capi, torch, np, keyframes, hill, baseline):
    from lidarslam_ros2_amd import MapArray

    clouds, poses = make_drive(np, keyframes, a.points, hill, seed=keyframes)
    ma = MapArray()
    for rec, P in zip(clouds, poses):
        ma.append(torch.from_numpy(rec).cuda(), P, 0.0)
    n = keyframes * a.points
    row = dict(map=name, keyframes=keyframes, records=n, leaf=a.leaf)
    raw = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    thin = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    asm_ms, legs, whole_ms = [], {k: [] for k in LEGS}, []
    save = {(k, f): [] for k in KINDS for f in (False, True)}
    size = {}
    path = os.path.join(a.dir, f"map_filter_profile_{name}.pcd")
    base_ms = []
    m = 0
    try:
        for it in range(a.warmup + a.reps):
            reg.assembleMap(ma.submaps, None, out=raw)
            t_asm = reg._getf(capi.MAP_ASSEMBLY_MS)
            t0 = time.perf_counter()
            got, _ = reg.assembleMap(ma.submaps, None, out=thin, leaf=a.leaf)
            t1 = time.perf_counter()
            m = int(got.shape[0])
            t_leg = [reg._getf(capi.MAP_FILTER_BBOX_MS + k) for k in range(len(LEGS))]
            if it >= a.warmup:
                asm_ms.append(t_asm)
                whole_ms.append((t1 - t0) * 1e3)
                for k, name_k in enumerate(LEGS):
                    legs[name_k].append(t_leg[k])
            # the files: fewer repetitions (the unfiltered text of a map is hundreds of megabytes)
            if it < a.warmup + a.save_reps:
                for kind in KINDS:
                    for filtered in (False, True):
                        if os.path.exists(path):
                            os.remove(path)
                        t0 = time.perf_counter()
                        size[(kind, filtered)] = ma.save_map(reg, path, None, data=kind, leaf=a.leaf if filtered else None)
                        t1 = time.perf_counter()
                        if it >= min(a.warmup, 1):
                            save[(kind, filtered)].append((t1 - t0) * 1e3)
            if baseline and it >= a.warmup:
                t0 = time.perf_counter()
                host_raw, _ = reg.assembleMap(ma.submaps, None, out=np.empty((n, 32), np.uint8))
                old = reg.voxelGridFilterPointCloud2(host_raw.reshape(-1), n, 32, (0, 4, 8, 16), a.leaf)
                t1 = time.perf_counter()
                base_ms.append((t1 - t0) * 1e3)
                if it == a.warmup:
                    row["baseline_same_bytes"] = bool(np.array_equal(old, got.cpu().numpy()))
    finally:
        if os.path.exists(path):
            os.remove(path)
    bits = reg.mapFilterKeyBits()
    row.update(kept=m, kept_ratio=m / n, key_bits=bits, assemble_ms=_stats(asm_ms), assemble_filtered_wall_ms=_stats(whole_ms),
               legs_ms={k: _stats(v) for k, v in legs.items()})
    row["launch_sum_ms"] = sum(row["legs_ms"][k]["median"] for k in LEGS) + row["assemble_ms"]["median"]
    moved = dict(key=key_bytes(n, bits > 32), sort=sort_bytes(n, bits), centroid=centroid_bytes(n, m, bits > 32))
    row["bytes"] = moved
    row["bytes_per_s"] = {k: moved[k] / (row["legs_ms"][k]["median"] * 1e-3) for k in moved}
    row["share_of_hbm_peak"] = {k: row["bytes_per_s"][k] / HBM_PEAK for k in moved}
    row["save"] = {f"{kind}{'_filtered' if f else ''}": dict(ms=_stats(save[(kind, f)]), bytes=int(size[(kind, f)])) for kind in KINDS for f in (False, True)}
    if baseline:
        row["baseline_host_route_ms"] = _stats(base_ms)
    return row


def table(rows, a):
    out = ["# Thinning the whole map on the device: measured legs", "",
           f"`python tools/map_filter_profile.py --keyframes {a.keyframes} --points {a.points} --leaf {a.leaf} --reps {a.reps} --warmup {a.warmup}` on one "
           "MI355X; times in ms as median (min – max, n).  hipEvent brackets (LSR_PROFILE) for the launches, the host clock around "
           "calls that return synchronised for the rest.  Files in " + ("/dev/shm" if a.dir.startswith("/dev/shm") else "a temporary directory") + ".", ""]
    for r in rows:
        out += [f"## {r['map']}: {r['keyframes']} keyframes, {r['records']:,} records, leaf {r['leaf']} m", "",
                f"Kept {r['kept']:,} of {r['records']:,} records (ratio {r['kept_ratio']:.4f}); leaf index of {r['key_bits']} bits.", "",
                "| leg | ms | bytes moved | bytes/s | share of the 8 TB/s HBM peak |", "|---|---|---|---|---|",
                f"| `lsr_assemble_map` alone (the launch) | {_fmt(r['assemble_ms'], 3)} | | | |"]
        for k in LEGS:
            if k in r["bytes"]:
                out.append(f"| {k} | {_fmt(r['legs_ms'][k], 3)} | {r['bytes'][k]:,} | {r['bytes_per_s'][k] / 1e12:.2f} TB/s | {100 * r['share_of_hbm_peak'][k]:.1f} % |")
            else:
                out.append(f"| {k} | {_fmt(r['legs_ms'][k], 3)} | | | |")
        out += [f"| the launches' sum (assemble + filter) | {r['launch_sum_ms']:.3f} | | | |",
                f"| `lsr_assemble_map_filtered`, the whole call (host clock) | {_fmt(r['assemble_filtered_wall_ms'])} | | | |"]
        if "baseline_host_route_ms" in r:
            out.append(f"| before: `lsr_assemble_map` to the host + `lsr_voxel_grid_filter_pc2` host in / host out (host clock; same bytes: "
                       f"{r.get('baseline_same_bytes')}) | {_fmt(r['baseline_host_route_ms'])} | | | |")
        out += ["", "| file | unfiltered ms | unfiltered bytes | filtered ms | filtered bytes |", "|---|---|---|---|---|"]
        for kind in KINDS:
            u, f = r["save"][kind], r["save"][kind + "_filtered"]
            out.append(f"| {kind} | {_fmt(u['ms'])} | {u['bytes']:,} | {_fmt(f['ms'])} | {f['bytes']:,} |")
        out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=628)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--leaf", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--save-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.keyframes < 8:
        ap.error("--keyframes must be at least 8")
    import numpy as np
    import torch

    from lidarslam_ros2_amd import NormalDistributionsTransform, _capi as capi

    if not torch.cuda.is_available():
        raise SystemExit("map_filter_profile.py measures on the GPU: none is visible")
    own_dir = None
    if a.dir is None:
        own_dir = tempfile.mkdtemp(prefix="map_filter_profile_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        a.dir = own_dir
    try:
        reg = NormalDistributionsTransform(device=0)
        reg.setProfiling(True)
        rows = [profile_map(a, "drive", reg, capi, torch, np, a.keyframes, 20.0, False),
                profile_map(a, "small drive (int32 index)", reg, capi, torch, np, max(8, a.keyframes // 4), 0.0, True)]
    finally:
        if own_dir:
            os.rmdir(own_dir)
    print(json.dumps(dict(tool="map_filter_profile", rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(table(rows, a) + "\n")


if __name__ == "__main__":
    main()

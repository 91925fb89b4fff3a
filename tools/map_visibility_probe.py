#!/usr/bin/env python3
"""Times the visibility votes (lsr_depth_images_build, lsr_visibility_votes, lsr_assemble_map_static; csrc/map_visibility.hip) on the
synthetic drive of tools/map_filter_profile.py with a car driving ahead of the vehicle.  A tool, not a test; not wired into bench.py.

    python tools/map_visibility_probe.py [--keyframes 628] [--points 20000] [--reps 7] [--warmup 2] [--out profiles/map_visibility.md]
    rocprofv3 --kernel-trace --pmc COUNTERS --output-format csv -d DIR/NAME -o p -- python tools/map_visibility_probe.py --once
    python tools/map_visibility_probe.py --counters DIR [--out ...]        (adds the counters of those runs to the table; needs no device)

The counter runs are runs of their own, one per set that fits the slots: FETCH_SIZE; WRITE_SIZE; SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES
SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY.

The drive: 628 keyframes of 20 000 pcl::PointXYZI records 1.5 m apart on a circle, resident in HBM (12.6 M records); the last 300
records of every keyframe are replaced by samples of the surfaces of a 4 x 1.8 x 1.5 m box 8 m ahead of the vehicle.  The drive's
clouds are random samples of a ground plane and two walls, not ray casts: what the votes REMOVE there says nothing (the behaviour of
the definition is tests/test_map_visibility_cpu.py's); the work per record is that of a real drive with the same neighbour counts.

Timed (median, min - max over --reps after --warmup; hipEvent brackets through LSR_PROFILE for the launches, the host clock around the
synchronised call for the rest): the image of one new keyframe and of all keyframes, with and without the erosion; the votes; the
static assembly; lsr_assemble_map over the same records (LSR_MAP_ASSEMBLY_MS), the yardstick of profiles/map_window.md; the numpy
restatement on the host over the first --numpy-keyframes keyframes.  Bytes: what the algorithm needs, from the shapes.  There is no
threshold."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_ACHIEVABLE = 6.3e12   # bytes/s a streaming kernel reaches on an MI355X (8 TB/s peak)
N_CAR = 300


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _fmt(s, digits=3):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f} – {s['max']:.{digits}f}, n = {s['n']})"


def add_car(np, clouds, seed):
    """The last N_CAR records of every cloud become samples of the faces of a box 8 m ahead (pose-local: +x is the heading)."""
    rng = np.random.default_rng(seed)
    for rec in clouds:
        u = rng.uniform(-0.5, 0.5, (N_CAR, 3)) * (4.0, 1.8, 1.5)
        face = rng.integers(0, 3, N_CAR)
        u[np.arange(N_CAR), face] = np.where(rng.random(N_CAR) < 0.5, -0.5, 0.5) * np.array([4.0, 1.8, 1.5])[face]
        rec[-N_CAR:, :3] = (u + (8.0, 0.0, -1.0)).astype(np.float32)


def counters(directory):
    """Sums of the rocprofv3 counters per kernel of this unit -> {kernel: {counter: (sum, launches)}}."""
    out = {}
    for f in sorted(glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                k = re.sub(r"\(anonymous namespace\)::|lsr::|^void |\(.*$", "", r["Kernel_Name"])
                if not (k.startswith("vis_") or k.startswith("assemble_map") or k.startswith("mw_scan")):
                    continue
                s, n = out.setdefault(k, {}).get(r["Counter_Name"], (0.0, 0))
                out[k][r["Counter_Name"]] = (s + float(r["Counter_Value"]), n + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=628)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--numpy-keyframes", type=int, default=24)
    ap.add_argument("--once", action="store_true", help="one pass of every leg and nothing else: the program a counter run wraps")
    ap.add_argument("--counters", default=None, help="directory of a rocprofv3 --pmc run of --once: summarised, no device needed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.counters:
        c = counters(a.counters)
        print(json.dumps(dict(tool="map_visibility_probe", counters=c)))
        if a.out:
            names = sorted({n for v in c.values() for n in v})
            lines = ["", "## Counters (runs of their own)", "",
                     "`rocprofv3 --kernel-trace --pmc ...` around `tools/map_visibility_probe.py --once` (one pass of every leg), one run per "
                     "counter set; sums over the launches of a kernel.  On gfx950 FETCH_SIZE counts half the bytes of a wide streaming read "
                     "and is uncalibrated for narrower ones: a ratio between kernels, not an absolute.  FETCH_SIZE and WRITE_SIZE in KB.", "",
                     "| kernel | launches | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
            for k in sorted(c):
                lines.append(f"| `{k}` | {max(v[1] for v in c[k].values())} | " + " | ".join(f"{c[k][n][0]:,.0f}" if n in c[k] else "" for n in names) + " |")
            with open(a.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    import numpy as np
    import torch

    import map_visibility_numpy as MV
    from lidarslam_ros2_amd import MapArray, NormalDistributionsTransform, VisibilityParams, _capi as capi, visibilityPairs
    from map_filter_profile import make_drive

    if not torch.cuda.is_available():
        raise SystemExit("map_visibility_probe.py measures on the GPU: none is visible")
    clouds, poses = make_drive(np, a.keyframes, a.points, 20.0, seed=a.keyframes)
    add_car(np, clouds, a.keyframes)
    ma = MapArray()
    for rec, P in zip(clouds, poses):
        ma.append(torch.from_numpy(rec).cuda(), P, 0.0)
    subs = ma.submaps
    n, nk = a.keyframes * a.points, a.keyframes
    p = VisibilityParams()
    H, W4 = p.shape
    first_pair, other, _ = visibilityPairs(subs, None, p)
    n_pairs = int(other.size)
    pair_records = int(sum((int(first_pair[i + 1]) - int(first_pair[i])) * a.points for i in range(nk)))
    reg = NormalDistributionsTransform(device=0)
    reg.setProfiling(True)
    table = torch.empty((nk, H, W4), dtype=torch.float32, device="cuda")
    raw = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    T = {k: [] for k in ("one_ms", "one_call", "all_raw_ms", "all_ms", "all_call", "votes_ms", "votes_call", "static_ms", "static_call", "asm_ms")}
    kept = removed = 0
    reps = 1 if a.once else a.warmup + a.reps

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3

    for it in range(reps):
        _, t = clock(lambda: reg.depthImages(subs[-1:], p, out=table[-1:]))
        row = dict(one_ms=reg.visibilityMs()[0], one_call=t)
        reg.depthImages(subs, p, out=table, eroded=False)
        row["all_raw_ms"] = reg.visibilityMs()[0]
        _, t = clock(lambda: reg.depthImages(subs, p, out=table))
        row.update(all_ms=reg.visibilityMs()[0], all_call=t)
        (votes, _), t = clock(lambda: reg.visibilityVotes(subs, table, p, device_out=True))
        row.update(votes_ms=reg.visibilityMs()[1], votes_call=t)
        (rec, first, removed), t = clock(lambda: reg.assembleMapStatic(subs, table, p, out=out))
        kept = int(rec.shape[0])
        row.update(static_ms=reg.visibilityMs()[1], static_call=t)
        reg.assembleMap(subs, None, out=raw)
        row["asm_ms"] = reg._getf(capi.MAP_ASSEMBLY_MS)
        if a.once or it >= a.warmup:
            for k, v in row.items():
                T[k].append(v)
    vhist = torch.bincount(votes.to(torch.int64).clamp(max=8), minlength=9).cpu().tolist()
    # the restatement on the host, over the first keyframes and the pairs among them
    m = min(a.numpy_keyframes, nk)
    host = [c for c in clouds[:m]]
    t0 = time.perf_counter()
    E = MV.images(host, p)
    t_img = (time.perf_counter() - t0) * 1e3
    fp, ot, rl = visibilityPairs(subs[:m], None, p)
    t0 = time.perf_counter()
    ref = MV.votes(host, fp, ot, rl, E, p)
    t_votes = (time.perf_counter() - t0) * 1e3
    sub_votes, _ = reg.visibilityVotes(subs[:m], table[:m], p)
    same = bool(np.array_equal(sub_votes, ref)) and bool(np.array_equal(table[:m].cpu().numpy().view(np.uint32), E.view(np.uint32)))
    np_pair_records = int(ot.size) * a.points

    S = {k: _stats(v) for k, v in T.items()}
    img_bytes = n * 32 + 3 * nk * H * W4 * 4            # records read; the image filled, lowered in place (L2), read and written by the erosion
    votes_bytes = n * 32 + pair_records * 4 + n * 4   # records read, one pixel gathered per pair, votes written
    static_bytes = votes_bytes + 2 * n * 32 + 2 * n * 4 + n * 32 + kept * 32   # + the raw map written, the votes read twice, the raw map read, the kept records written
    asm_bytes = 2 * n * 32
    row = dict(records=n, keyframes=nk, pairs=n_pairs, pair_records=pair_records, kept=kept, removed=removed, vote_histogram=vhist, **S,
               image_bytes=img_bytes, votes_bytes=votes_bytes, static_bytes=static_bytes, assemble_bytes=asm_bytes,
               numpy=dict(keyframes=m, pair_records=np_pair_records, images_ms=t_img, votes_ms=t_votes, same_bits=same))
    print(json.dumps(dict(tool="map_visibility_probe", row=row)))
    if a.out and not a.once:
        def rate(b, ms):
            return f"{b / (ms * 1e-3) / 1e12:.2f} TB/s ({100 * b / (ms * 1e-3) / HBM_ACHIEVABLE:.0f} % of 6.3 TB/s)"

        dev_rate = pair_records / (S["votes_ms"]["median"] * 1e-3)
        np_rate = np_pair_records / (t_votes * 1e-3) if t_votes > 0 else float("nan")
        lines = ["# Moving objects out of the map: what the visibility votes cost, measured", "",
                 f"`python tools/map_visibility_probe.py --keyframes {nk} --points {a.points} --reps {a.reps} --warmup {a.warmup}` on one MI355X, one "
                 "session; times in ms as median (min – max, n).  hipEvent brackets (LSR_PROFILE) for the launches, the host clock around "
                 "calls that return synchronised for the rest.", "",
                 f"The map: the synthetic drive of `profiles/map_filter.md` with a car 8 m ahead in every keyframe, {n:,} pcl::PointXYZI records "
                 f"in {nk} keyframes resident in HBM.  Defaults: images of {H} x {W4}, keyframe_range 30 m, max_neighbours 32: {n_pairs:,} "
                 f"(keyframe, neighbour) pairs, {pair_records:,} (record, neighbour) tests.  The static map keeps {kept:,} records and leaves "
                 f"out {removed:,}; votes per record (0, 1, .. 7, 8+): {vhist}.  (The drive's clouds are random samples, not ray casts: the "
                 "count says nothing about the definition, see `tests/test_map_visibility_cpu.py` for that.)", "",
                 "| leg | launches, ms | whole call, ms | bytes needed | bytes/s of the launches |", "|---|---|---|---|---|",
                 f"| image of ONE new keyframe, eroded (`LSR_DEPTH_IMAGES_MS`) | {_fmt(S['one_ms'])} | {_fmt(S['one_call'])} | {a.points * 32 + 3 * H * W4 * 4:,} | launch bound |",
                 f"| images of all keyframes, not eroded | {_fmt(S['all_raw_ms'])} | | {n * 32 + nk * H * W4 * 4:,} | {rate(n * 32 + nk * H * W4 * 4, S['all_raw_ms']['median'])} |",
                 f"| images of all keyframes, eroded | {_fmt(S['all_ms'])} | {_fmt(S['all_call'])} | {img_bytes:,} | {rate(img_bytes, S['all_ms']['median'])} |",
                 f"| the erosion alone (the difference of the two medians) | {S['all_ms']['median'] - S['all_raw_ms']['median']:.3f} | | {2 * nk * H * W4 * 4:,} | |",
                 f"| votes (`LSR_VISIBILITY_MS`) | {_fmt(S['votes_ms'])} | {_fmt(S['votes_call'])} | {votes_bytes:,} | {rate(votes_bytes, S['votes_ms']['median'])} |",
                 f"| static assembly: votes, count, scan, write (`LSR_VISIBILITY_MS`; the raw map's launch is the next row) | {_fmt(S['static_ms'])} | {_fmt(S['static_call'])} | {static_bytes:,} | |",
                 f"| yardstick: `lsr_assemble_map`, the same records (`LSR_MAP_ASSEMBLY_MS`) | {_fmt(S['asm_ms'])} | | {asm_bytes:,} | {rate(asm_bytes, S['asm_ms']['median'])} |", "",
                 f"The votes take {S['votes_ms']['median'] / S['asm_ms']['median']:.2f} x, the static assembly's own launches "
                 f"{S['static_ms']['median'] / S['asm_ms']['median']:.2f} x and the whole static call "
                 f"{S['static_call']['median'] / S['asm_ms']['median']:.2f} x the assembly launch's time.  The votes make "
                 f"{dev_rate / 1e9:.1f} G (record, neighbour) tests per second.", "",
                 f"The numpy restatement on the host (`tests/map_visibility_numpy.py`), first {m} keyframes and the pairs among them: images "
                 f"{t_img:.1f} ms, votes {t_votes:.1f} ms for {np_pair_records:,} tests = {np_rate / 1e6:.1f} M tests per second — the device is "
                 f"{dev_rate / np_rate:,.0f} x faster per test.  Device and restatement agree bit for bit on those keyframes (images and votes): {same}.", ""]
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    main()

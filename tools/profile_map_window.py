#!/usr/bin/env python3
"""Times localising in a saved map (lsr_crop_map, lsr_set_input_target_window; csrc/map_window.hip) on the synthetic drive of
tools/map_filter_profile.py.  A tool, not a test; it is not wired into bench.py.

    python tools/profile_map_window.py [--keyframes 628] [--points 20000] [--reps 7] [--warmup 2] [--out profiles/map_window.md]

The map: that drive's 628 keyframes of 20 000 pcl::PointXYZI records assembled once (lsr_assemble_map, whose hipEvent time is taken
in the same run: LSR_MAP_ASSEMBLY_MS), 12.6 M records resident in HBM, 400 m x 400 m x 53 m.  The pose: keyframe 0's.  The window:
mapWindowAround(t, reach + slack, 1.0) with reach (50, 50, 10) m — the drive's scans reach 50 m — and slack (20, 20, 10) m.  The scans:
the pose-local records of keyframes 0 .. 7, each registered from the pose of the keyframe before it.

Timed (median, min - max over --reps after --warmup, the arms interleaved in one run): the cut (LSR_MAP_WINDOW_MS, hipEvents, beside
LSR_MAP_ASSEMBLY_MS for the same records); cut + target build (setInputTargetWindow, host clock: the call returns synchronised);
align per scan against the window and against the WHOLE map set as target with lsr_set_input_target_device — the arm that exists
without this code, the baseline; the table mode each arm's passes ran in (LSR_DEBUG_TABLE) and the bytes of cell_slot each reserved.
Bytes of the cut: the count reads every record, the write reads every record again and writes the kept ones.  Prints one JSON line and
writes the table.  There is no threshold."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

TABLE_MODES = {0: "dense global table", 1: "compact global table", 2: "table staged in LDS"}


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _fmt(s, digits=3):
    return f"{s['median']:.{digits}f} ({s['min']:.{digits}f} – {s['max']:.{digits}f}, n = {s['n']})"


def _stderr_of(fn):
    """fn() with the process's stderr (the library's own diagnostics included) captured -> (result, text)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode(errors="replace")


def _cell_slot_bytes(info):
    div = [int(b) - int(a) + 1 for a, b in zip(info["min_b"], info["max_b"])]
    return 4 * div[0] * div[1] * div[2], div


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=628)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.warmup < 1:
        ap.error("--warmup must be at least 1 (the first align of each arm runs with stderr captured, for its table mode)")
    os.environ["LSR_DEBUG_TABLE"] = "1"
    import numpy as np
    import torch

    from lidarslam_ros2_amd import MapArray, NormalDistributionsTransform, _capi as capi, mapWindowAround
    from map_filter_profile import make_drive

    if not torch.cuda.is_available():
        raise SystemExit("profile_map_window.py measures on the GPU: none is visible")
    clouds, poses = make_drive(np, a.keyframes, a.points, 20.0, seed=a.keyframes)
    ma = MapArray()
    for rec, P in zip(clouds, poses):
        ma.append(torch.from_numpy(rec).cuda(), P, 0.0)
    n = a.keyframes * a.points
    raw = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    reach, slack = (50.0, 50.0, 10.0), (20.0, 20.0, 10.0)
    w = mapWindowAround(poses[0][:3, 3], np.add(reach, slack), 1.0)

    def ndt():
        r = NormalDistributionsTransform(device=0)
        r.setResolution(1.0)
        r.setMaximumIterations(30)
        r.setTransformationEpsilon(0.01)
        return r

    tool, win, whole = ndt(), ndt(), ndt()
    tool.setProfiling(True)
    win.setProfiling(True)
    cut_buf = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    scans = [torch.from_numpy(np.ascontiguousarray(clouds[k][:, :3])).cuda() for k in range(a.scans)]
    guesses = [poses[max(k - 1, 0)].astype(np.float32) for k in range(a.scans)]
    asm_ms, cut_ms, target_ms, whole_target_ms = [], [], [], []
    align_ms = {"window": [], "whole": []}
    modes, iters, same = {}, {"window": [], "whole": []}, True
    kept = 0
    for it in range(a.warmup + a.reps):
        tool.assembleMap(ma.submaps, None, out=raw)
        t_asm = tool._getf(capi.MAP_ASSEMBLY_MS)
        kept = int(tool.cropMap(raw, w, out=cut_buf).shape[0])
        t_cut = tool.mapWindowMs()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        win.setInputTargetWindow(raw, w)
        t1 = time.perf_counter()
        whole.setInputTarget(raw.view(torch.float32))
        t2 = time.perf_counter()
        finals, per = {"window": [], "whole": []}, {"window": [], "whole": []}
        for k, (s, g) in enumerate(zip(scans, guesses)):          # the arms take turns scan by scan
            for name, r in (("window", win), ("whole", whole)):
                r.setInputSource(s)
                ta = time.perf_counter()
                if name not in modes:                             # (the library reports the mode of a process's first aligns only)
                    _, text = _stderr_of(lambda: r.align(g))
                    m = re.search(r"table mode (\d+)", text)
                    modes[name] = int(m.group(1)) if m else -1
                else:
                    r.align(g)
                per[name].append((time.perf_counter() - ta) * 1e3)
                finals[name].append((r.getFinalTransformation(), r.getFinalNumIteration()))
        if it >= a.warmup:
            for name in per:
                align_ms[name] += per[name]
        same = same and all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(finals["window"], finals["whole"]))
        iters = {k: [f[1] for f in v] for k, v in finals.items()}
        if it >= a.warmup:
            asm_ms.append(t_asm)
            cut_ms.append(t_cut)
            target_ms.append((t1 - t0) * 1e3)
            whole_target_ms.append((t2 - t1) * 1e3)
    cut_bytes = 2 * n * 32 + kept * 32
    asm_bytes = 2 * n * 32
    slot = {name: _cell_slot_bytes(r.gridInfo()) for name, r in (("window", win), ("whole", whole))}
    row = dict(records=n, kept=kept, window=dict(leaf=w.leaf, lo=w.lo, hi=w.hi), assemble_ms=_stats(asm_ms), cut_ms=_stats(cut_ms),
               cut_bytes=cut_bytes, assemble_bytes=asm_bytes, cut_target_ms=_stats(target_ms), whole_target_ms=_stats(whole_target_ms),
               align_ms={k: _stats(v) for k, v in align_ms.items()}, table_mode=modes, iterations=iters, same_bits=bool(same),
               cell_slot_bytes={k: v[0] for k, v in slot.items()}, grid_cells={k: v[1] for k, v in slot.items()})
    row["cut_bytes_per_s"] = cut_bytes / (row["cut_ms"]["median"] * 1e-3)
    row["assemble_bytes_per_s"] = asm_bytes / (row["assemble_ms"]["median"] * 1e-3)
    row["cut_over_assemble"] = row["cut_ms"]["median"] / row["assemble_ms"]["median"]
    print(json.dumps(dict(tool="profile_map_window", row=row)))
    if a.out:
        r = row
        lines = ["# Localising in a saved map: the cut and what it buys, measured", "",
                 f"`python tools/profile_map_window.py --keyframes {a.keyframes} --points {a.points} --reps {a.reps} --warmup {a.warmup}` on one MI355X, "
                 "one session; times in ms as median (min – max, n).  hipEvent brackets (LSR_PROFILE) for the launches, the host clock "
                 "around calls that return synchronised for the rest.", "",
                 f"The map: the synthetic drive of `profiles/map_filter.md`, {n:,} pcl::PointXYZI records resident in HBM.  The window: "
                 f"leaf {w.leaf}, cells {w.lo} .. {w.hi} (reach {reach} + slack {slack} m around keyframe 0's pose); it keeps {kept:,} records.", "",
                 "| leg | ms | bytes moved | bytes/s |", "|---|---|---|---|",
                 f"| `lsr_assemble_map`, wide form, the same records (`LSR_MAP_ASSEMBLY_MS`) | {_fmt(r['assemble_ms'])} | {asm_bytes:,} | {r['assemble_bytes_per_s'] / 1e12:.2f} TB/s |",
                 f"| the cut: count, scan, write (`LSR_MAP_WINDOW_MS`) | {_fmt(r['cut_ms'])} | {cut_bytes:,} | {r['cut_bytes_per_s'] / 1e12:.2f} TB/s |",
                 f"| cut + target build (`lsr_set_input_target_window`, host clock) | {_fmt(r['cut_target_ms'])} | | |",
                 f"| baseline: the whole map as target (`lsr_set_input_target_device`, host clock) | {_fmt(r['whole_target_ms'])} | | |", "",
                 f"The cut takes {r['cut_over_assemble']:.2f} x the assembly launch's time"
                 + (" — more than twice: slower than the expectation the feature was planned on." if r["cut_over_assemble"] > 2 else ".")
                 + "  Bytes of the cut: every record read by the count and again by the write, the kept ones written; of the assembly: every record read and written.", "",
                 "| arm | `align` per scan, host clock | table mode of its passes | `cell_slot` reserved | grid cells |", "|---|---|---|---|---|"]
        for name, label in (("window", "window target"), ("whole", "whole map as target (baseline)")):
            lines.append(f"| {label} | {_fmt(r['align_ms'][name])} | {TABLE_MODES.get(modes.get(name, -1), 'not reported')} | "
                         f"{r['cell_slot_bytes'][name]:,} bytes | {' x '.join(str(v) for v in r['grid_cells'][name])} |")
        lines += ["", f"Iterations per scan: window {iters['window']}, whole map {iters['whole']}; final transformations and iteration counts "
                  f"of the two arms equal bit for bit in every repetition: {same}.", ""]
        with open(a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""map.pcd from the device (lsr_format_pcd_ascii / lsr_save_pcd_ascii / lsr_save_map_pcd_ascii) against the machine, on
a synthetic map of `--submaps` x `--records` pcl::PointXYZI records (default 250 x 40 000 = 1e7).  Standalone: reads nothing outside
the repository, generates its data from a seed.

    python tools/pcd_probe.py [--out profiles/pcd_ascii.md] [--submaps 250] [--records 40000] [--reps 7] [--dir DIR]

The parent starts every step as a fresh child process under its own `timeout`, checks the exit status and starts nothing more after a
failure.  Steps (one JSON row each, times in ms, median / min / max of `reps` after `warmup`):
  format    device in, device out: the hipEvent brackets of the launches (LSR_PROFILE, LSR_PCD_FORMAT_MS) — the length pass + scan
            alone (a size query) and all three launches; text GB/s against HBM
  parts     the three stages of a save one after the other, each timed on its own: format (device to device, host clock), the text
            copied to pinned host memory, the text written to a file with one fwrite-sized write
  save      lsr_save_pcd_ascii from the resident map and lsr_save_map_pcd_ascii from the resident submaps, host clock around the call,
            to a file in `--dir` (default: /dev/shm when there is one, else the temporary directory) and to /dev/null
  baseline  the loop of a host ASCII writer as PCL runs it (one ostringstream of precision 8, a trim per line), compiled from
            tools/pcd_host_emu/harness.cpp, on the same records on this machine, to the same directory
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_TIMEOUT = {"format": 240, "parts": 240, "save": 420, "baseline": 420}
STEPS = ("format", "parts", "save", "baseline")


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _records(n_submaps, n_records):
    """(n, 8) float32, the same on every call: coordinates of a few hundred metres, intensities 0 .. 255, padding words zero."""
    import numpy as np

    rng = np.random.default_rng(7)
    n = n_submaps * n_records
    rec = np.zeros((n, 8), np.float32)
    rec[:, 0:3] = rng.uniform(-300.0, 300.0, (n, 3)).astype(np.float32)
    rec[:, 2] *= np.float32(0.05)
    rec[:, 4] = rng.integers(0, 256, n).astype(np.float32)
    return rec


def _setup(a):
    import numpy as np
    import torch

    from lidarslam_ros2_amd import NormalDistributionsTransform, SubMap, _capi

    if not torch.cuda.is_available():
        raise SystemExit("pcd_probe: no GPU visible (there is no CPU path to time)")
    reg = NormalDistributionsTransform(device=0)
    reg.setProfiling(True)
    rec = _records(a.submaps, a.records)
    d_rec = torch.from_numpy(rec).cuda()
    rng = np.random.default_rng(8)
    submaps = []
    for i in range(a.submaps):
        q = rng.normal(size=4) * [0.05, 0.05, 1.0, 1.0]
        submaps.append(SubMap(d_rec[i * a.records:(i + 1) * a.records], tuple(rng.uniform(-200, 200, 3)), tuple(q / np.linalg.norm(q)), float(i)))
    torch.cuda.synchronize()
    return torch, reg, rec, d_rec, submaps, _capi


def step_format(a):
    torch, reg, rec, d_rec, submaps, capi = _setup(a)
    lay = reg._layout(32, (0, 4, 8, 16))
    size = C.c_size_t()
    out = None
    length_ms, all_ms = [], []
    for it in range(a.warmup + a.reps):
        capi.check(reg._lib.lsr_format_pcd_ascii(reg._h, C.c_void_p(d_rec.data_ptr()), len(rec), C.byref(lay), 1, None, 0, 0, C.byref(size)), "size")
        t_len = reg._getf(capi.PCD_FORMAT_MS)
        if out is None:
            out = torch.empty(size.value, dtype=torch.uint8, device="cuda")
        reg.formatPCDASCII(d_rec, out=out)
        t_all = reg._getf(capi.PCD_FORMAT_MS)
        if it >= a.warmup:
            length_ms.append(t_len); all_ms.append(t_all)
    L, A = _stats(length_ms), _stats(all_ms)
    return dict(step="format", records=len(rec), text_bytes=size.value, length_and_scan_ms=L, three_launches_ms=A,
                write_pass_ms=A["median"] - L["median"], text_GBps=size.value / 1e9 / (A["median"] * 1e-3),
                records_per_s=len(rec) / (A["median"] * 1e-3))


def step_parts(a):
    torch, reg, rec, d_rec, submaps, capi = _setup(a)
    out = reg.formatPCDASCII(d_rec)
    pinned = torch.empty(out.numel(), dtype=torch.uint8).pin_memory()
    path = os.path.join(a.dir, "pcd_probe_parts.pcd")
    fmt, cp, wr = [], [], []
    try:
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            reg.formatPCDASCII(d_rec, out=out)
            t1 = time.perf_counter()
            pinned.copy_(out, non_blocking=True)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            with open(path, "wb") as f:
                f.write(memoryview(pinned.numpy()))
            t3 = time.perf_counter()
            if it >= a.warmup:
                fmt.append((t1 - t0) * 1e3); cp.append((t2 - t1) * 1e3); wr.append((t3 - t2) * 1e3)
    finally:
        if os.path.exists(path):
            os.remove(path)
    F, Cp, W = _stats(fmt), _stats(cp), _stats(wr)
    gb = out.numel() / 1e9
    return dict(step="parts", dir=a.dir, text_bytes=out.numel(), format_call_ms=F, copy_to_pinned_ms=Cp, file_write_ms=W,
                sum_of_medians_ms=F["median"] + Cp["median"] + W["median"], copy_GBps=gb / (Cp["median"] * 1e-3),
                file_write_GBps=gb / (W["median"] * 1e-3))


def step_save(a):
    torch, reg, rec, d_rec, submaps, capi = _setup(a)
    path = os.path.join(a.dir, "pcd_probe_save.pcd")
    rows = {"save_file": [], "save_null": [], "save_map_file": [], "save_map_null": []}
    fmt_ms = []
    size = map_size = 0
    try:
        for it in range(a.warmup + a.reps):
            for name, target in (("file", path), ("null", "/dev/null")):
                t0 = time.perf_counter()
                size = reg.savePCDFileASCII(target, d_rec)
                t1 = time.perf_counter()
                if name == "file":
                    fmt_ms.append(reg._getf(capi.PCD_FORMAT_MS))
                t2 = time.perf_counter()
                map_size = reg.saveMapPCDFileASCII(target, submaps)
                t3 = time.perf_counter()
                if it >= a.warmup:
                    rows["save_" + name].append((t1 - t0) * 1e3); rows["save_map_" + name].append((t3 - t2) * 1e3)
    finally:
        if os.path.exists(path):
            os.remove(path)
    r = {k + "_ms": _stats(v) for k, v in rows.items()}
    return dict(step="save", dir=a.dir, piece_records=reg.pcdPieceRecords(), text_bytes=size, map_text_bytes=map_size,
                format_launches_ms=_stats(fmt_ms[a.warmup:]), save_file_GBps=size / 1e9 / (r["save_file_ms"]["median"] * 1e-3), **r)


def step_baseline(a):
    import numpy as np

    rec = _records(a.submaps, a.records)
    with tempfile.TemporaryDirectory() as d:
        lib_path = os.path.join(d, "libpcdemu.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib_path, os.path.join(ROOT, "tools", "pcd_host_emu", "harness.cpp")])
        lib = C.CDLL(lib_path)
        lib.emu_host_writer_loop.restype = C.c_longlong
        lib.emu_host_writer_loop.argtypes = [C.c_char_p, C.c_void_p, C.c_longlong, C.c_int, C.POINTER(C.c_int), C.c_int]
        offs = (C.c_int * 4)(0, 4, 8, 16)
        rows = {"file": [], "null": []}
        path = os.path.join(a.dir, "pcd_probe_baseline.pcd")
        nbytes = 0
        try:
            for it in range(1 + max(2, a.reps // 3)):
                for name, target in (("file", path), ("null", "/dev/null")):
                    t0 = time.perf_counter()
                    nbytes = lib.emu_host_writer_loop(os.fsencode(target), C.c_void_p(rec.ctypes.data), len(rec), 32, offs, 4)
                    dt = (time.perf_counter() - t0) * 1e3
                    if nbytes <= 0:
                        raise SystemExit("the host writer loop failed")
                    if it >= 1:
                        rows[name].append(dt)
        finally:
            if os.path.exists(path):
                os.remove(path)
    return dict(step="baseline", dir=a.dir, records=len(rec), body_bytes=int(nbytes), host_loop_file_ms=_stats(rows["file"]),
                host_loop_null_ms=_stats(rows["null"]))


def _ms(s):
    return f"{s['median']:.2f} ({s['min']:.2f} – {s['max']:.2f}, n = {s['n']})"


def write_markdown(rows, path, a):
    by = {r["step"]: r for r in rows}
    out = ["# map.pcd from the device: `tools/pcd_probe.py`", "",
           f"Synthetic map of {a.submaps} submaps x {a.records} pcl::PointXYZI records; times in ms as median (min – max, n) after warm-up.", ""]
    if "format" in by:
        r = by["format"]
        out += ["## Formatting, device to device (hipEvent brackets, LSR_PCD_FORMAT_MS)", "",
                "| records | text bytes | length pass + scan | all three launches | write pass (difference of medians) | text GB/s | records/s |",
                "|---|---|---|---|---|---|---|",
                f"| {r['records']} | {r['text_bytes']} | {_ms(r['length_and_scan_ms'])} | {_ms(r['three_launches_ms'])} | {r['write_pass_ms']:.2f} | "
                f"{r['text_GBps']:.1f} | {r['records_per_s']:.3g} |", ""]
    if "parts" in by:
        r = by["parts"]
        out += [f"## The stages of a save one after the other (files in `{r['dir']}`)", "",
                "| format call (host clock) | text to pinned memory | file write | sum of medians | copy GB/s | file write GB/s |", "|---|---|---|---|---|---|",
                f"| {_ms(r['format_call_ms'])} | {_ms(r['copy_to_pinned_ms'])} | {_ms(r['file_write_ms'])} | {r['sum_of_medians_ms']:.1f} | "
                f"{r['copy_GBps']:.1f} | {r['file_write_GBps']:.2f} |", ""]
    if "save" in by:
        r = by["save"]
        out += [f"## The pipelined save (pieces of {r['piece_records']} records; host clock around the call)", "",
                "| call | to a file | to /dev/null |", "|---|---|---|",
                f"| lsr_save_pcd_ascii (resident map) | {_ms(r['save_file_ms'])} | {_ms(r['save_null_ms'])} |",
                f"| lsr_save_map_pcd_ascii (resident submaps) | {_ms(r['save_map_file_ms'])} | {_ms(r['save_map_null_ms'])} |", "",
                f"Formatting launches inside the save: {_ms(r['format_launches_ms'])}; file rate {r['save_file_GBps']:.2f} GB/s of text.", ""]
    if "baseline" in by:
        r = by["baseline"]
        out += ["## Host baseline: the PCL writer's loop restated (one ostringstream, precision 8, a trim per line)", "",
                "| to a file | to /dev/null |", "|---|---|", f"| {_ms(r['host_loop_file_ms'])} | {_ms(r['host_loop_null_ms'])} |", ""]
    if "save" in by and "baseline" in by:
        s, b = by["save"], by["baseline"]
        out += [f"Save from the resident map against the host loop, files: {b['host_loop_file_ms']['median'] / s['save_file_ms']['median']:.1f}x; "
                f"whole `do_save_map` line (assembly included) against the host loop alone: "
                f"{b['host_loop_file_ms']['median'] / s['save_map_file_ms']['median']:.1f}x.", ""]
    if "save" in by and "parts" in by:
        out += [f"Pipelined save {by['save']['save_file_ms']['median']:.1f} ms against format + copy + write measured separately "
                f"{by['parts']['sum_of_medians_ms']:.1f} ms.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_ascii.md"))
    ap.add_argument("--submaps", type=int, default=250)
    ap.add_argument("--records", type=int, default=40000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir())
    ap.add_argument("--step", choices=STEPS, help="(child) run one step in this process and print its row")
    a = ap.parse_args()
    if a.step:
        fn = {"format": step_format, "parts": step_parts, "save": step_save, "baseline": step_baseline}[a.step]
        print("ROW " + json.dumps(fn(a)), flush=True)
        return 0
    rows = []
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--submaps",
               str(a.submaps), "--records", str(a.records), "--reps", str(a.reps), "--warmup", str(a.warmup), "--dir", a.dir]
        p = subprocess.run(cmd, capture_output=True, text=True)
        row = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not row:
            print(f"step {step} failed with status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            break
        rows.append(json.loads(row[0]))
        print(row[0], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write_markdown(rows, a.out, a)
    with open(os.path.splitext(a.out)[0] + "_rows.json", "w") as f:
        json.dump(rows, f, indent=1)
    return 0 if len(rows) == len(STEPS) else 1


if __name__ == "__main__":
    sys.exit(main())

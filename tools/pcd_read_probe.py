#!/usr/bin/env python3
"""Reading map.pcd on the device (lsr_decode_pcd / lsr_load_pcd / lsr_set_input_target_pcd) against the machine, on the synthetic map
tools/pcd_probe.py uses for the writer: `--submaps` x `--records` pcl::PointXYZI records (default 250 x 40 000 = 1e7), written as text by
the device formatter.  Standalone: reads nothing outside the repository, generates its data from a seed.

    python tools/pcd_read_probe.py [--out profiles/pcd_read.md] [--submaps 250] [--records 40000] [--reps 7] [--dir DIR]

The parent starts every step as a fresh child process under its own `timeout`, checks the exit status and starts nothing more after a
failure.  Steps (one JSON row each, times in ms, median / min / max of `reps` after `warmup`):
  decode    device image in, device records out: the hipEvent brackets of the four launches (LSR_PROFILE, LSR_PCD_PARSE_MS), the host
            clock around the call, and the writer's LSR_PCD_FORMAT_MS for the same records, for scale
  load      lsr_load_pcd into a device buffer and lsr_set_input_target_pcd, host clock around the call, from a file in `--dir`
            (default: /dev/shm when there is one, else the temporary directory) that was just written, i.e. from the page cache
  kernels   the decode step once more under `rocprofv3 --kernel-trace --stats`: the time of each of the four kernels
  baseline  strtof over every value of the same file's body, one after the other on one host thread (tools/pcd_read_host_emu)
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_TIMEOUT = {"decode": 240, "load": 420, "kernels": 420, "baseline": 420}
STEPS = ("decode", "load", "baseline", "kernels")


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _records(n_submaps, n_records):
    """(n, 8) float32, the same on every call and the same as tools/pcd_probe.py: coordinates of a few hundred metres, intensities
    0 .. 255, padding words zero."""
    import numpy as np

    rng = np.random.default_rng(7)
    n = n_submaps * n_records
    rec = np.zeros((n, 8), np.float32)
    rec[:, 0:3] = rng.uniform(-300.0, 300.0, (n, 3)).astype(np.float32)
    rec[:, 2] *= np.float32(0.05)
    rec[:, 4] = rng.integers(0, 256, n).astype(np.float32)
    return rec


def _setup(a):
    import torch

    from lidarslam_ros2_amd import NormalDistributionsTransform, _capi

    if not torch.cuda.is_available():
        raise SystemExit("pcd_read_probe: no GPU visible (there is no CPU path to time)")
    reg = NormalDistributionsTransform(device=0)
    reg.setProfiling(True)
    rec = _records(a.submaps, a.records)
    d_rec = torch.from_numpy(rec).cuda()
    torch.cuda.synchronize()
    return torch, reg, rec, d_rec, _capi


def step_decode(a):
    torch, reg, rec, d_rec, capi = _setup(a)
    text = reg.formatPCDASCII(d_rec)
    format_ms = reg._getf(capi.PCD_FORMAT_MS)
    lay = reg._layout(32, (0, 4, 8, 16))
    out = torch.empty((len(rec), 32), dtype=torch.uint8, device="cuda")
    n = C.c_size_t()
    parse_ms, call_ms = [], []
    for it in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        capi.check(reg._lib.lsr_decode_pcd(reg._h, C.c_void_p(text.data_ptr()), text.numel(), 1, C.c_void_p(out.data_ptr()), len(rec), C.byref(lay), 1,
                                           C.byref(n)), "decode")
        dt = (time.perf_counter() - t0) * 1e3
        if it >= a.warmup:
            parse_ms.append(reg._getf(capi.PCD_PARSE_MS)); call_ms.append(dt)
    # what came back is what "%.8g" kept: formatting it again gives the same text
    same = bool(torch.equal(reg.formatPCDASCII(out), text))
    P = _stats(parse_ms)
    return dict(step="decode", records=len(rec), text_bytes=text.numel(), four_launches_ms=P, call_ms=_stats(call_ms), writer_format_ms=format_ms,
                text_GBps=text.numel() / 1e9 / (P["median"] * 1e-3), records_per_s=len(rec) / (P["median"] * 1e-3),
                unresolved=reg.pcdUnresolvedTokens(), text_round_trip_equal=same)


def step_load(a):
    torch, reg, rec, d_rec, capi = _setup(a)
    path = os.path.join(a.dir, "pcd_read_probe.pcd")
    reg.setResolution(3.0)
    lay = reg._layout(32, (0, 4, 8, 16))
    out = torch.empty((len(rec), 32), dtype=torch.uint8, device="cuda")
    n = C.c_size_t()
    load_ms, target_ms, parse_ms, read_ms = [], [], [], []
    try:
        size = reg.savePCDFileASCII(path, d_rec)
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            capi.check(reg._lib.lsr_load_pcd(reg._h, os.fsencode(path), C.c_void_p(out.data_ptr()), len(rec), C.byref(lay), 1, C.byref(n)), "load")
            t1 = time.perf_counter()
            p = reg._getf(capi.PCD_PARSE_MS)
            t2 = time.perf_counter()
            reg.setInputTargetPCD(path)
            t3 = time.perf_counter()
            with open(path, "rb") as f:               # the file read alone, one thread, pieces of the same size into one buffer
                buf = bytearray(reg.pcdReadPieceBytes())
                t4 = time.perf_counter()
                while f.readinto(buf):
                    pass
                t5 = time.perf_counter()
            if it >= a.warmup:
                load_ms.append((t1 - t0) * 1e3); target_ms.append((t3 - t2) * 1e3); parse_ms.append(p); read_ms.append((t5 - t4) * 1e3)
    finally:
        if os.path.exists(path):
            os.remove(path)
    L = _stats(load_ms)
    return dict(step="load", dir=a.dir, piece_bytes=reg.pcdReadPieceBytes(), file_bytes=size, load_ms=L, set_input_target_pcd_ms=_stats(target_ms),
                launches_inside_load_ms=_stats(parse_ms), file_read_alone_ms=_stats(read_ms), load_GBps=size / 1e9 / (L["median"] * 1e-3))


def step_kernels(a):
    """(child of the rocprofv3 run) a few decodes, nothing printed but the row marker."""
    torch, reg, rec, d_rec, capi = _setup(a)
    text = reg.formatPCDASCII(d_rec)
    for _ in range(a.warmup + a.reps):
        reg.decodePCD(text)
    return dict(step="kernels_child", decodes=a.warmup + a.reps)


def run_kernels(a, base_cmd):
    d = tempfile.mkdtemp(prefix="pcd_read_probe_")
    try:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT["kernels"]), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t",
               "--"] + base_cmd + ["--step", "kernels_child"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not files:
            return p, None
        rows = []
        for r in csv.DictReader(open(files[0])):
            if "pcdr_" in r["Name"]:
                name = r["Name"].split("pcdr_")[1].split("(")[0]
                rows.append(dict(kernel="pcdr_" + name, calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3, min_us=int(r["MinNs"]) / 1e3,
                                 max_us=int(r["MaxNs"]) / 1e3))
        return p, dict(step="kernels", decodes=a.warmup + a.reps, kernels=sorted(rows, key=lambda r: r["kernel"]))
    finally:
        shutil.rmtree(d, ignore_errors=True)


def step_baseline(a):
    torch, reg, rec, d_rec, capi = _setup(a)
    path = os.path.join(a.dir, "pcd_read_probe_baseline.pcd")
    with tempfile.TemporaryDirectory() as d:
        lib_path = os.path.join(d, "libpcdreademu.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", lib_path, os.path.join(ROOT, "tools", "pcd_read_host_emu", "harness.cpp")])
        lib = C.CDLL(lib_path)
        lib.emu_host_strtof_loop.restype = C.c_longlong
        lib.emu_host_strtof_loop.argtypes = [C.c_char_p, C.POINTER(C.c_double)]
        ms, tokens = [], 0
        try:
            reg.savePCDFileASCII(path, d_rec)
            del reg, d_rec
            for it in range(1 + max(2, a.reps // 3)):
                s = C.c_double()
                t0 = time.perf_counter()
                tokens = lib.emu_host_strtof_loop(os.fsencode(path), C.byref(s))
                dt = (time.perf_counter() - t0) * 1e3
                if tokens <= 0:
                    raise SystemExit("the host strtof loop failed")
                if it >= 1:
                    ms.append(dt)
        finally:
            if os.path.exists(path):
                os.remove(path)
    return dict(step="baseline", dir=a.dir, values=int(tokens), host_strtof_loop_ms=_stats(ms))


def _ms(s):
    return f"{s['median']:.2f} ({s['min']:.2f} – {s['max']:.2f}, n = {s['n']})"


def write_markdown(rows, path, a):
    by = {r["step"]: r for r in rows}
    out = ["# Reading map.pcd on the device: `tools/pcd_read_probe.py`", "",
           f"Synthetic map of {a.submaps} submaps x {a.records} pcl::PointXYZI records, its text written by the device formatter; times in ms as "
           "median (min – max, n) after warm-up.", ""]
    if "decode" in by:
        r = by["decode"]
        out += ["## Decoding, device image to device records (hipEvent brackets, LSR_PCD_PARSE_MS)", "",
                "| records | text bytes | four launches | lsr_decode_pcd (host clock) | text GB/s | records/s | unresolved values | writer, LSR_PCD_FORMAT_MS |",
                "|---|---|---|---|---|---|---|---|",
                f"| {r['records']} | {r['text_bytes']} | {_ms(r['four_launches_ms'])} | {_ms(r['call_ms'])} | {r['text_GBps']:.1f} | {r['records_per_s']:.3g} | "
                f"{r['unresolved']} | {r['writer_format_ms']:.2f} |", "",
                f"The decoded records formatted again give the same text: {r['text_round_trip_equal']}.", ""]
    if "kernels" in by:
        r = by["kernels"]
        out += [f"## The kernels of a decode (`rocprofv3 --kernel-trace --stats`, {r['decodes']} decodes)", "", "| kernel | calls | avg us | min us | max us |",
                "|---|---|---|---|---|"]
        out += [f"| `{k['kernel']}` | {k['calls']} | {k['avg_us']:.1f} | {k['min_us']:.1f} | {k['max_us']:.1f} |" for k in r["kernels"]] + [""]
    if "load" in by:
        r = by["load"]
        out += [f"## From a file in the page cache (`{r['dir']}`, pieces of {r['piece_bytes']} bytes; host clock around the call)", "",
                "| file bytes | lsr_load_pcd to a device buffer | lsr_set_input_target_pcd | launches inside the load | the file read alone, one thread | load GB/s |",
                "|---|---|---|---|---|---|",
                f"| {r['file_bytes']} | {_ms(r['load_ms'])} | {_ms(r['set_input_target_pcd_ms'])} | {_ms(r['launches_inside_load_ms'])} | "
                f"{_ms(r['file_read_alone_ms'])} | {r['load_GBps']:.2f} |", ""]
    if "baseline" in by:
        r = by["baseline"]
        out += ["## Host baseline: strtof over every value of the same body, one thread", "", "| values | strtof loop |", "|---|---|",
                f"| {r['values']} | {_ms(r['host_strtof_loop_ms'])} |", ""]
    if "load" in by and "baseline" in by:
        out += [f"lsr_load_pcd against the host strtof loop alone: {by['baseline']['host_strtof_loop_ms']['median'] / by['load']['load_ms']['median']:.1f}x.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_read.md"))
    ap.add_argument("--submaps", type=int, default=250)
    ap.add_argument("--records", type=int, default=40000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir())
    ap.add_argument("--step", choices=STEPS + ("kernels_child",), help="(child) run one step in this process and print its row")
    a = ap.parse_args()
    if a.step:
        fn = {"decode": step_decode, "load": step_load, "kernels_child": step_kernels, "baseline": step_baseline}[a.step]
        print("ROW " + json.dumps(fn(a)), flush=True)
        return 0
    rows = []
    base = [sys.executable, os.path.abspath(__file__), "--submaps", str(a.submaps), "--records", str(a.records), "--reps", str(a.reps), "--warmup",
            str(a.warmup), "--dir", a.dir]
    for step in STEPS:
        if step == "kernels":
            p, row = run_kernels(a, base)
            row = [json.dumps(row)] if row else []
        else:
            p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT[step])] + base + ["--step", step], capture_output=True, text=True)
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

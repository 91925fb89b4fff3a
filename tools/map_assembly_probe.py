#!/usr/bin/env python3
"""Map assembly (lsr_assemble_map) against the machine: a device-to-device hipMemcpyAsync of the map's bytes is the
yardstick — the kernel reads and writes exactly the bytes the copy does, plus nine multiplies or adds per record and a scalar table
lookup per slice.  Standalone: reads nothing outside the repository, generates its data from a seed.

    python tools/map_assembly_probe.py [--out profiles/map_assembly_rows.json] [--submaps 300] [--records 33000] [--reps 25]

The parent starts every GPU step as a fresh child process under its own `timeout`, checks the exit status and starts nothing more
after a failure.  Steps (one JSON row each, times in ms, median / min / max of `reps` after `warmup`):
  device    in ONE process, alternating: hipMemcpyAsync D2D of total x 32 bytes (hipEvents on the stream); the wide form and the
            general form (the same records from base pointers moved off their 16-byte boundary: 4 bytes) on the same volume, device
            in, device out — the kernel's own hipEvent bracket (LSR_PROFILE, LSR_MAP_ASSEMBLY_MS)
  host_out  device in, HOST out: host clock around the whole call (the copy to pageable host memory over PCIe bounds it)
  append    one keyframe of `records` records appended to the resident map: the kernel's bracket and the host clock around the call
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_TIMEOUT = {"device": 240, "host_out": 240, "append": 120}


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _setup(n_submaps, n_records, shift=0):
    """-> (torch, stream, registration object on that stream, submaps over ONE resident buffer, output buffer)."""
    import numpy as np
    import torch

    from lidarslam_ros2_amd import NormalDistributionsTransform, SubMap, _capi

    if not torch.cuda.is_available():
        raise SystemExit("map_assembly_probe: no GPU visible (there is no CPU path to time)")
    stream = torch.cuda.Stream()
    reg = NormalDistributionsTransform(device=0, stream=stream.cuda_stream)
    reg.setProfiling(True)
    g = torch.Generator(device="cuda").manual_seed(7)
    nbytes = n_submaps * n_records * 32
    src = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    src[: nbytes].view(torch.float32).copy_((torch.rand(nbytes // 4, device="cuda", generator=g) - 0.5) * 120.0)
    if shift:
        src[shift: shift + nbytes] = src[: nbytes].clone()
    rng = np.random.default_rng(7)
    submaps = []
    for i in range(n_submaps):
        q = rng.normal(size=4)
        view = src[shift + i * n_records * 32: shift + (i + 1) * n_records * 32]
        submaps.append(SubMap(view, tuple(rng.uniform(-200, 200, 3)), tuple(q / np.linalg.norm(q)), float(i)))
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return torch, stream, reg, submaps, out, _capi


def step_device(a):
    torch, stream, reg, submaps, out, capi = _setup(a.submaps, a.records)
    _, _, reg_g, submaps_g, _, _ = _setup(a.submaps, a.records, shift=4)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nbytes = a.submaps * a.records * 32
    src_ptr = submaps[0].cloud.data_ptr()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = {"copy": [], "wide": [], "general": []}
    for it in range(a.warmup + a.reps):
        with torch.cuda.stream(stream):
            e0.record(stream)
            st = hip.hipMemcpyAsync(out.data_ptr(), src_ptr, nbytes, 3, C.c_void_p(stream.cuda_stream))   # 3 = hipMemcpyDeviceToDevice
            e1.record(stream)
            stream.synchronize()
            if st != 0:
                raise SystemExit(f"hipMemcpyAsync failed: {st}")
            t_copy = e0.elapsed_time(e1)
            reg.assembleMap(submaps, out=out)
            t_wide, form_w = reg._getf(capi.MAP_ASSEMBLY_MS), reg.mapAssemblyForm()
            reg_g.assembleMap(submaps_g, out=out)
            t_gen, form_g = reg_g._getf(capi.MAP_ASSEMBLY_MS), reg_g.mapAssemblyForm()
        if (form_w, form_g) != (1, 2):
            raise SystemExit(f"unexpected forms {form_w} {form_g}")
        if it >= a.warmup:
            rows["copy"].append(t_copy); rows["wide"].append(t_wide); rows["general"].append(t_gen)
    r = {k: _stats(v) for k, v in rows.items()}
    gb = 2 * nbytes / 1e9
    return dict(step="device", submaps=a.submaps, records_per_submap=a.records, map_bytes=nbytes, copy_ms=r["copy"], wide_ms=r["wide"],
                general_ms=r["general"], copy_GBps=gb / (r["copy"]["median"] * 1e-3), wide_GBps=gb / (r["wide"]["median"] * 1e-3),
                general_GBps=gb / (r["general"]["median"] * 1e-3), wide_over_copy=r["wide"]["median"] / r["copy"]["median"],
                general_over_copy=r["general"]["median"] / r["copy"]["median"])


def step_host_out(a):
    import numpy as np

    torch, stream, reg, submaps, _, capi = _setup(a.submaps, a.records)
    nbytes = a.submaps * a.records * 32
    host = np.zeros(nbytes, np.uint8)
    wall, kern = [], []
    for it in range(2 + max(3, a.reps // 5)):
        t0 = time.perf_counter()
        reg.assembleMap(submaps, out=host)
        dt = (time.perf_counter() - t0) * 1e3
        if it >= 2:
            wall.append(dt); kern.append(reg._getf(capi.MAP_ASSEMBLY_MS))
    w = _stats(wall)
    return dict(step="host_out", map_bytes=nbytes, call_wall_ms=w, kernel_ms=_stats(kern), host_GBps=nbytes / 1e9 / (w["median"] * 1e-3))


def step_append(a):
    torch, stream, reg, submaps, out, capi = _setup(a.submaps, a.records)
    reg.assembleMap(submaps[:-1], out=out)
    at = (a.submaps - 1) * a.records * 32
    wall, kern = [], []
    for it in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        reg.assembleMap(submaps[-1:], out=out[at:])
        dt = (time.perf_counter() - t0) * 1e3
        if it >= a.warmup:
            wall.append(dt); kern.append(reg._getf(capi.MAP_ASSEMBLY_MS))
    return dict(step="append", records=a.records, resident_records=(a.submaps - 1) * a.records, call_wall_ms=_stats(wall), kernel_ms=_stats(kern))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_assembly_rows.json"))
    ap.add_argument("--submaps", type=int, default=300)
    ap.add_argument("--records", type=int, default=33000)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step", choices=sorted(STEP_TIMEOUT), help="(child) run one step in this process and print its row")
    a = ap.parse_args()
    if a.step:
        print("ROW " + json.dumps({"device": step_device, "host_out": step_host_out, "append": step_append}[a.step](a)), flush=True)
        return 0
    rows = []
    for step in ("device", "host_out", "append"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step, "--submaps",
               str(a.submaps), "--records", str(a.records), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        row = [ln[4:] for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not row:
            print(f"step {step} failed with status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", flush=True)
            break
        rows.append(json.loads(row[0]))
        print(row[0], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)
    return 0 if len(rows) == 3 else 1


if __name__ == "__main__":
    sys.exit(main())

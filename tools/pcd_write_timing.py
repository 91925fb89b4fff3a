#!/usr/bin/env python3
"""Times writing map.pcd as DATA ascii, DATA binary and DATA binary_compressed from a map resident on the device (lsr_save_pcd,
csrc/pcd_deflate.hip), the three kinds interleaved in one run so that they meet the same machine state.  A tool, not a test.

    python tools/pcd_write_timing.py [--records 10000000] [--reps 5] [--warmup 1] [--dir DIR] [--out profiles/pcd_write.md]

The maps are those of tools/pcd_compressed_timing.py: --records pcl::PointXYZI records on a centimetre grid with intensities 0 .. 255
("grid"), and an all-zero map ("zeros").  Per map and kind: the file's bytes; the host clock around lsr_save_pcd to a file in --dir
(default: /dev/shm when there is one, the fastest local file system) and to /dev/null; for the compressed kind LSR_PCD_DEFLATE_MS (the
hipEvent brackets of gather, chunk compressor, scan and compaction), a one-thread host lzfg_compress (tests/cpp/lzf_greedy.cpp) of the
same field-major image as the baseline, and the device stream's size against that encoder's.  Every written file is read back with
lsr_load_pcd and compared with the records, byte for byte (the ASCII file: to the 8 digits it holds).  Prints one JSON line and writes the table.  There is no threshold."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

KINDS = ("ascii", "binary", "binary_compressed")


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _fmt(s):
    return f"{s['median']:.2f} ({s['min']:.2f} – {s['max']:.2f}, n = {s['n']})"


def run_case(a, name, reg, capi, codec, lzf_codec, torch, np):
    from pcd_compressed_timing import _cloud

    n = a.records
    pts = _cloud(n, name == "zeros")
    rec = np.zeros((n, 8), np.float32)
    rec[:, 0:3], rec[:, 4] = pts[:, 0:3], pts[:, 3]
    d_rec = torch.from_numpy(rec).cuda()
    image = np.ascontiguousarray(pts.T).reshape(-1).view(np.uint8)          # field-major: the x block, the y block, ...
    host_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        greedy = lzf_codec.compress(codec, image)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    path = os.path.join(a.dir, f"pcd_write_timing_{name}.pcd")
    row = dict(case=name, records=n, image_bytes=int(image.size), greedy_stream_bytes=int(greedy.size), host_one_thread_compress_ms=_stats(host_ms))
    to_file, to_null, deflate, size = {k: [] for k in KINDS}, {k: [] for k in KINDS}, [], {}
    want = d_rec.view(torch.uint8).view(n, 32)
    same = {}
    try:
        for it in range(a.warmup + a.reps):
            for kind in KINDS:
                if os.path.exists(path):      # (outside the clock: truncating the file of the kind before is not this kind's cost)
                    os.remove(path)
                t0 = time.perf_counter()
                size[kind] = reg.savePCDFile(path, d_rec, data=kind)
                t1 = time.perf_counter()
                if kind == "binary_compressed":
                    ms = reg.pcdDeflateMs()
                if it == 0:       # what was written is the map
                    got = reg.loadPCDFile(path, device=True)
                    # binary kinds: the bytes; ascii: "%.8g" and back is the float or its neighbour (8 of the 9 digits a float32 needs)
                    same[kind] = bool(torch.equal(got, want)) if kind != "ascii" else bool(
                        torch.allclose(got.view(torch.float32), want.view(torch.float32), rtol=2.5e-7, atol=0.0))
                    del got
                t2 = time.perf_counter()
                reg.savePCDFile("/dev/null", d_rec, data=kind)
                t3 = time.perf_counter()
                if it >= a.warmup:
                    to_file[kind].append((t1 - t0) * 1e3)
                    to_null[kind].append((t3 - t2) * 1e3)
                    if kind == "binary_compressed":
                        deflate.append(ms)
    finally:
        if os.path.exists(path):
            os.remove(path)
    stream_bytes = int(reg.lzfDeflate(torch.from_numpy(image).cuda()).numel())
    row.update(file_bytes=size, save_to_file_ms={k: _stats(v) for k, v in to_file.items()}, save_to_null_ms={k: _stats(v) for k, v in to_null.items()},
               deflate_ms=_stats(deflate), device_stream_bytes=stream_bytes, loaded_records_are_the_map=same)
    return row


def render(rows, a):
    out = ["# Writing map.pcd as ascii, binary and binary_compressed from the device: `tools/pcd_write_timing.py`", "",
           f"{a.records} pcl::PointXYZI records resident in HBM; times in ms by the host clock around `lsr_save_pcd`, median (min – max, n) of "
           f"{a.reps} after {a.warmup} warm-up, the three kinds interleaved in one run; one MI355X, one process; files in `{a.dir_name}`.",
           "`grid`: coordinates on a centimetre grid, intensities 0 .. 255; `zeros`: an all-zero map.", "",
           "| map | kind | file bytes | save to a file | save to /dev/null | `lsr_load_pcd` returns the map (ascii: to 8 digits) |", "|---|---|---|---|---|---|"]
    for r in rows:
        for k in KINDS:
            out.append(f"| {r['case']} | {k} | {r['file_bytes'][k]} | {_fmt(r['save_to_file_ms'][k])} | {_fmt(r['save_to_null_ms'][k])} | "
                       f"{r['loaded_records_are_the_map'][k]} |")
    out += ["", "## The compressor", "",
            "| map | image | device stream (chunks of 4096 bytes) | greedy encoder's stream (`tests/cpp/lzf_greedy.cpp`) | device / greedy | "
            "`LSR_PCD_DEFLATE_MS` (gather, compress, scan, compact) | host, one thread, `lzfg_compress` |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['case']} | {r['image_bytes']} | {r['device_stream_bytes']} ({100.0 * r['device_stream_bytes'] / r['image_bytes']:.1f} %) | "
                   f"{r['greedy_stream_bytes']} ({100.0 * r['greedy_stream_bytes'] / r['image_bytes']:.1f} %) | "
                   f"{r['device_stream_bytes'] / r['greedy_stream_bytes']:.3f} | {_fmt(r['deflate_ms'])} | {_fmt(r['host_one_thread_compress_ms'])} |")
    out += ["", "## Reading", ""]
    for r in rows:
        f = r["save_to_file_ms"]
        faster, fewer = f["binary"]["median"] < f["ascii"]["median"], r["file_bytes"]["binary"] < r["file_bytes"]["ascii"]
        out.append(f"* `{r['case']}`: the binary save to a file takes {f['binary']['median']:.1f} ms against {f['ascii']['median']:.1f} ms for ASCII "
                   f"({r['file_bytes']['binary'] / r['file_bytes']['ascii']:.2f} of the bytes): " +
                   ("faster, as expected of a save bound by the file write." if faster and fewer else
                    "faster, though it writes more bytes." if faster else
                    "slower, as the bytes say: the text of this map is the smaller file (a zero is two bytes of text, four of binary), and "
                    "a save is bound by the file write." if not fewer else
                    "NOT faster, against the expectation — the file write did not dominate this run; see the /dev/null column.") +
                   f"  Compressed: {f['binary_compressed']['median']:.1f} ms for {r['file_bytes']['binary_compressed'] / r['file_bytes']['binary']:.2f} "
                   f"of the binary file's bytes, {r['deflate_ms']['median']:.2f} ms of it in the deflate launches; the host encoder needs "
                   f"{r['host_one_thread_compress_ms']['median']:.0f} ms for the same image on one thread.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_write.md"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import lzf_codec
    from lidarslam_ros2_amd import NormalDistributionsTransform, _capi

    if not torch.cuda.is_available():
        raise SystemExit("pcd_write_timing: no GPU visible (there is no CPU path to time)")
    made = a.dir is None
    if made:
        a.dir = tempfile.mkdtemp(prefix="pcd_write_timing_", dir="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
    a.dir_name = os.path.dirname(a.dir) if made else a.dir
    codec = lzf_codec.load_codec()
    reg = NormalDistributionsTransform(device=0)
    reg.setProfiling(True)
    reg.pcdReadCompressed(True)
    try:
        rows = [run_case(a, name, reg, _capi, codec, lzf_codec, torch, np) for name in ("grid", "zeros")]
    finally:
        if made:
            os.rmdir(a.dir)
    with open(a.out, "w") as f:
        f.write(render(rows, a))
    print(json.dumps(dict(tool="pcd_write_timing", rows=rows)))
    if not all(all(r["loaded_records_are_the_map"].values()) for r in rows):
        raise SystemExit("pcd_write_timing: a written file does not read back as the map")


if __name__ == "__main__":
    main()

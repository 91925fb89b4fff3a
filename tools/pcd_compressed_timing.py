#!/usr/bin/env python3
"""Times reading a DATA binary_compressed map on the device (LSR_PCD_READ_COMPRESSED, csrc/pcd_lzf.hip) against a one-thread host
inflate of the same stream and against the DATA binary file of the same cloud.  A tool, not a test.

    python tools/pcd_compressed_timing.py [--records 10000000] [--reps 3] [--warmup 1] [--dir DIR] [--out profiles/pcd_compressed.md]

The map: --records pcl::PointXYZI records (x y z intensity, 16 bytes a point in the file) — the 10^7 points SURVEY.md 8f N5 / N7 name —
compressed two ways: by the greedy encoder of tests/cpp/lzf_greedy.cpp ("greedy"), and as an all-zero map ("zeros": one literal byte and
distance-1 references, the deepest chain a file of that size can hold).  Per compression:
  decode    lsr_decode_pcd, device image in, device records out: LSR_PCD_INFLATE_MS (the hipEvent brackets of the launches) and the rest
            of the call by the host clock
  load      lsr_load_pcd from a file in the page cache, device records out
  host      the same stream inflated by lzf_greedy.cpp's literal decoder on one host thread (no upload, no records)
  binary    lsr_load_pcd of the same cloud's DATA binary file (a path this feature does not touch)
Every run checks that the compressed file's records are the binary file's, byte for byte.  Prints one JSON line and writes the table."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], n=len(v))


def _header(n, kind):
    return (f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\n"
            f"WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA {kind}\n").encode()


def _cloud(n, zeros):
    """(n, 4) float32 x y z intensity: coordinates of a few hundred metres on a centimetre grid (what a voxel-filtered map holds),
    intensities 0 .. 255 — or all zero."""
    import numpy as np

    if zeros:
        return np.zeros((n, 4), np.float32)
    rng = np.random.default_rng(7)
    pts = np.empty((n, 4), np.float32)
    pts[:, 0:3] = np.round(rng.uniform(-300.0, 300.0, (n, 3)), 2).astype(np.float32)
    pts[:, 2] *= np.float32(0.05)
    pts[:, 3] = rng.integers(0, 256, n).astype(np.float32)
    return pts


def run_case(a, name, reg, capi, codec, lzf_codec, torch, np):
    n = a.records
    pts = _cloud(n, name == "zeros")
    image = np.ascontiguousarray(pts.T).reshape(-1).view(np.uint8)          # field-major: the x block, the y block, ...
    t0 = time.perf_counter()
    stream = lzf_codec.compress(codec, image)
    encode_ms = (time.perf_counter() - t0) * 1e3
    c_img = _header(n, "binary_compressed") + struct.pack("<II", stream.size, image.size) + stream.tobytes()
    b_img = _header(n, "binary") + pts.tobytes()
    c_path, b_path = os.path.join(a.dir, f"pcd_compressed_timing_{name}_c.pcd"), os.path.join(a.dir, f"pcd_compressed_timing_{name}_b.pcd")
    lay = reg._layout(32, (0, 4, 8, 16))
    out_c = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    out_b = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    cnt = C.c_size_t()
    row = dict(case=name, records=n, image_bytes=int(image.size), stream_bytes=int(stream.size), host_encode_ms=encode_ms)
    try:
        with open(c_path, "wb") as f:
            f.write(c_img)
        with open(b_path, "wb") as f:
            f.write(b_img)
        d_img = torch.from_numpy(np.frombuffer(c_img, np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        inflate, call, load_c, load_b, host = [], [], [], [], []
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            capi.check(reg._lib.lsr_decode_pcd(reg._h, C.c_void_p(d_img.data_ptr()), d_img.numel(), 1, C.c_void_p(out_c.data_ptr()), n, C.byref(lay), 1,
                                               C.byref(cnt)), "decode")
            t1 = time.perf_counter()
            ms = reg._getf(capi.PCD_INFLATE_MS)
            t2 = time.perf_counter()
            capi.check(reg._lib.lsr_load_pcd(reg._h, os.fsencode(c_path), C.c_void_p(out_c.data_ptr()), n, C.byref(lay), 1, C.byref(cnt)), "load")
            t3 = time.perf_counter()
            capi.check(reg._lib.lsr_load_pcd(reg._h, os.fsencode(b_path), C.c_void_p(out_b.data_ptr()), n, C.byref(lay), 1, C.byref(cnt)), "load binary")
            t4 = time.perf_counter()
            if it >= a.warmup:
                inflate.append(ms); call.append((t1 - t0) * 1e3); load_c.append((t3 - t2) * 1e3); load_b.append((t4 - t3) * 1e3)
        for _ in range(max(1, a.reps - 1)):
            t0 = time.perf_counter()
            st, back = lzf_codec.decompress(codec, stream, image.size)
            host.append((time.perf_counter() - t0) * 1e3)
            assert st == image.size
        row.update(same_records_as_binary=bool(torch.equal(out_c, out_b)), host_inflate_same_image=bool((back == image).all()),
                   decode_inflate_ms=_stats(inflate), decode_call_ms=_stats(call), load_compressed_ms=_stats(load_c), load_binary_ms=_stats(load_b),
                   host_one_thread_inflate_ms=_stats(host))
        row["decode_rest_ms"] = row["decode_call_ms"]["median"] - row["decode_inflate_ms"]["median"]
    finally:
        for p in (c_path, b_path):
            if os.path.exists(p):
                os.remove(p)
    return row


def render(rows, a):
    out = ["# Reading a DATA binary_compressed map on the device: `tools/pcd_compressed_timing.py`", "",
           f"{a.records} x y z intensity points (16 bytes a point in the file); medians of {a.reps} after {a.warmup} warm-up; MI355X, one process; files in the page cache.",
           "`greedy`: coordinates on a centimetre grid, compressed by `tests/cpp/lzf_greedy.cpp`; `zeros`: an all-zero map, one literal byte and",
           "distance-1 references (the deepest chain a file of that size can hold).", "",
           "| case | inflated | stream | decode: inflate launches (`LSR_PCD_INFLATE_MS`) | decode: rest of the call | decode: whole call | load compressed file | host, one thread, inflate only | load binary file | records = binary file's |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['case']} | {r['image_bytes'] / 1e6:.1f} MB | {r['stream_bytes'] / 1e6:.2f} MB | {r['decode_inflate_ms']['median']:.2f} ms | "
                   f"{r['decode_rest_ms']:.2f} ms | {r['decode_call_ms']['median']:.2f} ms | {r['load_compressed_ms']['median']:.2f} ms | "
                   f"{r['host_one_thread_inflate_ms']['median']:.2f} ms | {r['load_binary_ms']['median']:.2f} ms | {r['same_records_as_binary']} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcd_compressed.md"))
    a = ap.parse_args()
    import numpy as np
    import torch

    import lzf_codec
    from lidarslam_ros2_amd import NormalDistributionsTransform, _capi

    if not torch.cuda.is_available():
        raise SystemExit("pcd_compressed_timing: no GPU visible (there is no CPU path to time)")
    made = a.dir is None
    if made:
        a.dir = tempfile.mkdtemp(prefix="pcd_compressed_timing_")
    codec = lzf_codec.load_codec()
    reg = NormalDistributionsTransform(device=0)
    reg.setProfiling(True)
    reg.pcdReadCompressed(True)
    try:
        rows = [run_case(a, name, reg, _capi, codec, lzf_codec, torch, np) for name in ("greedy", "zeros")]
    finally:
        if made:
            os.rmdir(a.dir)
    with open(a.out, "w") as f:
        f.write(render(rows, a))
    print(json.dumps(dict(tool="pcd_compressed_timing", rows=rows)))
    if not all(r["same_records_as_binary"] and r["host_inflate_same_image"] for r in rows):
        raise SystemExit("pcd_compressed_timing: records differ")


if __name__ == "__main__":
    main()

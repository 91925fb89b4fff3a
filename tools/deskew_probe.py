"""What the IMU de-skew costs on the device.  (1) hipEvents around lsr_deskew_pc2 on a device-resident raw payload of 146k points
(the call enqueues one 10 KB table copy and four launches and returns when its mailbox word arrives); (2) the frontend's scan-in ->
pose-out (FrontendReplay.receive_cloud: de-skew, range filter, VoxelGrid, setInputSource, align) with and without use_imu on the same
scans.  Warm-up first, then the median and the spread of the repetitions; one JSON line at the end.

    python tools/deskew_probe.py [--points 146000] [--reps 200] [--warmup 20] [--scans 12] [--out profiles/deskew_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T0 = 1000.0      # stamp of the first scan [s]


def stamps_200hz(t_first, t_last):
    return t_first + 0.00123 + 0.005 * np.arange(int(np.floor((t_last - t_first) / 0.005)) + 1)


def sweep_scan(n, rng):
    """n points in payload order, one clockwise turn of azimuth with a little jitter, ranges 2 .. 60 m"""
    ori = -1.0 + 2 * np.pi * 0.98 * np.arange(n) / max(n - 1, 1) + rng.uniform(-0.01, 0.01, n)
    r = rng.uniform(2.0, 60.0, n)
    return np.stack([r * np.cos(-ori), r * np.sin(-ori), rng.uniform(-2.0, 6.0, n)], axis=1).astype(np.float32)


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), min=float(v.min()), n=int(v.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=146000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scans", type=int, default=12)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform, synth
    from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload

    rng = np.random.default_rng(0)
    res = dict(points=a.points, device=torch.cuda.get_device_name(0))

    # ---- (1) the call on its own
    reg = NormalDistributionsTransform(device=0)
    msgs = [((0.0, 0.0, float(np.sin(0.1 * (s - T0))), float(np.cos(0.1 * (s - T0)))), (0.0, 0.0, 0.2), (0.2, 0.0, 9.81), float(s))
            for s in stamps_200hz(T0 - 0.05, T0 + 0.15)]
    xyz = sweep_scan(a.points, rng)
    payload = torch.from_numpy(as_pc2_payload(xyz)).cuda()
    out = torch.empty_like(payload)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for form, dst in (("out_of_place", out), ("in_place", None)):
        dev_ms, host_ms = [], []
        for it in range(a.warmup + a.reps):
            reg.imuReset(0.1)                   # every repetition sees the same queue and the same cursor
            for m in msgs:
                reg.receiveImu(*m)
            work = dst if dst is not None else payload.clone()
            torch.cuda.synchronize()
            # the events go on the stream the handle orders itself behind (torch's current one) and are closed after the call returned:
            # the handle has waited for its mailbox by then, so e1 - e0 brackets everything the call put on the device
            e0.record()
            t0 = time.perf_counter()
            _, info = reg.deskewPointCloud2(payload if dst is not None else work, a.points, 32, (0, 4, 8, 16), T0, out=work)
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            if it >= a.warmup:
                dev_ms.append(e0.elapsed_time(e1)); host_ms.append((t1 - t0) * 1e3)
        assert info["n_skipped"] == 0 and info["start_missing"] == 0
        res["deskew_%s_event_ms" % form] = _stats(dev_ms)
        res["deskew_%s_host_ms" % form] = _stats(host_ms)

    # ---- (2) scan in -> pose out, with and without use_imu
    import multiprocessing as mp

    with mp.get_context("spawn").Pool(min(16, len(os.sched_getaffinity(0)))) as p:
        drive = synth.cfg_frontend_drive(a.scans, pool=p)

    def ndt():
        r = NormalDistributionsTransform(device=0)
        r.setResolution(5.0); r.setTransformationEpsilon(0.01); r.setMaximumIterations(35); r.setNeighborhoodSearchMethod(DIRECT7)
        return r

    to_dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    for use_imu in (False, True):
        secs = []
        for rep in range(3):                    # the first drive warms allocations and the filter's device-side form
            fr = FrontendReplay(ndt(), FrontendParams(use_imu=use_imu), to_device=to_dev, mapper=ndt())
            fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
            o = FrontendResult()
            for j, scan in enumerate(drive["scans"]):
                t_scan = T0 + 0.1 * j
                if use_imu:                     # a sensor at rest in the IMU's eyes: the de-skew runs in full and moves nothing much
                    for s in stamps_200hz(t_scan - (0.05 if j == 0 else -0.005), t_scan + 0.1):
                        fr.receive_imu((0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 9.81), float(s))
                pl = torch.from_numpy(as_pc2_payload(scan)).cuda()
                torch.cuda.synchronize()
                fr.receive_cloud(pl, int(scan.shape[0]), o, scan_time=t_scan)
            fr.finish(o)
            if rep:
                secs += o.scan_seconds[1:]
        res["frontend_scan_ms_use_imu_%s" % ("on" if use_imu else "off")] = _stats(np.asarray(secs) * 1e3)
        res["frontend_points_per_scan"] = int(np.mean([s.shape[0] for s in drive["scans"]]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""The sensor-frame transform on the 147k-point PointXYZI payload of tools/frontend_scan_probe.py (profiles/sensor_transform.md).

    --step kernels   REPS source calls without a mount (pc2_ingest_kernel<false>), REPS with one (pc2_ingest_kernel<true>) and REPS
                     stand-alone transforms in place (pc2_transform_kernel), alternating — the target of a
                     `rocprofv3 --kernel-trace --stats` run of its own
    --step plain     the source calls without a mount only: runs on a tree that predates the feature as well (--tree), which is how
                     the parent commit's pc2_ingest_kernel is taken
    --step replay    the frontend replay over 12 scans with and without a mount, alternating drives; prints the medians of
                     scan_in_to_pose_out (host clock around calls that end in a wait for the device), profiler off
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=("kernels", "plain", "replay"), default="kernels")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose package is imported")
ap.add_argument("--reps", type=int, default=100)
args = ap.parse_args()
sys.path.insert(0, args.tree); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import multiprocessing as mp

import numpy as np

from lidarslam_ros2_amd import synth
from _cache import cached

MOUNT = ((1.2, 0.0, 2.0), (0.0, 0.0, 0.0, 1.0))   # scanmatcher/launch/mapping_car.launch.py:28


def _pool():
    return mp.get_context("fork").Pool(min(16, len(os.sched_getaffinity(0))))


def _ndt():
    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform
    r = NormalDistributionsTransform(0); r.setResolution(5.0); r.setTransformationEpsilon(0.01); r.setMaximumIterations(35); r.setNeighborhoodSearchMethod(DIRECT7)
    return r


if args.step in ("kernels", "plain"):
    def _c2():
        with _pool() as p: return synth.cfg_ndt_30k(pool=p, keep_parts=True)
    case = cached("probe_cfg_ndt_30k_parts", _c2)
    import torch
    from lidarslam_ros2_amd.frontend import as_pc2_payload
    raw = case.raw_source
    n = int(raw.shape[0])
    payload = torch.from_numpy(as_pc2_payload(raw)).cuda(); torch.cuda.synchronize()
    work = payload.clone()
    r = _ndt()
    kept = []
    for _ in range(args.reps):
        kept.append(r.setInputSourcePointCloud2(payload, n, 32, (0, 4, 8, 16), 0.1, 100.0, 0.2))
        if args.step == "kernels":
            kept.append(r.setInputSourcePointCloud2(payload, n, 32, (0, 4, 8, 16), 0.1, 100.0, 0.2, sensor_transform=MOUNT))
            r.transformPointCloud2(work, n, 32, (0, 4, 8, 16), MOUNT[0], MOUNT[1], out=work)
    torch.cuda.synchronize()
    print("sensor_transform_probe %s: %d points, %d repetitions, points kept %s" % (args.step, n, args.reps, sorted(set(kept))), flush=True)
else:
    def _drive():
        with _pool() as p: return synth.cfg_frontend_drive(12, pool=p)
    drive = cached("probe_cfg_frontend_drive_12", _drive)
    import torch
    from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload
    hosts = [as_pc2_payload(s) for s in drive["scans"]]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    to_device = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()

    def replay(mount):
        # the same payloads either way: with the mount they are read as sensor-frame records, so the two drives do the same work per
        # scan on different coordinates — what is compared is the time, not the poses
        p = FrontendParams() if mount is None else FrontendParams(sensor_translation=mount[0], sensor_rotation_xyzw=mount[1])
        fr = FrontendReplay(_ndt(), p, to_device=to_device, mapper=_ndt())
        fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
        out = FrontendResult()
        for h, d in zip(hosts, devs):
            fr.receive_cloud(d, int(h.shape[0]), out, payload_host=h)
        fr.finish(out)
        return out.scan_seconds

    # a mount small enough for the drive to stay a drive (the scans are robot-frame scans): 1 cm, so that every scan still registers
    small = ((0.01, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    replay(None); replay(small)   # warm-up: code objects, buffers
    plain, mounted = [], []
    for _ in range(max(1, args.reps // 20)):
        plain += replay(None)[1:]
        mounted += replay(small)[1:]
    us = lambda v: 1e6 * float(np.median(v))
    print("sensor_transform_probe replay: scan_in_to_pose_out median %.1f us without a mount (%d scans), %.1f us with one (%d scans)" %
          (us(plain), len(plain), us(mounted), len(mounted)), flush=True)

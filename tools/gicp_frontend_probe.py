"""The frontend in GICP mode over the 24-scan drive of tests/test_gicp_frontend_gpu.py (trans_for_mapupdate 1.25 m: eight map updates),
asynchronous map side, hand-over lag 0 (--lag), device-resident payloads and keyframes, after one warm-up drive: what a scan costs when it
takes a new target over against what a normal scan costs.  Prints ONE JSON object (kept as profiles/gicp_frontend_probe.json).

  --lazy     the builder never calls prepareTarget: the scan that takes a target over computes the target's covariances inside its
             align, as the reference does (the "before" shape on the same build)
  --window   additionally times lsr_set_input_target_frames_filtered of the drive's 10-frame window with resident keyframes, and the
             path it replaces: per-frame assembly (setInputTargetFrames) + the stand-alone filter of the same points, host in / host out
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiprocessing as mp

from lidarslam_ros2_amd import synth
from _cache import cached


def _drive():
    with mp.get_context("fork").Pool(min(64, len(os.sched_getaffinity(0)))) as p:
        return synth.cfg_frontend_drive(24, pool=p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lazy", action="store_true")
    ap.add_argument("--window", action="store_true")
    ap.add_argument("--lag", type=int, default=0, help="hand-over lag in scans (0: the next callback waits for the map side; 1: it runs under the next scan)")
    ap.add_argument("--drives", type=int, default=3, help="measured drives after the warm-up one (medians are over all their scans)")
    args = ap.parse_args()
    drive = cached("probe_frontend_drive24", _drive)
    import torch

    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint
    from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload, _records

    def make():
        g = GeneralizedIterativeClosestPoint(0)
        g.setMaxCorrespondenceDistance(5.0); g.setTransformationEpsilon(1e-8)
        return g

    reg, mapper, builder = make(), make(), make()
    if args.lazy:
        builder.prepareTarget = lambda: None
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    hosts = [as_pc2_payload(s) for s in drive["scans"]]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    torch.cuda.synchronize()
    normal, taking, taking_net, updates, waits, forms, prepared = [], [], [], [], [], [], []
    for rep in range(1 + args.drives):
        fr = FrontendReplay(reg, FrontendParams(registration_method="GICP", trans_for_mapupdate=1.25), to_device=to_dev, mapper=mapper,
                            builder=builder, async_update=True, swap_lag=args.lag)
        hand_over = fr._hand_over

        def look(fr=fr, hand_over=hand_over):
            hand_over()
            prepared.append(bool(fr.reg.targetPrepared()))

        fr._hand_over = look
        fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
        out = FrontendResult()
        for d, h in zip(devs, hosts):
            fr.receive_cloud(d, int(d.shape[0]), out, payload_host=h)
            forms.append(builder.voxelFilterForm())
        fr.finish(out)
        if rep == 0:
            prepared.clear(); forms.clear()
            continue
        took = {j: w for j, w in zip(out.swap_at, out.swap_wait_seconds)}   # the wait for the worker is inside the scan's clock
        for j, s in enumerate(out.scan_seconds):
            (taking if j in took else normal).append(s)
            if j in took:
                taking_net.append(s - took[j])
        updates += out.update_seconds; waits += out.swap_wait_seconds
    ms = lambda v: {"median_ms": 1e3 * float(np.median(v)), "max_ms": 1e3 * float(np.max(v)), "n": len(v)}
    res = {"what": "GICP frontend, 24-scan drive, asynchronous map side, lag %d, %d measured drives after one warm-up" % (args.lag, args.drives),
           "prepare_target": not args.lazy,
           "scan_not_taking_a_target": ms(normal), "scan_taking_a_target": ms(taking),
           "scan_taking_a_target_without_its_wait_for_the_worker": ms(taking_net),
           "taking_over_normal_median": float(np.median(taking) / np.median(normal)),
           "taking_without_wait_over_normal_median": float(np.median(taking_net) / np.median(normal)),
           "update": ms(updates), "swap_wait": ms(waits),
           "target_prepared_at_hand_over": sorted(set(prepared)), "builder_voxel_filter_forms": sorted(set(forms)),
           "updates_at": out.update_at}
    if args.window:
        frames = [to_dev(_records(as_pc2_payload(f))) for f in drive["frames"]][::-1]
        poses = [np.asarray(P, np.float64) for P in drive["frame_poses"]][::-1]
        torch.cuda.synchronize()
        w = make()
        t_new, t_old_assembly, t_old_filter = [], [], []
        for rep in range(8):
            t0 = time.perf_counter()
            n_new = w.setInputTargetFramesFiltered(frames, poses, 0.2)
            t_new.append(time.perf_counter() - t0)
        form = w.voxelFilterForm()
        # the path before: the window assembled frame by frame into a target (device), and the filter of the same points through the
        # host (the only filter there was for a cloud that is not a scan)
        import oracle.oracle as O
        assembled = np.concatenate([O.transform_point_cloud(_records(as_pc2_payload(f))[:, :3], np.asarray(P, np.float32))
                                    for f, P in zip(drive["frames"][::-1], poses)])
        v = make()
        for rep in range(8):
            t0 = time.perf_counter()
            v.setInputTargetFrames(frames, poses)
            t1 = time.perf_counter()
            filtered = v.voxelGridFilter(assembled, 0.2)
            t2 = time.perf_counter()
            v.setInputTarget(filtered)
            t3 = time.perf_counter()
            t_old_assembly.append(t1 - t0); t_old_filter.append(t3 - t1)
        res["window"] = {"points_in": int(assembled.shape[0]), "points_out": int(n_new), "filter_form": int(form),
                         "set_input_target_frames_filtered_ms": 1e3 * float(np.median(t_new[2:])),
                         "before_per_frame_assembly_ms": 1e3 * float(np.median(t_old_assembly[2:])),
                         "before_host_filter_and_set_input_target_ms": 1e3 * float(np.median(t_old_filter[2:]))}
    for o in (reg, mapper, builder):
        o.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

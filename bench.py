#!/usr/bin/env python
"""bench.py — headline benchmark of the registration hot path (BASELINE.json).

  python bench.py --gpus N --steps K --warmup W            (N=1 default; N>1 without a launcher: spawns N ranks itself)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one scan registration as the frontend performs it per LiDAR scan
(scanmatcher_component.cpp:329,353): setInputSource(30k-pt scan, already resident in HBM) + NDT
align() against the resident 10-frame submap — BASELINE.json configs[1]: ndt_resolution 5.0,
vg_size_for_input 0.2, DIRECT7, fixed 30 iterations (max_iterations=30, transformation_epsilon=0 so
the loop never exits early).  The K timed steps are K DIFFERENT scans (a stream:
positions 0.5 / 1.0 / 1.5 m past the last keyframe, own noise and sub-sample each).  value =
registrations/s over all ranks (weak scaling: every rank registers its own scan stream against its
own copy of the submap; the only exchange is one all-gather of the K result records per rank at the
end — SURVEY.md §8e).

A plain run sets up, warms up, times the K steps and prints the headline line; --dump-outputs DIR also writes what the
last timed step returned (dump_outputs).  With --full the JSON line also carries
  roofline       derivative kernel: algorithmic bytes per launch / hipEvent-measured launch
                 duration vs 8 TB/s, next to the HBM bytes the PMC counters saw (profiles/pmc_ndt_eval_latest.json);
  cpu_baseline   the CPU oracle (C++/OpenMP restatement of ndt_omp — NOT ndt_omp itself) on this box's host cores;
  scan_stream    per-registration latency (median, p10, p90) over >= 50 different scans, cfg 2 and cfg 1 settings,
                 HBM-resident and host-resident (pageable / pinned) scans;
  cfg4_loop_batch 64 DISTINCT (target, source, guess) loop-closure candidates, each paying setInputTarget +
                 setInputSource + align + getFitnessScore (graph_based_slam_component.cpp:181-231), sharded over the ranks
                 with one all-gather of 64-byte records (lsr_align_batch_sharded);
  cfg5_dense     120k-pt 64-line scan vs 20-frame submap, ndt_resolution 2.0;
  gicp_cfg3, loop_gate, set_input_target.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import multiprocessing as mp
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)
PMC_GICP_FILE = os.path.join(ROOT, "profiles", "pmc_gicp_latest.json")  # written by tools/pmc_gicp.sh
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_ndt_eval_latest.json")  # written by tools/pmc_ndt.sh (rocprofv3 --pmc passes)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also run every other leg (roofline, cfg 3/4/5, streams, loop gate, CPU baseline); off: the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy")
    ap.add_argument("--stream", type=int, default=50, help="--full: scans in the latency-statistics stream (>= 50)")
    ap.add_argument("--candidates", type=int, default=64, help="--full: loop-closure candidates of the cfg 4 leg")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the cpu_baseline leg")
    ap.add_argument("--no-extras", action="store_true", help="--full: headline + roofline only")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--workers", type=int, default=0, help="workload-generation processes (default: host threads / ranks, <= 64)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` without torchrun spawns the N ranks itself
# ------------------------------------------------------------------------------------------------------------------
def self_spawn(args) -> int:
    import torch

    ndev = torch.cuda.device_count()
    shared = bool(os.environ.get("LSR_BENCH_FORCE_DIST"))  # exercise the N-rank path on fewer devices (ranks share GPUs)
    if ndev < args.gpus and not shared:
        print(f"bench.py: --gpus {args.gpus} but only {ndev} device(s) are visible", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", LSR_BENCH_CHILD="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    return rc


def make_comm(lib, dist, rank, world, dev_index):
    """The library's communicator for the data-path collectives (csrc/comm.hip): rank 0 draws the 128-byte id, the control plane
    (gloo) carries it, every rank calls lsr_comm_create.  -> (handle or None, description for config.collective).  Creation runs
    under a watchdog and the ranks agree on the outcome over gloo: if ANY rank failed, every rank gives its communicator up and the
    records travel over gloo instead — the line is printed either way and says which it was."""
    from lidarslam_ros2_amd import _capi

    if dist is None:
        return None, "none (one rank)"
    import threading

    box = {}

    def _create():
        try:
            ident = (C.c_char * 128)()
            idb = None
            if rank == 0:
                try:
                    _capi.check(lib.lsr_comm_unique_id(ident), "lsr_comm_unique_id")
                    idb = bytes(ident)
                except Exception as e:
                    box["err"] = repr(e)
            b = [idb]
            dist.broadcast_object_list(b, src=0)
            if b[0] is None:
                box.setdefault("err", "rank 0 could not draw a unique id")
                return
            ident = (C.c_char * 128).from_buffer_copy(b[0])
            comm = C.c_void_p()
            _capi.check(lib.lsr_comm_create(ident, rank, world, dev_index, C.byref(comm)), "lsr_comm_create")
            box["comm"] = comm
        except Exception as e:
            box["err"] = repr(e)

    # RCCL prints a version banner on stdout when a communicator is created; stdout must carry exactly one JSON line
    sys.stdout.flush()
    saved_fd = os.dup(1)
    os.dup2(2, 1)
    try:
        th = threading.Thread(target=_create, daemon=True)
        th.start()
        th.join(float(os.environ.get("LSR_BENCH_COMM_TIMEOUT", "180")))
        if th.is_alive():
            box["err"] = "lsr_comm_create did not return within its watchdog time"
    finally:
        sys.stdout.flush()
        os.dup2(saved_fd, 1)
        os.close(saved_fd)
    ok = [None] * world
    dist.all_gather_object(ok, box.get("err"))
    errs = [f"rank {r}: {e}" for r, e in enumerate(ok) if e]
    lib_name = os.environ.get("LSR_RCCL_LIB")
    kind = f"stand-in collective library {os.path.basename(lib_name)} (ranks share a device; test infrastructure)" if lib_name else "RCCL over xGMI"
    if errs:
        if "comm" in box and not any("watchdog" in e for e in errs):
            lib.lsr_comm_destroy(box["comm"])
        return None, "gloo all-gather of the records on the host — the library's communicator could not be created: " + "; ".join(errs)[:400]
    return box["comm"], f"lsr_comm_all_gather_records / lsr_align_batch_sharded / lsr_set_input_target_bcast: ncclAllGather + ncclBroadcast of the library's own communicator ({kind})"


LDS_PEAK_GBS = 256 * 128 * 2.4   # 256 CUs x 128 B per clock x 2.4 GHz = 78 643 GB/s (MI355X_MICROARCH.md: LDS bandwidth per CU)
SIMDS, CLOCK_MHZ = 1024.0, 2400.0
LDS_BYTES_PER_PAIR = 50          # one (point, voxel) pair read from the LDS image: 2-byte cell -> slot entry + 48-byte leaf record


def price_pass(us, pairs, valu_insts=None, traffic_bytes=None, table_in_lds=True):
    """Every resource that can bind a derivative launch, each as a fraction of ITS peak (no SURVEY-8d bytes priced
    against HBM where the records are gathered from LDS): VALU issue (wave-instructions x 4 cycles / SIMD-cycles of the launch), LDS
    bandwidth (pairs x 50 B / 78.6 TB/s; global-table kernels: none), HBM (the counters' bytes / 8 TB/s).  `binding` = the largest of
    them, or "latency" when none reaches 0.35 (the launch is a chain of dependent latencies: boundary, head read, controller,
    gather -> exp -> weight)."""
    r = {}
    if valu_insts:
        r["frac_valu"] = valu_insts * 4.0 / (SIMDS * us * CLOCK_MHZ)
    r["frac_lds"] = (pairs * LDS_BYTES_PER_PAIR / (us * 1e-6) / 1e9 / LDS_PEAK_GBS) if table_in_lds else 0.0
    if traffic_bytes:
        r["frac_hbm_traffic"] = traffic_bytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS
    cands = {"valu": r.get("frac_valu", 0.0), "lds": r["frac_lds"], "hbm": r.get("frac_hbm_traffic", 0.0)}
    top = max(cands, key=cands.get)
    r["binding"] = top if cands[top] >= 0.35 else "latency"
    return r


def pct(v, q):
    return float(np.percentile(np.asarray(v, np.float64), q))


def lat_stats(ts):
    ts = np.asarray(ts, np.float64) * 1e3
    return {"n": int(ts.size), "median_ms": float(np.median(ts)), "p10_ms": pct(ts, 10), "p90_ms": pct(ts, 90), "mean_ms": float(ts.mean()),
            "registrations_per_s": float(1e3 / np.median(ts))}


def dump_outputs(d, final, res):
    """--dump-outputs: what lsr_align hands its caller for the last timed step — the final transformation (row-major 4x4) and
    the lsr_result fields (gpu_ms, a timing, left out) — one DIR/<name>.npy each, so that two builds can be compared."""
    os.makedirs(d, exist_ok=True)
    arrays = {"final_transformation": np.asarray(final, np.float32), "score": np.float64(res.score),
              "iterations": np.float64(res.iterations), "converged": np.float64(res.converged),
              "n_evaluations": np.float64(res.n_evaluations), "n_correspondences": np.float64(res.n_correspondences)}
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), np.asarray(a))


def _candidate_job(c):
    from lidarslam_ros2_amd import synth

    k = synth.cfg_loop_candidate(c)
    return c, k.target, k.source, k.guess, k.truth


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_spawn(args))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    extras = args.full and not args.no_extras

    # ---- workloads first: generated by forked worker processes BEFORE this process touches the GPU
    from lidarslam_ros2_amd import synth
    from lidarslam_ros2_amd.sharding import shard_range

    t_gen = time.perf_counter()
    cores = len(os.sched_getaffinity(0))
    nwork = args.workers or max(1, min(64, cores // max(1, world)))
    n_stream = max(args.stream if (extras and rank == 0) else 0, min(args.steps + args.warmup, 64))
    my_cands = list(shard_range(args.candidates, world, rank)) if extras else []
    # LSR_BENCH_CACHE_DIR (tools/round_profiles.sh sets it): the deterministic synthetic clouds are kept on disk so that the
    # rocprofv3 / PMC re-runs of this command inside one GPU session do not ray-cast them again.  Nothing timed changes.
    cache = None
    if os.environ.get("LSR_BENCH_CACHE_DIR"):
        cache = os.path.join(os.environ["LSR_BENCH_CACHE_DIR"],
                             f"bench4_r{rank}w{world}_s{n_stream}_c{args.candidates}_e{int(extras)}.pkl")
    drive = drive20 = route_full = None
    if cache and os.path.exists(cache):
        import pickle
        with open(cache, "rb") as f:
            case, stream, cands, dense, gc, drive, drive20, route_full = pickle.load(f)
    else:
        with mp.get_context("fork").Pool(nwork) as pool:
            case = synth.cfg_ndt_30k(seed=0, pool=pool, keep_parts=(extras and rank == 0))   # the 10-frame submap (same on every rank) + its own next scan
            stream = synth.cfg_scan_stream(n_stream, seed=rank, pool=pool)   # this rank's scan stream
            cands = pool.map(_candidate_job, my_cands, chunksize=1) if my_cands else []
            dense = synth.cfg_dense_120k(seed=rank, pool=pool) if extras else None   # every rank: its own cfg 5 scan + submap
            gc = synth.cfg_gicp_30k(seed=rank, pool=pool) if extras else None
            # the frontend's RAW input over a drive (rank 0, one GPU): ten keyframes + scans every 0.5 m, map update every 1.5 m
            drive = synth.cfg_frontend_drive(max(12, min(args.stream, 60)), seed=0, pool=pool) if (extras and rank == 0 and world == 1) else None
            # the reference's own shipped parameter sets at full size: the 20-frame window of lidarslam/param/lidarslam.yaml
            # (24 scans = 8 map updates) and a there-and-back route of full-size submaps for the backend's loop gate
            drive20 = synth.cfg_frontend_drive(24, seed=0, pool=pool, n_keyframes=20) if (extras and rank == 0 and world == 1) else None
            route_full = synth.cfg_loop_route_full(pool=pool) if (extras and rank == 0 and world == 1) else None
        if cache:
            import pickle
            os.makedirs(os.path.dirname(cache), exist_ok=True)
            with open(cache + ".tmp", "wb") as f:
                pickle.dump((case, stream, cands, dense, gc, drive, drive20, route_full), f, protocol=4)
            os.replace(cache + ".tmp", cache)
    t_gen = time.perf_counter() - t_gen

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the registration core has no CPU path")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if local_rank < ndev else 0   # ranks share devices only under LSR_BENCH_FORCE_DIST
    own_device = world <= ndev
    torch.cuda.set_device(dev_index)
    dist = None
    backend = None
    if world > 1 or os.environ.get("LSR_BENCH_FORCE_DIST"):
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # ONE RCCL client per process (VERDICT r05 #1b): torch.distributed is the CONTROL plane only — barrier, the 128-byte id, the
        # max-reduce of the clocks, per-rank report objects — and runs on gloo; the data-path collective (the all-gather of the
        # 64-byte result records, the broadcast of a shared submap) is the library's own communicator (csrc/comm.hip -> RCCL over
        # xGMI), created once below and destroyed normally at the end.  Round 5 held torch's NCCL process group AND the library's
        # communicator in one address space and met a double free in ncclCommDestroy.
        backend = "gloo"
        # gloo announces its connections on stdout; stdout must carry exactly one JSON line: C-level stdout points at stderr meanwhile
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("gloo", rank=rank, world_size=world)
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
        if not own_device and not os.environ.get("LSR_RCCL_LIB"):
            # ranks share a device (LSR_BENCH_FORCE_DIST on a one-GPU box): RCCL refuses that layout; the shared-memory stand-in of
            # the tests carries the collectives so that comm.hip still runs every world > 1 line (test infrastructure, never timed
            # for a headline: the line says so in config.collective_library)
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from ccl_stub import build_stub
            if rank == 0:
                build_stub()
            dist.barrier()
            os.environ["LSR_RCCL_LIB"] = build_stub()

    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform, _capi
    from lidarslam_ros2_amd.posemath import pose_delta

    lib = _capi.load()
    fptr = C.POINTER(C.c_float)
    res, max_iter = 5.0, 30
    tstream = torch.cuda.current_stream().cuda_stream
    comm, comm_note = make_comm(lib, dist, rank, world, dev_index)

    def make_ndt(eps=0.0, mi=max_iter, resolution=res):
        r = NormalDistributionsTransform(device=dev_index, stream=tstream)
        r.setResolution(resolution)
        r.setTransformationEpsilon(eps)
        r.setMaximumIterations(mi)
        r.setNeighborhoodSearchMethod(DIRECT7)
        return r

    ndt = make_ndt()
    tgt_dev = torch.from_numpy(synth.as_pointxyzi(case.target)).cuda()
    ndt.setInputTarget(tgt_dev)
    grid = ndt.gridInfo()
    # the stream's scans as pcl::PointXYZI records in HBM, guesses as column-major 4x4
    src_dev = [torch.from_numpy(synth.as_pointxyzi(s)).cuda() for s, _, _ in stream]
    g16 = [np.ascontiguousarray(g.T, np.float32).reshape(16) for _, g, _ in stream]
    n_src_pts = int(src_dev[0].shape[0])
    fin16 = np.zeros(16, np.float32)
    torch.cuda.synchronize()

    # The timed loop drives the C ABI directly (what a C++ caller does): no per-step numpy conversions.
    def step(reg, j):
        _capi.check(lib.lsr_set_input_source_device(reg._h, C.c_void_p(src_dev[j].data_ptr()), 32, n_src_pts), "lsr_set_input_source_device")
        _capi.check(lib.lsr_align(reg._h, g16[j].ctypes.data_as(fptr), fin16.ctypes.data_as(fptr), C.byref(reg._last), None, 0), "lsr_align")
        reg._n_source = n_src_pts

    nss = len(src_dev)
    for k in range(args.warmup):
        step(ndt, k % nss)
    torch.cuda.synchronize()
    rec_np = np.zeros((args.steps, 16), np.float32)   # 64-byte result records (lsr_shard_record): row-major 3x4 | score | iterations | converged | fitness
    all_np = np.zeros((world, args.steps, 16), np.float32)

    def gather_records():
        """C1: the pose all-gather of the K records of every rank — the library's communicator (ncclAllGather over xGMI); gloo only
        if that communicator could not be created (the line then says so)."""
        if dist is None:
            return
        if comm is not None:
            _capi.check(lib.lsr_comm_all_gather_records(comm, rec_np.ctypes.data_as(C.c_void_p), args.steps, all_np.ctypes.data_as(C.c_void_p)),
                        "lsr_comm_all_gather_records")
        else:
            got = [torch.empty((args.steps, 16)) for _ in range(world)]
            dist.all_gather(got, torch.from_numpy(rec_np))

    if dist is not None:
        gather_records()   # warm-up of the one collective of the path too: RCCL sets up its all-gather channels on first use
        torch.cuda.synchronize()
        dist.barrier()
    torch.cuda.synchronize()
    lat = np.zeros(args.steps)
    evals = np.zeros(args.steps)   # derivative passes of every timed registration (the scans of the stream differ)
    t0 = time.perf_counter()
    tk = t0
    for k in range(args.steps):
        step(ndt, (args.warmup + k) % nss)
        rec_np[k, :12] = fin16.reshape(4, 4).T[:3].reshape(12)   # final transformation (column-major 4x4 -> row-major 3x4) into the record
        rec_np[k, 12] = ndt._last.score
        rec_np[k, 13] = ndt._last.iterations
        rec_np[k, 14] = ndt._last.converged
        evals[k] = ndt._last.n_evaluations
        tn = time.perf_counter()
        lat[k] = tn - tk
        tk = tn
    gather_records()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        tmax = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    last = ndt.last_result
    j_last = (args.warmup + args.steps - 1) % nss
    gpu_final = fin16.reshape(4, 4).T.copy()   # final transformation of the last timed registration
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, gpu_final, ndt._last)
    err_t, err_r = pose_delta(gpu_final, stream[j_last][2])
    value = world * args.steps / elapsed

    out = {
        "metric": "scan registrations/sec (30k-pt scan vs 10-frame submap)",
        "value": value, "unit": "registrations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "median_ms_per_step": 1e3 * float(np.median(lat)), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "accumulation_dtype": "f64", "data": "synthetic",
        "config": {"workload": "cfg2: single NDT align(), 30000-pt VLP-32 scan (vg 0.2) vs 10-frame submap (vg 0.1), "
                               "ndt_resolution 5.0, DIRECT7, max_iterations 30, transformation_epsilon 0; "
                               f"{args.steps} different scans (stream of {nss})",
                   "target_points": int(case.target.shape[0]), "source_points": n_src_pts,
                   "voxels_valid": grid["n_valid"], "newton_iterations": last["iterations"],
                   "derivative_passes_per_align": float(evals.mean()), "derivative_passes_last_scan": last["n_evaluations"],
                   "parallelism": f"1 registration stream per GPU x{world}",
                   "control_plane": backend, "collective": comm_note, "ranks_share_a_device": not own_device},
        "step_latency": lat_stats(lat),
        "last_step_error_vs_truth": {"translation_m": err_t, "rotation_rad": err_r},
        "ndt_iterations_per_s": world * args.steps * last["iterations"] / elapsed,
        "derivative_passes_per_s": world * float(evals.sum()) / elapsed,
        "workload_generation_s": t_gen, "workload_workers": nwork,
    }

    # ------------------------------------------------------------------------------------------------------------
    # cfg 4 (all ranks): 64 distinct candidates sharded over the ranks, one all-gather of 64-byte records
    # ------------------------------------------------------------------------------------------------------------
    # ---- roofline of the dominant kernel (K3+K4 derivative pass), hipEvents around the launch chains (rank 0; before the
    # multi-rank leg so that it is in the line whatever happens there)
    if rank == 0 and args.full:
        try:
            out["roofline"] = roofline_leg(ndt, step, n_src_pts, grid)
        except Exception as e:
            out["roofline"] = {"error": repr(e)}

    cfg4 = None
    cfg4_hung = False
    if extras and args.candidates > 0:
        box = {}

        def _leg():
            try:
                torch.cuda.set_device(dev_index)   # the current device is per thread
                box["v"] = run_cfg4(args, lib, rank, world, dev_index, tstream, cands, dist, comm, torch, synth)
            except Exception as e:  # the headline line must still be printed
                box["v"] = {"error": repr(e)}

        if world > 1:
            # A rank that fails inside communicator creation leaves the others waiting in RCCL's bootstrap: the leg runs under
            # a watchdog, and a rank whose leg does not come back prints (rank 0) / leaves without the final barrier.
            import threading
            th = threading.Thread(target=_leg, daemon=True)
            th.start()
            th.join(float(os.environ.get("LSR_BENCH_CFG4_TIMEOUT", "240")))
            if th.is_alive():
                cfg4_hung = True
                cfg4 = {"error": "the multi-rank cfg 4 leg did not finish within its watchdog time"}
            else:
                cfg4 = box.get("v")
        else:
            _leg()
            cfg4 = box.get("v")

    # ---- N > 1: the other batch shape, sharded — N keyframes vs ONE submap broadcast from rank 0 (every rank; watchdog as above)
    sharded_st = None
    if extras and dist is not None and comm is not None and not cfg4_hung:
        import threading
        box2 = {}

        def _leg2():
            try:
                torch.cuda.set_device(dev_index)
                box2["v"] = shared_target_sharded_leg(lib, comm, dist, rank, world, make_ndt, tgt_dev, src_dev, g16, n_src_pts, torch)
            except Exception as e:
                box2["v"] = {"error": repr(e)}

        th2 = threading.Thread(target=_leg2, daemon=True)
        th2.start()
        th2.join(float(os.environ.get("LSR_BENCH_CFG4_TIMEOUT", "240")))
        if th2.is_alive():
            cfg4_hung = True
            sharded_st = {"error": "the sharded shared-target leg did not finish within its watchdog time"}
        else:
            sharded_st = box2.get("v")

    stash = {}
    # ---- cfg 5 and cfg 3 on EVERY rank (BASELINE config 5 reads "1 and 8 GPUs"): each rank registers its own workload, the rank-0
    # line carries the per-rank figures and their sum (weak scaling; no collective on the data path)
    per_rank = {}
    if extras and not cfg4_hung:
        for name, fn in (("cfg5_dense", lambda: cfg5_leg(make_ndt, dense, torch, synth)),
                         ("gicp_cfg3", lambda: gicp_leg(gc, dev_index, tstream, torch, synth))):
            try:
                per_rank[name] = fn()
            except Exception as e:
                per_rank[name] = {"error": repr(e)}
        if dist is not None:
            gathered = [None] * world
            dist.all_gather_object(gathered, per_rank)
        else:
            gathered = [per_rank]
    if rank == 0:
        if cfg4 is not None:
            out["cfg4_loop_batch"] = cfg4
        if sharded_st is not None:
            out["ndt_shared_target_sharded"] = sharded_st
        if extras and not cfg4_hung:
            for name in ("cfg5_dense", "gicp_cfg3"):
                out[name] = gathered[0].get(name, {})
                if world > 1 and isinstance(out[name], dict):
                    rates = [g.get(name, {}).get("registrations_per_s") for g in gathered]
                    out[name]["ranks"] = {"registrations_per_s_per_rank": rates,
                                          "registrations_per_s_all_ranks": float(sum(r for r in rates if r)) if all(rates) else None,
                                          "median_ms_per_rank": [g.get(name, {}).get("median_ms") for g in gathered]}

        # The remaining legs are single-GPU reports: at N > 1 the other ranks would only wait for rank 0, and the CPU
        # baseline is defined at N = 1.
        if world == 1 and extras:
            legs = [("set_input_target", lambda: target_leg(ndt, tgt_dev, case)),
                    ("scan_stream", lambda: stream_leg(args, lib, make_ndt, ndt, stream, src_dev, g16, n_src_pts, torch, synth)),
                    ("ndt_shared_target_batch", lambda: shared_target_leg(lib, make_ndt, ndt, src_dev, g16, n_src_pts, torch, tgt_dev, dev_index)),
                    ("frontend_stream", lambda: frontend_stream_leg(drive, dev_index, tstream, torch, args)),
                    ("frontend_stream_lidarslam_yaml", lambda: frontend_stream_ref_leg(drive20, dev_index, tstream, torch, args)),
                    ("loop_gate", lambda: loop_gate_leg(dev_index, tstream, torch, synth, stash)),
                    ("loop_gate_reference_params", lambda: loop_gate_ref_leg(route_full, dev_index, tstream, torch, synth, args)),
                    ("next_rows", lambda: next_rows_leg(case, dev_index, tstream, torch, synth, args))]
            for name, fn in legs:
                try:
                    out[name] = fn()
                except Exception as e:
                    out[name] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_cpu:
            try:
                cpu_leg(args, out, stash, case, stream, j_last, gpu_final, res, max_iter)
            except Exception as e:
                out["cpu_baseline"] = {"error": repr(e)}
        # the fed-chip figures next to the single-scan one: the derivative kernel on the workloads that fill the chip
        if isinstance(out.get("roofline"), dict):
            cr = (cfg4 or {}).get("chain_roofline") if isinstance(cfg4, dict) else None
            if isinstance(cr, dict) and "achieved" in cr:
                try:   # counter traffic of the lane kernel on a 16-member launch (tools/pmc_ndt.sh on tools/trace_probe.py)
                    pb = json.load(open(PMC_FILE)).get("batch")
                    if pb and pb.get("bytes_per_launch"):
                        cr["traffic"] = int(pb["bytes_per_launch"])
                        cr["traffic_is"] = "HBM bytes of the MEDIAN launch of a 16-member chain (2 x FETCH_SIZE + WRITE_SIZE): " + str(pb.get("kernel"))
                        cr["traffic_per_member_pass_vs_algorithmic"] = (pb["bytes_per_launch"] / 16.0) / (cr["algorithmic_bytes"] / max(1, cr["member_passes"]))
                except Exception:
                    pass
                out["roofline"]["batch"] = cr
                # the same figures as top-level SCALARS of `roofline` (a consumer that keeps only scalar keys still sees the fed-chip
                # numbers): the candidate set's launch chains priced by SURVEY.md 8d bytes, its counter traffic, and
                # the VALU issue utilisation of its kernel — wave-instructions per member-pass x 4 issue cycles / (1024 SIMDs x time
                # per member-pass at 2.4 GHz) — which is the roofline that actually binds this kernel
                rl = out["roofline"]
                rl["batch_chain_ms"] = cr["chain_ms"]; rl["batch_member_passes"] = cr["member_passes"]
                rl["batch_us_per_member_pass"] = cr["us_per_member_pass"]
                rl["batch_algorithmic_8d_GBps"] = cr["achieved"]   # SURVEY 8d bytes per second: NOT an HBM utilisation (the records come from LDS)
                if cr.get("traffic"):
                    rl["batch_traffic_bytes"] = cr["traffic"]
                try:
                    pb = json.load(open(PMC_FILE)).get("batch") or {}
                    members = 16.0   # the counter launch holds 16 members (tools/pmc_ndt.sh)
                    pairs_mp = cr["mean_valid_pairs_per_point"] * 30000.0   # valid pairs of one member-pass
                    pr = price_pass(cr["us_per_member_pass"], pairs_mp, (pb["SQ_INSTS_VALU"] / members) if pb.get("SQ_INSTS_VALU") else None,
                                    (pb["bytes_per_launch"] / members) if pb.get("bytes_per_launch") else None)
                    if pb.get("SQ_INSTS_VALU"):
                        rl["batch_valu_insts_per_member_pass"] = pb["SQ_INSTS_VALU"] / members
                    for k_, v_ in pr.items():
                        rl["batch_" + k_] = v_
                        cr[k_] = v_
                except Exception:
                    pass
                cr.pop("frac", None); cr.pop("peak", None)   # (the 8d figure stays as `achieved`, labelled; no fraction of HBM is claimed for it)
                cr["achieved_is"] = "SURVEY.md 8d algorithmic bytes per second of the set's launch chains; the kernel gathers its records from LDS: see frac_valu / frac_lds / frac_hbm_traffic"
            c5 = out.get("cfg5_dense")
            if isinstance(c5, dict) and "avg_pass_us" in c5:
                pr5 = {}
                try:
                    p5 = json.load(open(PMC_FILE)).get("cfg5") or {}
                    pr5 = price_pass(c5["avg_pass_us"], c5.get("valid_pairs_per_pass", 0), p5.get("SQ_INSTS_VALU"), p5.get("bytes_per_launch"), table_in_lds=False)
                except Exception:
                    pass
                out["roofline"]["cfg5"] = dict({"kernel": "ndt_eval_lane_kernel<7, dense global table, 512> (single 120k-pt scan)", "avg_launch_us": c5["avg_pass_us"],
                                                "algorithmic_bytes_per_launch": c5.get("algorithmic_bytes_per_pass"),
                                                "frac_algorithmic_8d": c5.get("algorithmic_frac_of_hbm_peak"), "traffic": c5.get("traffic")}, **pr5)
                out["roofline"]["cfg5_frac"] = c5.get("algorithmic_frac_of_hbm_peak")   # global-table gathers: 8d bytes against HBM, as the contract prices them
                out["roofline"]["cfg5_pass_us"] = c5["avg_pass_us"]
                for k_, v_ in pr5.items():
                    out["roofline"]["cfg5_" + k_] = v_
                if c5.get("traffic"):
                    out["roofline"]["cfg5_traffic_bytes"] = c5.get("traffic")
            sb = out.get("ndt_shared_target_batch")
            if isinstance(sb, dict) and isinstance(sb.get("cfg2_fixed_30"), dict):
                st_ = sb["cfg2_fixed_30"]
                out["roofline"]["shared_target_us_per_member_pass"] = st_.get("us_per_member_pass")
                out["roofline"]["shared_target_algorithmic_8d_GBps"] = st_.get("chain_algorithmic_8d_GBps")
                try:   # the same kernel as the candidate set's (lane, LDS table, 512): its counters per member-pass
                    pb = json.load(open(PMC_FILE)).get("batch") or {}
                    pr = price_pass(st_["us_per_member_pass"], st_.get("valid_pairs_per_member_pass", 0), (pb["SQ_INSTS_VALU"] / 16.0) if pb.get("SQ_INSTS_VALU") else None,
                                    (pb["bytes_per_launch"] / 16.0) if pb.get("bytes_per_launch") else None)
                    for k_, v_ in pr.items():
                        out["roofline"]["shared_target_" + k_] = v_
                        st_[k_] = v_
                except Exception:
                    pass
        # the 8-GPU projection of the candidate set as top-level scalars: inputs and result
        pj = (cfg4 or {}).get("projected_8gpu") if isinstance(cfg4, dict) else None
        if isinstance(pj, dict) and isinstance(pj.get("block"), dict):
            out["cfg4_set_ms_one_gpu"] = pj["block"]["set_ms_on_one_gpu"]
            out["cfg4_max_share_ms_block"] = pj["block"]["max_share_ms"]
            out["cfg4_projected_speedup_8_gpus"] = pj["block"]["projected_speedup_8_gpus"]
            if isinstance(pj.get("planned_longest_first"), dict):
                out["cfg4_max_share_ms_planned"] = pj["planned_longest_first"]["max_share_ms"]
        # ... and of the other batch shape (N keyframes vs ONE submap: the one that fills a chip; VERDICT r05 #1c)
        sp = (out.get("ndt_shared_target_batch") or {}).get("sharded_8_projection") if isinstance(out.get("ndt_shared_target_batch"), dict) else None
        if isinstance(sp, dict) and "projected_speedup_8_gpus" in sp:
            out["shared_target_scans_total"] = sp["scans_total"]
            out["shared_target_set_ms_one_gpu"] = min(x for x in (sp["one_gpu_ms_as_8_sets"], sp["one_gpu_ms_as_one_set"]) if x)
            out["shared_target_max_share_ms"] = sp["max_share_ms"] + sp["xgmi_broadcast_allowance_ms"]
            out["shared_target_projected_speedup_8_gpus"] = sp["projected_speedup_8_gpus"]
        print(json.dumps(out), flush=True)

    if cfg4_hung:
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(0)   # the stuck leg holds a thread inside the collective library: no orderly shutdown is possible
    if dist is not None:
        dist.barrier()
        if comm is not None:
            lib.lsr_comm_destroy(comm)   # destroyed normally: this process holds ONE collective-library client
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------------------
def roofline_leg(ndt, step, n_src, grid):
    ndt.setProfiling(True)
    ndt.getProfile(reset=True)
    for _ in range(3):
        step(ndt, 0)
    prof = ndt.getProfile(reset=True)
    ndt.setProfiling(False)
    nblocks = (n_src + 127) // 128                      # quad kernel: 128 points per workgroup
    launches = max(1, prof["deriv_launches"])
    avg_us = 1e3 * prof["deriv_ms_total"] / launches
    pairs = prof["deriv_pairs"]
    alg_bytes = n_src * 12 + pairs * 40 + nblocks * 224
    achieved = alg_bytes / (avg_us * 1e-6) / 1e9
    r = {"bound": "latency (lds-gather)", "priced_against": "hbm",
         "kernel": "ndt_eval_quad_kernel<7> (derivative pass + fused Newton/More-Thuente controller)",
         "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
         "traffic": None, "traffic_source": None,
         "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_us": avg_us, "valid_pairs_per_point": pairs / n_src,
         "compulsory_bytes_per_launch": n_src * 12 + grid["n_valid"] * 36,
         "note": "achieved = ALGORITHMIC bytes (SURVEY.md 8d: N*12 + pairs*40 + G*224; the voxel records are gathered from an LDS "
                 "copy of the table, so most of these bytes never reach HBM) / hipEvent time per launch (launch to launch, the ~1 us "
                 "dependent-launch gap included).  `traffic` = HBM bytes per launch by the PMC counters; frac_by_traffic prices "
                 "those.  A single 30k-pt scan is LATENCY bound, not HBM bound (kernel boundary + head + controller step + one dependent LDS gather; "
                 "its whole working set is 0.4 MB), see DESIGN.md §4"}
    try:
        pmc = json.load(open(PMC_FILE))
        r["traffic"] = int(pmc["bytes_per_launch"])
        r["traffic_source"] = os.path.relpath(PMC_FILE, ROOT) + " <- " + pmc.get("source", "")
        r["frac_by_traffic"] = r["traffic"] / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS
        r["traffic_kernel"] = pmc.get("kernel")
        if pmc.get("SQ_INSTS_VALU"):
            # VALU utilisation next to frac = wave-instructions x 4 issue cycles / (1024 SIMDs x launch duration at 2.4 GHz)
            r["valu_utilisation"] = pmc["SQ_INSTS_VALU"] * 4.0 / (1024.0 * avg_us * 2400.0)
            r["valu_wave_instructions_per_launch"] = pmc["SQ_INSTS_VALU"]
        if pmc.get("SQ_WAIT_ANY") and pmc.get("SQ_WAVE_CYCLES"):
            r["wave_cycles_waiting"] = pmc["SQ_WAIT_ANY"] / pmc["SQ_WAVE_CYCLES"]
        if pmc.get("SQ_LDS_BANK_CONFLICT") and pmc.get("SQ_ACTIVE_INST_LDS"):
            r["lds_conflict_frac_of_lds_active"] = pmc["SQ_LDS_BANK_CONFLICT"] / pmc["SQ_ACTIVE_INST_LDS"]   # bank-conflict cycles / LDS-active cycles
        r.update(price_pass(avg_us, pairs, pmc.get("SQ_INSTS_VALU"), r["traffic"]))
        r["bound"] = r["binding"] + (" (boundary + head read + controller + one dependent LDS gather)" if r["binding"] == "latency" else "")
    except Exception:
        pass
    r["frac_is"] = "SURVEY.md 8d ALGORITHMIC bytes / launch time / 8 TB/s (the contract's figure); what binds the kernel: `binding`, frac_valu / frac_lds / frac_hbm_traffic"
    return r


def target_leg(ndt, tgt_dev, case):
    import torch

    ts = []
    for _ in range(20):
        t0 = time.perf_counter()
        ndt.setInputTarget(tgt_dev)          # K1/K2: voxel-covariance grid from the HBM-resident submap
        ts.append(time.perf_counter() - t0)
    torch.cuda.synchronize()
    m = float(np.median(ts))
    return {"median_ms": 1e3 * m, "p10_ms": 1e3 * pct(ts, 10), "p90_ms": 1e3 * pct(ts, 90), "target_points": int(case.target.shape[0]),
            "algorithmic_GBps": case.target.shape[0] * 20 / m / 1e9,   # ~20 B per target point
            "frac_of_hbm_peak": case.target.shape[0] * 20 / m / 1e9 / HBM_PEAK_GBS,
            "what": "setInputTarget on the HBM-resident 10-frame submap (PointXYZI records): de-interleave + bbox + counting sort + leaf sums + finalise + LDS table image"}


def stream_leg(args, lib, make_ndt, ndt, stream, src_dev, g16, n_src_pts, torch, synth):
    """Per-registration latency over a stream of different scans: cfg 2 and cfg 1 settings, device- and host-resident scans."""
    from lidarslam_ros2_amd import _capi
    from lidarslam_ros2_amd.posemath import pose_delta

    fptr = C.POINTER(C.c_float)
    fin = np.zeros(16, np.float32)
    n = len(src_dev)
    out = {"scans": n}

    def run(reg, setter, srcs):
        ts, its, errs = [], [], []
        for j in range(min(5, n)):
            setter(reg, srcs[j]); _capi.check(lib.lsr_align(reg._h, g16[j].ctypes.data_as(fptr), fin.ctypes.data_as(fptr), C.byref(reg._last), None, 0), "lsr_align")
        for j in range(n):
            t0 = time.perf_counter()
            setter(reg, srcs[j])
            _capi.check(lib.lsr_align(reg._h, g16[j].ctypes.data_as(fptr), fin.ctypes.data_as(fptr), C.byref(reg._last), None, 0), "lsr_align")
            ts.append(time.perf_counter() - t0)
            its.append(int(reg._last.iterations))
            errs.append(pose_delta(fin.reshape(4, 4).T, stream[j][2]))
        s = lat_stats(ts)
        s["newton_iterations_median"] = float(np.median(its))
        s["max_error_vs_truth"] = {"translation_m": float(max(e[0] for e in errs)), "rotation_rad": float(max(e[1] for e in errs))}
        return s

    def set_dev(reg, t):
        _capi.check(lib.lsr_set_input_source_device(reg._h, C.c_void_p(t.data_ptr()), 32, n_src_pts), "lsr_set_input_source_device")

    def set_host(reg, a):
        _capi.check(lib.lsr_set_input_source(reg._h, C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()), 32, n_src_pts),
                    "lsr_set_input_source")

    out["cfg2_device_source"] = run(ndt, set_dev, src_dev)
    front = make_ndt(eps=0.01, mi=35)         # the reference's own settings (scanmatcher_component.cpp:105-113)
    front.shareTargetOf(ndt)
    out["cfg1_device_source"] = run(front, set_dev, src_dev)
    host_pageable = [synth.as_pointxyzi(s) for s, _, _ in stream]
    out["cfg1_host_source_pageable"] = run(front, set_host, host_pageable)   # what the INTEGRATION.md binding does with a pcl cloud
    host_pinned = [torch.from_numpy(a).pin_memory() for a in host_pageable]
    out["cfg1_host_source_pinned"] = run(front, set_host, host_pinned)
    out["what"] = ("setInputSource + align per scan, host clock around the two C-ABI calls; cfg1 = transformation_epsilon 0.01, "
                   "max_iterations 35; host sources pay one 960 KB PCIe copy per scan")
    return out


def shared_target_leg(lib, make_ndt, owner, src_dev, g16, n_src_pts, torch, tgt_dev=None, dev_index=0):
    """north_star's other batch shape — "N keyframes vs. submap" (VERDICT r04 missing #2): the scans of the stream registered against
    the ONE resident 10-frame submap in shared launches.  Every member is its own registration object sharing the owner's target
    (lsr_share_target: one voxel table in HBM, one LDS image); lsr_set_input_source_batch + lsr_align_batch per set.  This is
    BASELINE's metric workload (30k-pt scan vs 10-frame submap) in the form that fills the chip.  cfg 2 settings (fixed 30
    iterations: the headline's schedule) and cfg 1 (the reference's own: eps 0.01); every member's final transformation is compared
    bit for bit with registering it alone (reference call site: scanmatcher_component.cpp:304-329, once per scan)."""
    from lidarslam_ros2_amd import _capi

    fptr = C.POINTER(C.c_float)
    m = min(len(src_dev), 64)
    out = {"members": m, "target_points_shared": True}
    for name, eps, mi in (("cfg2_fixed_30", 0.0, 30), ("cfg1_reference", 0.01, 35)):
        regs = []
        for _ in range(m):
            r = make_ndt(eps=eps, mi=mi)
            r.shareTargetOf(owner)
            regs.append(r)
        hs = (C.c_void_p * m)(*[r._h for r in regs])
        sptr = (C.c_void_p * m)(*[C.c_void_p(src_dev[j].data_ptr()) for j in range(m)])
        scnt = (C.c_size_t * m)(*[n_src_pts] * m)
        G = np.ascontiguousarray(np.stack(g16[:m]), np.float32)
        finals = np.zeros((m, 16), np.float32)
        res = (_capi.Result * m)()
        ts = []
        for rep in range(6):
            t0 = time.perf_counter()
            _capi.check(lib.lsr_set_input_source_batch(hs, m, sptr, scnt, 32, 1), "lsr_set_input_source_batch")
            _capi.check(lib.lsr_align_batch(hs, m, G.ctypes.data_as(fptr), finals.ctypes.data_as(fptr), res), "lsr_align_batch")
            if rep >= 2:
                ts.append(time.perf_counter() - t0)
        batch_T = finals.copy()
        passes = [int(r.n_evaluations) for r in res]
        pairs = [int(r.n_correspondences) for r in res]
        # the chain alone, hipEvents on the lead's stream (as roofline.batch does for the cfg-4 set)
        lead = regs[0]
        lead.setProfiling(True); lead.getProfile(reset=True)
        _capi.check(lib.lsr_align_batch(hs, m, G.ctypes.data_as(fptr), finals.ctypes.data_as(fptr), res), "lsr_align_batch")
        prof = lead.getProfile(reset=True); lead.setProfiling(False)
        # one by one through the same objects (quad kernel)
        one = np.zeros(16, np.float32)
        same, t1 = 0, []
        for j in range(m):
            t0 = time.perf_counter()
            _capi.check(lib.lsr_set_input_source_device(regs[j]._h, C.c_void_p(src_dev[j].data_ptr()), 32, n_src_pts), "lsr_set_input_source_device")
            _capi.check(lib.lsr_align(regs[j]._h, G[j].ctypes.data_as(fptr), one.ctypes.data_as(fptr), C.byref(regs[j]._last), None, 0), "lsr_align")
            t1.append(time.perf_counter() - t0)
            same += int(np.array_equal(one, batch_T[j]))
        tb = float(np.median(ts))
        alg = sum(e * (n_src_pts * 12 + p * 40) for e, p in zip(passes, pairs)) + prof["deriv_launches"] * 512 * 256
        ms_chain = prof["deriv_ms_total"]
        out[name] = {"ms_per_set": 1e3 * tb, "registrations_per_s": m / tb, "ms_per_registration_in_the_set": 1e3 * tb / m,
                     "one_by_one_ms_per_registration": 1e3 * float(np.median(t1)), "speedup_vs_one_by_one": float(np.sum(t1)) / tb,
                     "same_bits_as_one_by_one": same, "member_passes": int(sum(passes)), "launches": int(prof["deriv_launches"]),
                     "chain_ms": ms_chain, "us_per_member_pass": 1e3 * ms_chain / max(1, sum(passes)),
                     "valid_pairs_per_member_pass": float(sum(e * p for e, p in zip(passes, pairs))) / max(1, sum(passes)),
                     "chain_algorithmic_8d_GBps": alg / (ms_chain * 1e-3) / 1e9}   # SURVEY 8d bytes per second (gathers served from LDS: not an HBM utilisation)
        for r in regs:
            r.close()
    out["what"] = ("the stream's scans as ONE set against the shared 10-frame submap: lsr_set_input_source_batch + lsr_align_batch per set, "
                   "host clock; chain_ms = hipEvents around the set's launch chains")
    try:
        out["sharded_8_projection"] = shared_target_projection(lib, make_ndt, tgt_dev, src_dev, g16, n_src_pts, dev_index)
    except Exception as e:
        out["sharded_8_projection"] = {"error": repr(e)}
    return out


def shared_target_projection(lib, make_ndt, tgt_dev, src_dev, g16, n_src_pts, dev_index, world=8):
    """What ONE GPU can say about north_star's ">= 6x batched-scan throughput at 8 GPUs" on the batch shape that fills a chip: 8 x m
    scans against ONE submap (cfg 2 schedule).  One GPU: setInputTarget once, then all 8 x m scans — as 8 sets of m one after the
    other AND as one set of 8 x m, whichever is faster.  One of 8 ranks: the submap arrives (lsr_set_input_target_bcast; here
    lsr_set_input_target_device stands in for broadcast + build: the 21 MB records over xGMI at >= 50 GB/s are ~0.4 ms more, added
    below as an allowance), the voxel grid is built redundantly per rank, the rank registers ITS m scans
    (lsr_set_input_source_batch + lsr_align_batch_sharded through a one-rank communicator, records exchanged).  Projection = one-GPU
    time / share time.  A projection from single-GPU measurements, not a scaling run: bench.py --gpus 8 runs the real thing
    (ndt_shared_target_sharded)."""
    from lidarslam_ros2_amd import _capi

    fptr = C.POINTER(C.c_float)
    m = min(len(src_dev), 55)
    total = m * world
    owner = make_ndt(eps=0.0, mi=30)
    regs = []
    for _ in range(total):
        r = make_ndt(eps=0.0, mi=30)
        regs.append(r)
    comm = C.c_void_p()
    _capi.check(lib.lsr_comm_create(None, 0, 1, dev_index, C.byref(comm)), "lsr_comm_create")
    hs = (C.c_void_p * total)(*[r._h for r in regs])
    sptr = (C.c_void_p * total)(*[C.c_void_p(src_dev[j % m].data_ptr()) for j in range(total)])
    scnt = (C.c_size_t * total)(*[n_src_pts] * total)
    G = np.ascontiguousarray(np.stack([g16[j % m] for j in range(total)]), np.float32)
    finals = np.zeros((total, 16), np.float32)
    res = (_capi.Result * total)()
    recs = (_capi.ShardRecord * total)()
    n_t = int(tgt_dev.shape[0])

    def set_target():
        _capi.check(lib.lsr_set_input_target_device(owner._h, C.c_void_p(tgt_dev.data_ptr()), 32, n_t), "lsr_set_input_target_device")
        for r in regs:
            r.shareTargetOf(owner)

    def sub(a, k):   # a ctypes / numpy view of members [k*m, (k+1)*m)
        return (type(a)._type_ * m).from_buffer(a, k * m * C.sizeof(type(a)._type_))

    def one_gpu_sets():
        t0 = time.perf_counter()
        set_target()
        for k in range(world):
            _capi.check(lib.lsr_set_input_source_batch(sub(hs, k), m, sub(sptr, k), sub(scnt, k), 32, 1), "lsr_set_input_source_batch")
            _capi.check(lib.lsr_align_batch(sub(hs, k), m, G[k * m:].ctypes.data_as(fptr), finals[k * m:].ctypes.data_as(fptr), sub(res, k)), "lsr_align_batch")
        return time.perf_counter() - t0

    def one_gpu_whole():
        t0 = time.perf_counter()
        set_target()
        _capi.check(lib.lsr_set_input_source_batch(hs, total, sptr, scnt, 32, 1), "lsr_set_input_source_batch")
        _capi.check(lib.lsr_align_batch(hs, total, G.ctypes.data_as(fptr), finals.ctypes.data_as(fptr), res), "lsr_align_batch")
        return time.perf_counter() - t0

    def share(k):
        t0 = time.perf_counter()
        set_target()
        _capi.check(lib.lsr_set_input_source_batch(sub(hs, k), m, sub(sptr, k), sub(scnt, k), 32, 1), "lsr_set_input_source_batch")
        _capi.check(lib.lsr_align_batch_sharded(comm, sub(hs, k), m, m, G[k * m:].ctypes.data_as(fptr), 0, recs), "lsr_align_batch_sharded")
        return time.perf_counter() - t0

    one_gpu_sets(); t_sets = min(one_gpu_sets() for _ in range(2))
    sets_T = finals.copy()
    try:
        one_gpu_whole(); t_whole = min(one_gpu_whole() for _ in range(2))
        whole_same = int(sum(np.array_equal(finals[j], sets_T[j]) for j in range(total)))
    except Exception as e:   # a set of 440 may exceed what one launch chain takes: the 8-sets form then stands alone
        t_whole, whole_same = None, repr(e)
    share(0); t_share = [min(share(k) for _ in range(2)) for k in range(world)]
    lib.lsr_comm_destroy(comm)
    for r in regs:
        r.close()
    owner.close()
    xgmi_allowance = (n_t * 32) / 50e9   # the records of the submap, one hop at 50 GB/s (a third of a link's 153 GB/s)
    t_one = min(t_sets, t_whole) if t_whole else t_sets
    t_rank = max(t_share) + xgmi_allowance
    return {"scans_total": total, "scans_per_rank": m, "ranks": world,
            "one_gpu_ms_as_8_sets": 1e3 * t_sets, "one_gpu_ms_as_one_set": (1e3 * t_whole) if t_whole else None, "one_set_same_bits_as_8_sets": whole_same,
            "share_ms": [round(1e3 * t, 4) for t in t_share], "max_share_ms": 1e3 * max(t_share), "xgmi_broadcast_allowance_ms": 1e3 * xgmi_allowance,
            "projected_speedup_8_gpus": t_one / t_rank, "registrations_per_s_one_gpu": total / t_one, "projected_registrations_per_s_8_gpus": total / t_rank,
            "note": "strong scaling of 8 x m scans vs ONE submap; the share includes the per-rank (redundant) voxel-grid build and the record exchange"}


def shared_target_sharded_leg(lib, comm, dist, rank, world, make_ndt, tgt_dev, src_dev, g16, n_src_pts, torch):
    """N > 1: north_star's "N keyframes vs. submap" sharded across the ranks as SURVEY.md 8e partitions it — rank 0 holds the
    10-frame submap (scanmatcher_component.cpp:449-464) and broadcasts its records (lsr_set_input_target_bcast: ncclBroadcast over
    xGMI), every rank builds the voxel grid, shares it among its m registration objects (lsr_share_target) and registers ITS m scans
    in shared launches; one ncclAllGather of the 64-byte records (lsr_align_batch_sharded) gives every rank all world x m poses.
    Timed from before the broadcast to after the all-gather, max over ranks.  cfg 2 schedule (30 fixed iterations)."""
    from lidarslam_ros2_amd import _capi

    fptr = C.POINTER(C.c_float)
    mt = torch.tensor([min(len(src_dev), 55)], dtype=torch.int64)
    dist.all_reduce(mt, op=dist.ReduceOp.MIN)   # the same share size on every rank (rank 0's stream is longer: it feeds the latency statistics)
    m = int(mt.item())
    owner = make_ndt(eps=0.0, mi=30)
    regs = [make_ndt(eps=0.0, mi=30) for _ in range(m)]
    hs = (C.c_void_p * m)(*[r._h for r in regs])
    sptr = (C.c_void_p * m)(*[C.c_void_p(src_dev[j].data_ptr()) for j in range(m)])
    scnt = (C.c_size_t * m)(*[n_src_pts] * m)
    G = np.ascontiguousarray(np.stack(g16[:m]), np.float32)
    recs = (_capi.ShardRecord * (m * world))()
    n_t = int(tgt_dev.shape[0])

    def round_():
        dist.barrier()
        t0 = time.perf_counter()
        _capi.check(lib.lsr_set_input_target_bcast(comm, owner._h, C.c_void_p(tgt_dev.data_ptr()) if rank == 0 else None, 32, n_t if rank == 0 else 0, 1, 0),
                    "lsr_set_input_target_bcast")
        t1 = time.perf_counter()
        for r in regs:
            r.shareTargetOf(owner)
        _capi.check(lib.lsr_set_input_source_batch(hs, m, sptr, scnt, 32, 1), "lsr_set_input_source_batch")
        _capi.check(lib.lsr_align_batch_sharded(comm, hs, m, m * world, G.ctypes.data_as(fptr), 0, recs), "lsr_align_batch_sharded")
        t2 = time.perf_counter()
        v = torch.tensor([t2 - t0, t1 - t0], dtype=torch.float64)
        dist.all_reduce(v, op=dist.ReduceOp.MAX)
        return float(v[0]), float(v[1])

    round_()
    best = min((round_() for _ in range(3)), key=lambda x: x[0])
    conv = int(sum(1 for k in range(m * world) if recs[k].converged > 0.5))
    for r in regs:
        r.close()
    owner.close()
    return {"scans_total": m * world, "scans_per_rank": m, "ranks": world, "ms_per_round": 1e3 * best[0], "ms_broadcast_and_grid_build": 1e3 * best[1],
            "registrations_per_s_all_ranks": m * world / best[0], "records_converged": conv,
            "what": "rank 0's submap by lsr_set_input_target_bcast, m scans per rank in shared launches, one all-gather of world x m records; max over ranks"}


def frontend_stream_leg(drive, dev_index, tstream, torch, args, res=5.0, params=None, label=None, light=False):
    """The frontend loop as the reference runs it, end to end (VERDICT r04 missing #4): scanmatcher_component.cpp:296-356 per scan,
    :436-481 per map update, replayed by lidarslam_ros2_amd.frontend.FrontendReplay over RAW scans (~147k points each) of a drive with
    a map update every 1.5 m.  scan_in_to_pose_out = raw PointCloud2 payload -> range filter -> VoxelGrid(vg_size_for_input) ->
    setInputSource -> align at the reference's settings; map_update = range filter + VoxelGrid(vg_size_for_map) of the scan into a
    keyframe that stays in HBM (lsr_set_input_source_pc2 on a second object + lsr_get_source_pc2_device) + assembly of the last
    num_targeted_cloud submaps + setInputTarget; the variant that takes the keyframe through the host, as the reference stores its
    submaps, is reported next to it.  `async_map_update` (round 6): the map side on a WORKER THREAD with its own objects and streams
    (scanmatcher_component.cpp:427-434), the callback takes the finished target over with lsr_share_target (:298-320) — hand-over lag 0
    (target in place for the very next scan) and 1 (the next scan is registered while the map side runs).  The same loop on the CPU
    oracle gives the parity of the WHOLE sequence: both sides feed on their own previous poses and their own maps.
    `res` / `params`: ndt_resolution and the frontend's parameters (default: BASELINE cfg 1/2; `light`: fewer variants)."""
    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform
    from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload
    from lidarslam_ros2_amd.posemath import pose_delta

    if drive is None:
        return {"skipped": "workload generated without the drive"}
    prm = params or FrontendParams()
    hosts = [as_pc2_payload(s) for s in drive["scans"]]
    devs = [torch.from_numpy(h).cuda() for h in hosts]
    torch.cuda.synchronize()

    def make(own_stream=False):
        # own_stream: True = a stream of the object's own, False = torch's current stream, an integer = that HIP stream
        st = None if own_stream is True else tstream if own_stream is False else own_stream
        r = NormalDistributionsTransform(device=dev_index, stream=st)
        r.setResolution(res); r.setTransformationEpsilon(0.01); r.setMaximumIterations(35); r.setNeighborhoodSearchMethod(DIRECT7)
        return r

    def replay(reg, device_payloads, to_device, mapper=None, builder=None, async_update=False, swap_lag=0):
        fr = FrontendReplay(reg, prm, to_device=to_device, mapper=mapper, builder=builder, async_update=async_update, swap_lag=swap_lag)
        fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
        res_ = FrontendResult()
        t0 = time.perf_counter()
        for h, d in zip(hosts, devs):
            fr.receive_cloud(d if device_payloads else h, int(h.shape[0]), res_, payload_host=h)
        fr.finish(res_)
        res_.wall_seconds = time.perf_counter() - t0
        return res_

    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    reg, mapper = make(), make()
    replay(reg, True, to_dev, mapper)         # first pass: allocations
    g = replay(reg, True, to_dev, mapper)     # keyframes produced and kept in HBM (lsr_get_source_pc2_device)
    n = len(g.poses)
    errs = [pose_delta(a, t) for a, t in zip(g.poses, drive["truths"])]
    upd = np.asarray(g.update_seconds) * 1e3
    out = {"scans": n, "raw_points_per_scan": int(np.mean([h.shape[0] for h in hosts])), "points_kept_median": float(np.median(g.points_kept)),
           "map_updates": len(g.update_at), "newton_iterations_median": float(np.median(g.iterations)),
           "settings": {"ndt_resolution": res, "vg_size_for_input": prm.vg_size_for_input, "vg_size_for_map": prm.vg_size_for_map,
                        "num_targeted_cloud": prm.num_targeted_cloud, "scan_min_range": prm.scan_min_range, "scan_max_range": prm.scan_max_range,
                        "trans_for_mapupdate": prm.trans_for_mapupdate, "transformation_epsilon": 0.01, "max_iterations": 35},
           "scan_in_to_pose_out": lat_stats(g.scan_seconds),
           "map_update_ms": {"median": float(np.median(upd)) if upd.size else None, "p90": pct(upd, 90) if upd.size else None},
           "ms_per_scan_with_map_update_amortised": 1e3 * g.wall_seconds / n,
           "max_error_vs_truth": {"translation_m": float(max(e[0] for e in errs)), "rotation_rad": float(max(e[1] for e in errs))},
           "what": "receiveCloud + updateMap replayed per scan through the C ABI (lsr_set_input_source_pc2, lsr_align, lsr_voxel_grid_filter_pc2, "
                   "lsr_set_input_target_frames); ms_per_scan_with_map_update_amortised = wall clock of the whole drive / scans"}
    if not light:
        gk = replay(reg, True, to_dev)            # keyframes through the host, as the reference stores its submaps (ROS messages)
        gh = replay(reg, False, to_dev)           # raw payload from host memory: one ~4.7 MB PCIe copy per scan
        upd_host = np.asarray(gk.update_seconds) * 1e3
        out["scan_in_to_pose_out_host_payload_pcie_inclusive"] = lat_stats(gh.scan_seconds)
        out["map_update_ms_keyframes_through_host"] = {"median": float(np.median(upd_host)) if upd_host.size else None,
                                                       "what": "lsr_voxel_grid_filter_pc2 host in / host out (range mask in numpy) + upload of the filtered keyframe, PCIe-inclusive"}
        out["device_and_host_keyframes_same_poses"] = bool(all(np.array_equal(a, b) for a, b in zip(g.poses, gk.poses)))
        out["host_payload_same_poses"] = bool(all(np.array_equal(a, b) for a, b in zip(g.poses, gh.poses)))
    # ---- the map side off the scan path: worker thread + mapper + builder on their own streams, hand-over by lsr_share_target
    try:
        # the callback's object stays on the stream the payloads live on (no cross-stream wait per scan); the map side gets its own
        # and shares ONE (every further hardware queue in use lengthens the dependent launches of all the others: measured)
        map_stream = torch.cuda.Stream(device=dev_index)
        ms = map_stream.cuda_stream if os.environ.get("LSR_BENCH_ASYNC_MAP_STREAMS", "1") == "1" else True
        a_reg, a_map, a_bld = make(os.environ.get("LSR_BENCH_ASYNC_REG_STREAM", "torch") == "own"), make(ms), make(ms)
        asy = {}
        for lag in (0, 1):
            ser = replay(a_reg, True, to_dev, a_map, a_bld, False, lag)
            replay(a_reg, True, to_dev, a_map, a_bld, True, lag)
            thr = replay(a_reg, True, to_dev, a_map, a_bld, True, lag)
            sc = np.asarray(thr.scan_seconds) * 1e3
            if os.environ.get("LSR_BENCH_DUMP_SCANS"):
                print(f"[scan dump lag {lag}] inline", np.round(np.asarray(g.scan_seconds) * 1e3, 3).tolist(), "\n serial", np.round(np.asarray(ser.scan_seconds) * 1e3, 3).tolist(),
                      "\n threaded", np.round(sc, 3).tolist(), "\n update_at", thr.update_at, "swap_at", thr.swap_at, "iterations", thr.iterations, file=sys.stderr)
            on_swap = [sc[j] for j in thr.swap_at if j < len(sc)]
            off_swap = [sc[j] for j in range(len(sc)) if j not in set(thr.swap_at)]
            trig = [sc[j] for j in thr.update_at]
            asy[f"hand_over_lag_{lag}"] = {
                "scan_in_to_pose_out": lat_stats(thr.scan_seconds),
                "scan_ms_median_on_hand_over_scans": float(np.median(on_swap)) if on_swap else None,
                "scan_ms_median_on_other_scans": float(np.median(off_swap)) if off_swap else None,
                "scan_ms_median_on_scans_that_trigger_an_update": float(np.median(trig)) if trig else None,
                "hand_over_wait_ms_median": 1e3 * float(np.median(thr.swap_wait_seconds)) if thr.swap_wait_seconds else None,
                "map_update_on_the_worker_ms_median": 1e3 * float(np.median(thr.update_seconds)) if thr.update_seconds else None,
                "ms_per_scan_with_map_update_amortised": 1e3 * thr.wall_seconds / n,
                "serial_replay_same_lag_ms_per_scan_amortised": 1e3 * ser.wall_seconds / n,
                "same_poses_as_the_serial_replay": bool(all(np.array_equal(x, y) for x, y in zip(thr.poses, ser.poses))),
                "map_updates": len(thr.update_at)}
            if lag == 0:
                asy["hand_over_lag_0"]["same_poses_as_the_inline_replay"] = bool(all(np.array_equal(x, y) for x, y in zip(thr.poses, g.poses)))
        asy["what"] = ("updateMap on a worker thread (mapper filters the keyframe, builder assembles the window and builds the voxel grid, each on its own "
                       "stream); the callback's object only registers and takes the finished target over (lsr_share_target).  Back-to-back replay: a 10 Hz "
                       "sensor leaves 100 ms between scans, here the next scan starts at once — lag 0 therefore waits for the worker, lag 1 overlaps it")
        out["async_map_update"] = asy
        a_reg.close(); a_map.close(); a_bld.close()
    except Exception as e:
        out["async_map_update"] = {"error": repr(e)}
    if not args.no_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from frontend_oracle import OracleFrontendRegistration   # test infrastructure: the checker, outside every timed region

        n_cpu = n if not light else min(n, 9)   # the oracle takes 40-150 ms per scan: a bounded prefix of the drive for the second parameter set
        hosts_cpu = hosts[:n_cpu]
        fr = FrontendReplay(OracleFrontendRegistration(res, 0.01, 35), prm)
        fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
        c = FrontendResult()
        t0 = time.perf_counter()
        for h in hosts_cpu:
            fr.receive_cloud(h, int(h.shape[0]), c, payload_host=h)
        t_cpu = time.perf_counter() - t0
        d = [pose_delta(a, b) for a, b in zip(g.poses[:n_cpu], c.poses)]
        out["parity_vs_cpu_over_the_stream"] = {"scans_compared": n_cpu, "max_translation_m": float(max(x[0] for x in d)), "max_rotation_rad": float(max(x[1] for x in d)),
                                                "same_keyframes": bool([u for u in g.update_at if u < n_cpu] == c.update_at), "same_points_kept": bool(g.points_kept[:n_cpu] == c.points_kept),
                                                "same_newton_iterations": bool(g.iterations[:n_cpu] == c.iterations), "cpu_port_ms_per_scan": 1e3 * t_cpu / n_cpu}
    reg.close(); mapper.close()
    return out


def frontend_stream_ref_leg(drive20, dev_index, tstream, torch, args):
    """The frontend loop at the parameter set the reference SHIPS (lidarslam/param/lidarslam.yaml:5-17): ndt_resolution 2.0,
    vg_size_for_input 0.5, vg_size_for_map 0.1, scan range 1.0..200.0 m, num_targeted_cloud 20, trans_for_mapupdate 1.5 — a 20-frame
    window (~1.3 M target points, dense global voxel table) instead of BASELINE's 10 frames at 5 m."""
    from lidarslam_ros2_amd.frontend import FrontendParams

    prm = FrontendParams(vg_size_for_input=0.5, vg_size_for_map=0.1, trans_for_mapupdate=1.5, scan_min_range=1.0, scan_max_range=200.0, num_targeted_cloud=20)
    out = frontend_stream_leg(drive20, dev_index, tstream, torch, args, res=2.0, params=prm, light=True)
    if isinstance(out, dict):
        out["parameter_set"] = "lidarslam/param/lidarslam.yaml scan_matcher"
    return out


def loop_gate_ref_leg(route, dev_index, tstream, torch, synth, args):
    """GraphBasedSlamComponent::searchLoop (graph_based_slam_component.cpp:164-252) at the two parameter sets the reference ships, on a
    route of FULL-SIZE submaps (one VLP-32 revolution at vg_size_for_map 0.1 each, ~65k points; > 100 m of travel between the two visits
    of the start): lidarslam/param/lidarslam.yaml:30-41 — NDT, ndt_resolution 1.0, voxel_leaf_size 0.1, threshold 0.7,
    distance_loop_closure 100, range 20, search_submap_num 2 — and graph_based_slam/param/graphbasedslam.yaml:3-7 — GICP,
    voxel_leaf_size 0.2, threshold 1.5, distance_loop_closure 30 (range 20 and search_submap_num 3: the node's defaults, :37-40).
    parity_vs_cpu: the same gate on the CPU oracle (a bounded leg: one search each)."""
    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint, LoopClosureParams, NormalDistributionsTransform, SubMap, search_loop
    from lidarslam_ros2_amd.posemath import pose_delta

    if route is None:
        return {"skipped": "workload generated without the full-size route"}
    sms = [SubMap(torch.from_numpy(synth.as_pointxyzi(s["cloud"])).cuda(), s["position"], s["orientation"], s["distance"]) for s in route]
    torch.cuda.synchronize()
    sets = {
        "lidarslam_yaml_ndt": (dict(threshold_loop_closure_score=0.7, distance_loop_closure=100.0, range_of_searching_loop_closure=20.0, search_submap_num=2,
                                    voxel_leaf_size=0.1), "ndt"),
        "graphbasedslam_yaml_gicp": (dict(threshold_loop_closure_score=1.5, distance_loop_closure=30.0, range_of_searching_loop_closure=20.0, search_submap_num=3,
                                          voxel_leaf_size=0.2), "gicp"),
    }
    out = {"submaps": len(route), "points_per_submap_median": int(np.median([s["cloud"].shape[0] for s in route])), "route_length_m": float(route[-1]["distance"])}
    for name, (lp, method) in sets.items():
        try:
            if method == "ndt":   # graph_based_slam_component.cpp:64-72
                back = NormalDistributionsTransform(device=dev_index, stream=tstream)
                back.setMaximumIterations(100); back.setResolution(1.0); back.setTransformationEpsilon(0.01)
            else:                 # :74-82
                back = GeneralizedIterativeClosestPoint(device=dev_index, stream=tstream)
                back.setMaxCorrespondenceDistance(30); back.setMaximumIterations(100); back.setTransformationEpsilon(1e-8)
                back.setEuclideanFitnessEpsilon(1e-6); back.setRANSACIterations(0)
            edges = search_loop(back, sms, LoopClosureParams(**lp))
            torch.cuda.synchronize()
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                edges = search_loop(back, sms, LoopClosureParams(**lp))
                ts.append(time.perf_counter() - t0)
            e = edges[0]
            truth = np.linalg.inv(route[e.pair_id[0]]["truth"]) @ route[-1]["truth"]
            et = pose_delta(e.relative_pose, truth)
            r = {"settings": dict(lp, method=method, **({"ndt_resolution": 1.0} if method == "ndt" else {"max_correspondence_distance": 30.0})),
                 "ms_per_search": 1e3 * float(np.median(ts[2:])), "edge": list(e.pair_id), "fitness_score": e.fitness_score, "accepted": e.accepted,
                 "target_points": e.n_target_points, "source_points": int(route[-1]["cloud"].shape[0]), "iterations": e.iterations,
                 "relative_pose_error_vs_truth": {"translation_m": et[0], "rotation_rad": et[1]}}
            if not args.no_cpu:
                from oracle import oracle as O   # the checker, outside every timed region

                t0 = time.perf_counter()
                if method == "ndt":
                    ref = O.search_loop(route, **lp, ndt_resolution=1.0, trans_eps=0.01, max_iterations=100, num_threads=min(64, O.max_threads()))
                else:
                    ref = O.search_loop(route, **lp, method="gicp", gicp_corr_dist=30.0, gicp_trans_eps=1e-8, max_iterations=100, gicp_solver=0, num_threads=min(64, O.max_threads()))
                t_cpu = time.perf_counter() - t0
                o = ref[0]
                d = pose_delta(e.final_transformation, o["final"])
                r["parity_vs_cpu"] = {"same_edge": bool(tuple(e.pair_id) == tuple(o["pair_id"])), "same_target_points": bool(e.n_target_points == o["n_target_points"]),
                                      "same_gate_decision": bool(e.accepted == o["accepted"]), "translation_m": d[0], "rotation_rad": d[1],
                                      "fitness_rel_diff": abs(e.fitness_score - o["fitness_score"]) / max(abs(o["fitness_score"]), 1e-300),
                                      "cpu_port_ms_per_search": 1e3 * t_cpu,
                                      "note": "GICP: the oracle's inner solver is the reference's BFGS, the device runs Gauss-Newton (north_star)" if method == "gicp" else "same schedule"}
            back.close()
            out[name] = r
        except Exception as ex:
            out[name] = {"error": repr(ex)}
    return out


def cfg5_leg(make_ndt, dense, torch, synth):
    from lidarslam_ros2_amd.posemath import pose_delta

    r = make_ndt(eps=0.01, mi=35, resolution=2.0)
    tgt = torch.from_numpy(synth.as_pointxyzi(dense.target)).cuda()
    src = torch.from_numpy(synth.as_pointxyzi(dense.source)).cuda()
    t0 = time.perf_counter(); r.setInputTarget(tgt); t_first = time.perf_counter() - t0
    tt = []
    for _ in range(5):
        t0 = time.perf_counter(); r.setInputTarget(tgt); tt.append(time.perf_counter() - t0)
    ts = []
    for k in range(13):
        t0 = time.perf_counter(); r.setInputSource(src); r.align(dense.guess); dt = time.perf_counter() - t0
        if k >= 3:
            ts.append(dt)
    r.setProfiling(True); r.getProfile(reset=True); r.align(dense.guess); p = r.getProfile(reset=True); r.setProfiling(False)
    e = pose_delta(r.getFinalTransformation(), dense.truth)
    s = lat_stats(ts)
    n_src = int(dense.source.shape[0])
    avg_us = 1e3 * p["deriv_ms_total"] / max(1, p["deriv_launches"])
    alg = n_src * 12 + p["deriv_pairs"] * 40 + ((n_src + 127) // 128) * 224
    s.update({"target_points": int(dense.target.shape[0]), "source_points": n_src, "grid": {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.gridInfo().items()},
              "set_input_target_ms": 1e3 * float(np.median(tt)), "set_input_target_first_ms": 1e3 * t_first,
              "newton_iterations": r.last_result["iterations"], "derivative_passes": r.last_result["n_evaluations"],
              "avg_pass_us": avg_us, "algorithmic_bytes_per_pass": alg, "algorithmic_frac_of_hbm_peak": alg / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
              "valid_pairs_per_pass": int(p["deriv_pairs"]),
              "error_vs_truth": {"translation_m": e[0], "rotation_rad": e[1]},
              "what": "cfg 5: 120000-pt 64-line scan (vg 0.1) vs 20-frame submap, ndt_resolution 2.0, transformation_epsilon 0.01"})
    try:
        pmc = json.load(open(PMC_FILE)).get("cfg5")
    except Exception:
        pmc = None
    if pmc and pmc.get("bytes_per_launch"):
        s.update({"traffic": int(pmc["bytes_per_launch"]), "traffic_kernel": pmc.get("kernel"),
                  "frac_by_traffic": pmc["bytes_per_launch"] / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS})
    # the reference's own demo resolutions on the same clouds: ndt_resolution 1.0 is its backend's
    # (lidarslam/param/lidarslam.yaml:33), 1.5 the tukuba frontend's; 10 fixed iterations each so that the pass count is comparable
    other = {}
    for res_o in (1.0, 1.5):
        try:
            ro = make_ndt(eps=0.0, mi=10, resolution=res_o)
            ro.setInputTarget(tgt)                      # first call: allocations
            tts = []
            for _ in range(3):
                t0 = time.perf_counter(); ro.setInputTarget(tgt); tts.append(time.perf_counter() - t0)
            t_t = float(np.median(tts))
            ro.setInputSource(src)
            ro.align(dense.guess)
            ro.setProfiling(True); ro.getProfile(reset=True); ro.align(dense.guess); po = ro.getProfile(reset=True); ro.setProfiling(False)
            other["res_%g" % res_o] = {"avg_pass_us": 1e3 * po["deriv_ms_total"] / max(1, po["deriv_launches"]), "set_input_target_ms": 1e3 * t_t,
                                       "voxels_valid": ro.gridInfo()["n_valid"], "derivative_passes": ro.last_result["n_evaluations"],
                                       "valid_pairs_per_point": po["deriv_pairs"] / n_src}
            ro.close()
        except Exception as e:
            other["res_%g" % res_o] = {"error": repr(e)}
    s["reference_resolutions"] = other
    return s


def gicp_leg(gc, dev_index, tstream, torch, synth):
    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint
    from lidarslam_ros2_amd.posemath import pose_delta

    gicp = GeneralizedIterativeClosestPoint(device=dev_index, stream=tstream)
    gicp.setMaxCorrespondenceDistance(5.0)
    gicp.setTransformationEpsilon(1e-8)
    g_tgt = torch.from_numpy(synth.as_pointxyzi(gc.target)).cuda()
    g_src = torch.from_numpy(synth.as_pointxyzi(gc.source)).cuda()
    tg = time.perf_counter()
    gicp.setInputTarget(g_tgt)
    gicp.setInputSource(g_src)
    gicp.align(gc.guess)                       # first align also pays the target covariances (K5)
    torch.cuda.synchronize()
    t_first = time.perf_counter() - tg
    ts = []
    for _ in range(12):
        t0 = time.perf_counter()
        gicp.setInputSource(g_src)             # source covariances are recomputed per scan, as in the reference
        gicp.align(gc.guess)
        ts.append(time.perf_counter() - t0)
    gdt, gang = pose_delta(gicp.getFinalTransformation(), gc.truth)
    s = lat_stats(ts[2:])
    # a candidate set with the stand-alone backend's method (graph_based_slam/param/graphbasedslam.yaml:3): 8 GICP registrations
    # against the same target, one after the other and through lsr_align_batch (8 launch chains side by side)
    try:
        from lidarslam_ros2_amd import align_batch

        members = []
        for b in range(8):
            m = GeneralizedIterativeClosestPoint(device=dev_index)       # its own stream
            m.setMaxCorrespondenceDistance(5.0); m.setTransformationEpsilon(1e-8)
            m.shareTargetOf(gicp)
            m.setInputSource(g_src)
            m.align(gc.guess)
            members.append(m)
        guesses = [gc.guess] * 8
        t_serial, t_batch = [], []
        for _ in range(5):
            for m in members:
                m.setInputSource(g_src)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for m in members:
                m.align(gc.guess)
            t_serial.append(time.perf_counter() - t0)
            for m in members:
                m.setInputSource(g_src)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            finals, _ = align_batch(members, guesses)
            t_batch.append(time.perf_counter() - t0)
        same = all(np.array_equal(finals[b], members[b].getFinalTransformation()) for b in range(8))
        s["batch_of_8"] = {"one_by_one_ms": 1e3 * float(np.median(t_serial)), "side_by_side_ms": 1e3 * float(np.median(t_batch)),
                           "speedup": float(np.median(t_serial) / np.median(t_batch)), "poses_equal_the_single_aligns": bool(same),
                           "what": "setInputSource already done; 8 x align (20-NN covariances of the source included) vs lsr_align_batch"}
        for m in members:
            m.close()
    except Exception as e:
        s["batch_of_8"] = {"error": repr(e)}
    s.update({"first_registration_ms_incl_target_setup": 1e3 * t_first, "target_points": int(gc.target.shape[0]),
              "outer_iterations": gicp.last_result["iterations"], "gauss_newton_steps": gicp.last_result["n_evaluations"],
              "correspondences": gicp.last_result["n_correspondences"], "error_vs_truth": {"translation_m": gdt, "rotation_rad": gang},
              "what": "cfg 3: GICP, same 30k scan, target re-filtered at 0.2, corr dist 5.0, eps 1e-8; setInputSource (20-NN covariances) + align"})
    # K6 (correspondence search + pair records) against HBM: counter bytes and kernel time per outer iteration from the PMC
    # passes of tools/pmc_gicp.sh (separate rocprofv3 runs; file committed under profiles/)
    try:
        pg = json.load(open(PMC_GICP_FILE))
        k6 = pg.get("k6_per_outer_iteration")
        if k6 and k6.get("us"):
            s["k6_correspondences"] = {"hbm_bytes_per_outer_iteration": int(k6["bytes"]), "kernel_us_per_outer_iteration": float(k6["us"]),
                                       "achieved_gb_per_s": k6["bytes"] / (k6["us"] * 1e-6) / 1e9,
                                       "frac_of_hbm_peak": k6["bytes"] / (k6["us"] * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                       "bound": "latency (dependent cell probes of the sixteen-lane seeded search; one launch per outer iteration)", "source": pg.get("source")}
    except (OSError, ValueError, KeyError):
        pass
    return s


def next_rows_leg(case, dev_index, tstream, torch, synth, args):
    """SURVEY.md 8f rows N1 / N2 / N4 measured on what the frontend holds BEFORE its preprocessing: the raw source scan and the ten
    keyframe clouds of the cfg-1/2 submap.  N1+N4: range filter + VoxelGrid(0.2) + setInputSource from the PointCloud2 payload
    (scanmatcher_component.cpp:201-218,324-329) — payload resident in HBM, and from a host payload (PCIe-inclusive); the
    toROSMsg direction.  N2: transformPointCloud x 10 + concatenation + setInputTarget (:449-464,307) against setInputTarget of
    the already assembled submap.  The CPU figures are the oracle's restatements on one thread (bounded: a few calls)."""
    from lidarslam_ros2_amd import NormalDistributionsTransform

    if case.raw_source is None or case.frames is None:
        return {"skipped": "workload generated without its parts"}
    out = {}
    med = lambda ts: 1e3 * float(np.median(ts))
    ndt = NormalDistributionsTransform(device=dev_index, stream=tstream)
    ndt.setResolution(5.0)
    raw = synth.as_pointxyzi(case.raw_source)                       # (n, 8) fp32 = pcl::PointXYZI records, intensity 0
    n_raw = int(raw.shape[0])
    raw_dev = torch.from_numpy(raw).cuda()
    payload_host = raw.view(np.uint8).reshape(n_raw, 32)
    payload_dev = torch.from_numpy(payload_host.copy()).cuda()
    torch.cuda.synchronize()
    rmin, rmax, leaf = 0.1, 100.0, 0.2                              # scan_min_range / scan_max_range / vg_size_for_input (scanmatcher_component.cpp:42-45)

    def timed(fn, reps=15, warm=3):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); r = fn(); ts.append(time.perf_counter() - t0)
        return med(ts), r

    # the filtered-source entries return when the caller's buffer has been read and the count is known; the centroid launch may still
    # be running (a following align starts under it).  Timed here to the END of the device work: a device synchronisation inside the clock
    def done(v):
        torch.cuda.synchronize()
        return v

    t_dev, n_kept = timed(lambda: done(ndt.setInputSourceFrontend(raw_dev, rmin, rmax, leaf)))
    t_pc2_dev, n_kept2 = timed(lambda: done(ndt.setInputSourcePointCloud2(payload_dev, n_raw, 32, (0, 4, 8, 16), rmin, rmax, leaf)))
    t_pc2_host, _ = timed(lambda: done(ndt.setInputSourcePointCloud2(payload_host, n_raw, 32, (0, 4, 8, 16), rmin, rmax, leaf)))
    t_pc2_ret, _ = timed(lambda: ndt.setInputSourcePointCloud2(payload_dev, n_raw, 32, (0, 4, 8, 16), rmin, rmax, leaf))
    torch.cuda.synchronize()
    t_get, back = timed(lambda: ndt.getInputSourcePointCloud2())
    bytes_n1 = n_raw * 16 + int(n_kept) * 16
    out["source_preprocess"] = {"raw_points": n_raw, "points_kept": int(n_kept), "pc2_points_kept": int(n_kept2),
                                "ms_device_records": t_dev, "ms_device_pointcloud2_payload": t_pc2_dev,
                                "ms_device_payload_call_returns": t_pc2_ret,
                                "ms_host_pointcloud2_payload_pcie_inclusive": t_pc2_host, "ms_get_source_pointcloud2_to_host": t_get,
                                "algorithmic_GBps_device_payload": bytes_n1 / (t_pc2_dev * 1e-3) / 1e9,
                                "what": "range filter [0, 100 m] + VoxelGrid(0.2) incl. intensity + setInputSource (N1 + N4)"}
    # N2: submap assembly on the device
    frames_dev = [torch.from_numpy(synth.as_pointxyzi(f)).cuda() for f in case.frames]
    tgt_dev = torch.from_numpy(synth.as_pointxyzi(case.target)).cuda()
    torch.cuda.synchronize()
    t_frames, _ = timed(lambda: ndt.setInputTargetFrames(frames_dev, case.frame_poses), reps=12)
    grid_frames = ndt.gridInfo()
    t_plain, _ = timed(lambda: ndt.setInputTarget(tgt_dev), reps=12)
    grid_plain = ndt.gridInfo()
    n_t = int(case.target.shape[0])
    out["submap_assembly"] = {"frames": len(case.frames), "target_points": n_t, "ms_frames_to_voxel_grid": t_frames,
                              "ms_assembled_cloud_to_voxel_grid": t_plain, "ms_assembly_alone": t_frames - t_plain,
                              "same_voxel_grid": bool(grid_frames["n_valid"] == grid_plain["n_valid"] and
                                                      np.array_equal(grid_frames["min_b"], grid_plain["min_b"])),
                              "assembly_GBps": (n_t * (32 + 12)) / (max(t_frames - t_plain, 1e-6) * 1e-3) / 1e9,
                              "what": "10 x transformPointCloud + concatenation + setInputTarget from HBM-resident keyframes (N2)"}
    if not args.no_cpu:
        from oracle import oracle as O

        t0 = time.perf_counter()
        r64 = np.sqrt(case.raw_source[:, 0].astype(np.float64) ** 2 + case.raw_source[:, 1].astype(np.float64) ** 2)
        kept = case.raw_source[(rmin < r64) & (r64 < rmax)]          # the reference's test: horizontal range, open interval
        v = O.voxel_grid_filter_xyzi(synth.as_pointxyzi(kept), leaf, 4)
        t_cpu = time.perf_counter() - t0
        got = back.view(np.float32).reshape(-1, 8)[:, [0, 1, 2, 4]]
        out["source_preprocess"]["cpu_port_ms"] = 1e3 * t_cpu
        out["source_preprocess"]["parity_vs_cpu"] = {"same_count": bool(v.shape[0] == got.shape[0]),
                                                     "max_abs_diff": float(np.abs(v - got).max()) if v.shape == got.shape else None}
    ndt.close()
    return out


def loop_gate_leg(dev_index, tstream, torch, synth, stash):
    from lidarslam_ros2_amd import LoopClosureParams, NormalDistributionsTransform, SubMap, search_loop

    route = synth.make_loop_route()
    stash["route"] = route
    sms = [SubMap(torch.from_numpy(synth.as_pointxyzi(s["cloud"])).cuda(), s["position"], s["orientation"], s["distance"]) for s in route]
    lp = dict(threshold_loop_closure_score=1.0, distance_loop_closure=20.0, range_of_searching_loop_closure=10.0, search_submap_num=2,
              voxel_leaf_size=0.2)
    stash["lp"] = lp
    back = NormalDistributionsTransform(device=dev_index, stream=tstream)   # graph_based_slam_component.cpp:64-72
    back.setMaximumIterations(100)
    back.setResolution(5.0)
    back.setTransformationEpsilon(0.01)
    edges = search_loop(back, sms, LoopClosureParams(**lp))
    torch.cuda.synchronize()
    ts = []
    for _ in range(12):
        t0 = time.perf_counter()
        edges = search_loop(back, sms, LoopClosureParams(**lp))
        ts.append(time.perf_counter() - t0)
    stash["edges"] = edges
    return {"ms_per_search": 1e3 * float(np.median(ts[2:])), "submaps": len(route), "edge": list(edges[0].pair_id),
            "fitness_score": edges[0].fitness_score, "accepted": edges[0].accepted, "target_points": edges[0].n_target_points,
            "source_points": int(route[-1]["cloud"].shape[0]), "newton_iterations": edges[0].iterations,
            "what": "source transform + 5-submap window transform/concat + VoxelGrid(0.2) + setInputTarget + align + getFitnessScore "
                    "+ gate, clouds resident in HBM"}


def run_cfg4(args, lib, rank, world, dev_index, tstream, cands, dist, world_comm, torch, synth):
    """BASELINE cfg 4 as SURVEY.md §8d defines it: every candidate is its own (target, source, guess) and pays
    setInputTarget + setInputSource + align + getFitnessScore (graph_based_slam_component.cpp:181-231, backend settings
    max_iterations 100, transformation_epsilon 0.01, :64-72).  Candidates are sharded over the ranks (lsr_shard_range) and the
    64-byte result records all-gathered through the C ABI (lsr_align_batch_sharded: ncclAllGather over xGMI; on ranks that
    share a device the gather goes through the host)."""
    from lidarslam_ros2_amd import NormalDistributionsTransform, _capi
    from lidarslam_ros2_amd.posemath import pose_delta

    n_total = args.candidates
    fptr = C.POINTER(C.c_float)
    regs, tgts, srcs, guesses = [], [], [], []
    for c, target, source, guess, truth in cands:
        r = NormalDistributionsTransform(device=dev_index)     # its own stream: the staged batch entries overlap the candidates
        r.setResolution(5.0); r.setTransformationEpsilon(0.01); r.setMaximumIterations(100)
        regs.append(r)
        tgts.append(torch.from_numpy(synth.as_pointxyzi(target)).cuda())
        srcs.append(torch.from_numpy(synth.as_pointxyzi(source)).cuda())
        guesses.append(np.ascontiguousarray(np.asarray(guess, np.float32).T).reshape(16))
    torch.cuda.synchronize()
    nloc = len(regs)
    # the job's communicator (make_comm) when there is more than one rank; else a one-rank communicator (no RCCL behind it)
    comm = C.c_void_p()
    use_rccl = (world > 1 and world_comm is not None)
    if use_rccl:
        comm = world_comm
    else:
        _capi.check(lib.lsr_comm_create(None, 0, 1, dev_index, C.byref(comm)), "lsr_comm_create")   # one-rank communicator per process
    hs = (C.c_void_p * max(nloc, 1))(*[r._h for r in regs])
    G = np.ascontiguousarray(np.stack(guesses), np.float32) if nloc else np.zeros((1, 16), np.float32)
    n_rec = n_total if use_rccl else nloc
    recs = (_capi.ShardRecord * max(n_rec, 1))()

    tptr = (C.c_void_p * max(nloc, 1))(*[C.c_void_p(t.data_ptr()) for t in tgts])
    tcnt = (C.c_size_t * max(nloc, 1))(*[int(t.shape[0]) for t in tgts])
    sptr = (C.c_void_p * max(nloc, 1))(*[C.c_void_p(t.data_ptr()) for t in srcs])
    scnt = (C.c_size_t * max(nloc, 1))(*[int(t.shape[0]) for t in srcs])

    def one_round(batched: bool):
        """-> seconds for this rank's share; fills recs.  batched: the staged C-ABI entries (lsr_set_input_target_batch, the
        shared launch chain, lsr_get_fitness_score_batch inside lsr_align_batch_sharded); else the reference's loop, one
        candidate after the other."""
        t0 = time.perf_counter()
        if batched and nloc:
            _capi.check(lib.lsr_set_input_target_batch(hs, nloc, tptr, tcnt, 32, 1), "lsr_set_input_target_batch")
            _capi.check(lib.lsr_set_input_source_batch(hs, nloc, sptr, scnt, 32, 1), "lsr_set_input_source_batch")
        for b, (r, t, s) in enumerate(zip(regs, tgts, srcs)):
            if not batched:
                _capi.check(lib.lsr_set_input_target_device(r._h, C.c_void_p(t.data_ptr()), 32, int(t.shape[0])), "setInputTarget")
                _capi.check(lib.lsr_set_input_source_device(r._h, C.c_void_p(s.data_ptr()), 32, int(s.shape[0])), "setInputSource")
            if not batched:
                fin = np.zeros(16, np.float32)
                _capi.check(lib.lsr_align(r._h, guesses[b].ctypes.data_as(fptr), fin.ctypes.data_as(fptr), C.byref(r._last), None, 0), "align")
                f = C.c_double()
                _capi.check(lib.lsr_get_fitness_score(r._h, 1.7976931348623157e308, C.byref(f)), "getFitnessScore")
        if batched:
            if use_rccl:
                _capi.check(lib.lsr_align_batch_sharded(comm, hs, nloc, n_total, G.ctypes.data_as(fptr), 1, recs), "lsr_align_batch_sharded")
            elif nloc:
                _capi.check(lib.lsr_align_batch_sharded(comm, hs, nloc, nloc, G.ctypes.data_as(fptr), 1, recs), "lsr_align_batch_sharded")
        return time.perf_counter() - t0

    def sync_max(t):
        if dist is None:
            return t
        v = torch.tensor([t], dtype=torch.float64)
        dist.all_reduce(v, op=dist.ReduceOp.MAX)   # control plane (gloo)
        return float(v.item())

    one_round(True)   # warm-up (allocations, RCCL channels)
    if dist is not None:
        dist.barrier()
    t_batched = sync_max(min(one_round(True) for _ in range(3)))
    t_serial = sync_max(min(one_round(False) for _ in range(2))) if world == 1 else None
    if world == 1 and nloc:   # one input, one answer: the one-by-one loop (quad kernel) against the staged batch (lane kernel)
        serial_T = []
        for r in regs:
            fin = np.zeros(16, np.float32)
            _capi.check(lib.lsr_get_final_transformation(r._h, fin.ctypes.data_as(fptr)), "getFinalTransformation")
            serial_T.append(fin.copy())
    one_round(True)
    extra = {}
    if world == 1 and nloc:
        same = 0
        for b, r in enumerate(regs):
            fin = np.zeros(16, np.float32)
            _capi.check(lib.lsr_get_final_transformation(r._h, fin.ctypes.data_as(fptr)), "getFinalTransformation")
            same += int(np.array_equal(fin, serial_T[b]))
        extra["same_bits_as_one_by_one"] = {"candidates": nloc, "identical_final_transformations": same}
        try:
            extra["chain_roofline"] = cfg4_chain_roofline(lib, regs, hs, nloc, G, srcs, fptr)
        except Exception as e:   # never lose the line to a diagnostic leg
            extra["chain_roofline"] = {"error": repr(e)}
        try:
            extra["projected_8gpu"] = cfg4_projected_8gpu(lib, dev_index, regs, tgts, srcs, G, t_batched, fptr)
        except Exception as e:
            extra["projected_8gpu"] = {"error": repr(e)}
        one_round(True)   # leave the records of the full set in `recs` for the parity block below
    # parity sanity on this rank's share: registered pose vs ground truth
    errs = []
    for b, (c, target, source, guess, truth) in enumerate(cands):
        rr = recs[(cands[0][0] if use_rccl else 0) + b]
        T = np.eye(4); T[:3, :4] = np.asarray(rr.T, np.float64).reshape(3, 4)
        errs.append(pose_delta(T, truth))
    if not use_rccl:
        lib.lsr_comm_destroy(comm)
    if rank != 0:
        return None
    res = {"candidates": n_total, "ranks": world, "candidates_on_rank0": nloc,
           "value": n_total / t_batched, "unit": "registrations/s", "ms_per_candidate_set": 1e3 * t_batched,
           "collective": ("ncclAllGather of 64-byte records (lsr_align_batch_sharded)" if use_rccl else
                          "none (one rank)" if world == 1 else "per-rank tables only: the library's communicator could not be created"),
           "max_error_vs_truth_rank0": {"translation_m": float(max(e[0] for e in errs)) if errs else None,
                                        "rotation_rad": float(max(e[1] for e in errs)) if errs else None},
           "fitness_rank0": [float(recs[(cands[0][0] if use_rccl else 0) + b].fitness) for b in range(min(nloc, 4))],
           "iterations_rank0": [int(recs[(cands[0][0] if use_rccl else 0) + b].iterations) for b in range(nloc)],
           "what": "per candidate: setInputTarget (661k-pt submap -> voxel grid) + setInputSource + align (max_iterations 100, eps 0.01) + "
                   "getFitnessScore; all candidates of a rank advance in shared launches (lsr_align_batch)"}
    # every candidate rank 0 holds a record for, against the committed CPU-oracle fixture (tests/golden/make_cfg4_fixture.py)
    fx_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "cfg4_candidates_oracle.npz")
    if os.path.exists(fx_path) and nloc:
        fx = np.load(fx_path)
        first = cands[0][0]
        idxs = list(range(n_total)) if use_rccl else [first + b for b in range(nloc)]
        dts, angs, fits, it_equal, outliers = [], [], [], True, {}
        for c in idxs:
            if c >= fx["final"].shape[0]:
                continue
            rr = recs[c if use_rccl else c - first]
            T = np.eye(4); T[:3, :4] = np.asarray(rr.T, np.float64).reshape(3, 4)
            dt, ang = pose_delta(T, fx["final"][c])
            dts.append(dt); angs.append(ang)
            if dt > 1e-3 or ang > 1e-4:
                outliers[str(c)] = {"translation_m": float(dt), "rotation_rad": float(ang), "newton_iterations": int(rr.iterations)}
            it_equal = it_equal and int(rr.iterations) == int(fx["iterations"][c])
            fits.append(abs(float(rr.fitness) - float(fx["fitness"][c])) / float(fx["fitness"][c]))
        try:   # the CPU path's own spread on the candidates listed as beyond the bar
            fxt = np.load(os.path.join(ROOT, "tests", "golden", "cfg4_candidates_oracle_tight.npz"))
            for c in outliers:
                outliers[c]["cpu_spread_translation_m"] = float(fxt["cpu_spread_translation_m"][int(c)])
                outliers[c]["cpu_spread_rotation_rad"] = float(fxt["cpu_spread_rotation_rad"][int(c)])
        except (OSError, KeyError):
            pass
        if dts:
            res["vs_cpu_oracle_fixture"] = {"candidates_checked": len(dts), "max_translation_m": float(max(dts)),
                                            "max_rotation_rad": float(max(angs)), "newton_iterations_all_equal": bool(it_equal),
                                            "max_fitness_rel_diff": float(max(fits)),
                                            "within_1e-3m_1e-4rad": len(dts) - len(outliers), "beyond": outliers,
                                            "note": "eps 0.01 (the backend's schedule), staged batch path; the one-by-one path returns the same bits "
                                                    "(same_bits_as_one_by_one).  Round 3's 1.4 mm outlier (candidate 34) was the compiler fusing the point "
                                                    "transform differently in two kernels, not conditioning (DESIGN.md 2)",
                                            "fixture": "tests/golden/cfg4_candidates_oracle.npz (CPU oracle, all 64 candidates)"}
    if t_serial is not None:
        res["serial_one_by_one"] = {"value": n_total / t_serial, "unit": "registrations/s", "ms_per_candidate_set": 1e3 * t_serial}
    res.update(extra)
    return res


def cfg4_chain_roofline(lib, regs, hs, nloc, G, srcs, fptr):
    """The fed-chip roofline: the shared launch chain of the candidate set on its own — targets and sources
    resident, lsr_align_batch with the lead object's profiling on: hipEvents on the lead's stream from before the state uploads
    to the point where it has joined the set's launch chains (a set of six or more members runs as two chains on two streams).  Algorithmic bytes = sum over members of passes x (N x 12 + pairs x 40)
    + launches x workgroups x 256; priced against 8 TB/s.  The whole chain is priced, its thin tail (few members still running)
    included — the launches in which all 64 members are active run at the `full_load` figure of profiles/r04_*cfg4*."""
    from lidarslam_ros2_amd import _capi
    lead = regs[0]
    finals = np.zeros((nloc, 16), np.float32)
    res = (_capi.Result * nloc)()
    best = None
    for rep in range(4):
        lead.setProfiling(True); lead.getProfile(reset=True)
        _capi.check(lib.lsr_align_batch(hs, nloc, G.ctypes.data_as(fptr), finals.ctypes.data_as(fptr), res), "lsr_align_batch")
        prof = lead.getProfile(reset=True); lead.setProfiling(False)
        if rep and (best is None or prof["deriv_ms_total"] < best[0]["deriv_ms_total"]):
            best = (prof, [(int(r.n_evaluations), int(r.n_correspondences)) for r in res])
    prof, per = best
    n_pts = [int(t.shape[0]) for t in srcs]
    member_passes = sum(e for e, _ in per)
    alg = sum(e * (n * 12 + p * 40) for (e, p), n in zip(per, n_pts)) + prof["deriv_launches"] * 512 * 256
    ms = prof["deriv_ms_total"]
    achieved = alg / (ms * 1e-3) / 1e9
    return {"kernel": "ndt_eval_lane_kernel<7, LDS table, 512> (one lane per point, the set's two launch chains)",
            "members": nloc, "launches": prof["deriv_launches"], "member_passes": member_passes, "chain_ms": ms,
            "us_per_member_pass": 1e3 * ms / member_passes, "algorithmic_bytes": alg,
            "achieved": achieved, "unit": "GB/s",
            "mean_valid_pairs_per_point": sum(p for _, p in per) / max(1, sum(n_pts)),
            "note": "hipEvents on the lead object's stream around the set's launch chains as production runs them (two chains on two streams: "
                    "before the state uploads -> both chains joined), best of 3; bytes per SURVEY.md 8d"}


def cfg4_projected_8gpu(lib, dev_index, regs, tgts, srcs, G, t_set, fptr):
    """What ONE GPU can say about the 8-GPU figure: the eight shares of the 64-candidate set an 8-GPU node
    would run side by side — the static block partition and the cost-aware longest-first plan (costs = point visits) — are run one
    after the other here, each through the whole per-candidate path (lsr_set_input_target_batch, lsr_set_input_source_batch,
    lsr_align_batch_sharded with a one-rank communicator and fitness).  64-set time / slowest share = the scaling an 8-GPU node
    could reach before its (4 KiB, latency-bound) all-gather; a projection from single-GPU measurements, not a scaling run."""
    from lidarslam_ros2_amd import _capi
    n, world = len(regs), 8
    if n < world:
        return {"skipped": "fewer candidates than shares"}
    comm = C.c_void_p()
    _capi.check(lib.lsr_comm_create(None, 0, 1, dev_index, C.byref(comm)), "lsr_comm_create")
    cost = (C.c_double * n)(*[6.0 * int(t.shape[0]) + 34.0 * int(s.shape[0]) for t, s in zip(tgts, srcs)])
    owner, order, first = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int32 * (world + 1))()
    _capi.check(lib.lsr_shard_plan(n, cost, world, owner, order, first), "lsr_shard_plan")
    plans = {"block": [list(range(*(lambda f, c: (f, f + c))(*_shard_range(lib, n, world, r)))) for r in range(world)],
             "planned_longest_first": [[int(order[k]) for k in range(first[r], first[r + 1])] for r in range(world)]}
    out = {}
    for name, shares in plans.items():
        times = []
        for share in shares:
            m = len(share)
            if m == 0:
                times.append(0.0); continue
            hs = (C.c_void_p * m)(*[regs[i]._h for i in share])
            tp = (C.c_void_p * m)(*[C.c_void_p(tgts[i].data_ptr()) for i in share]); tc = (C.c_size_t * m)(*[int(tgts[i].shape[0]) for i in share])
            sp = (C.c_void_p * m)(*[C.c_void_p(srcs[i].data_ptr()) for i in share]); sc = (C.c_size_t * m)(*[int(srcs[i].shape[0]) for i in share])
            g = np.ascontiguousarray(G[share])
            recs = (_capi.ShardRecord * m)()
            best = None
            for rep in range(7):   # the first is a warm-up; best of six (a share is ~1 ms: one preempted call must not set the slowest share)
                t0 = time.perf_counter()
                _capi.check(lib.lsr_set_input_target_batch(hs, m, tp, tc, 32, 1), "t")
                _capi.check(lib.lsr_set_input_source_batch(hs, m, sp, sc, 32, 1), "s")
                _capi.check(lib.lsr_align_batch_sharded(comm, hs, m, m, g.ctypes.data_as(fptr), 1, recs), "a")
                dt = time.perf_counter() - t0
                if rep and (best is None or dt < best):
                    best = dt
            times.append(best)
        out[name] = {"share_ms": [round(1e3 * t, 4) for t in times], "max_share_ms": 1e3 * max(times), "mean_share_ms": 1e3 * sum(times) / len(times),
                     "set_ms_on_one_gpu": 1e3 * t_set, "projected_speedup_8_gpus": t_set / max(times)}
    lib.lsr_comm_destroy(comm)
    out["plan_is_the_block_partition"] = bool(plans["block"] == plans["planned_longest_first"])
    out["note"] = ("shares run one after the other on ONE GPU; projected_speedup = 64-set time on one GPU / slowest share, before the 4 KiB "
                   "all-gather (~0.03 ms).  north_star asks >= 6x at 8 GPUs.  The candidates of cfg 4 differ by a few hundred target points in "
                   "661 k: costs within 2 % of each other are ties for lsr_shard_plan, whose plan is then the block partition (the two rows "
                   "differ by measurement noise only)")
    return out


def _shard_range(lib, n, world, r):
    f, c = C.c_int(), C.c_int()
    lib.lsr_shard_range(n, world, r, C.byref(f), C.byref(c))
    return f.value, c.value


def cpu_leg(args, out, stash, case, stream, j_last, gpu_final, res, max_iter):
    """CPU baseline: the oracle (restatement of ndt_omp) on this box's host cores, bounded sample of the SAME workload (the last
    timed scan of the stream against the same submap); also the parity of the GPU pose against it."""
    from oracle import oracle as O
    from lidarslam_ros2_amd.posemath import pose_delta

    src, guess = stream[j_last][0], stream[j_last][1]
    g = O.VoxelGridCovariance(case.target, res)
    avail = min(len(os.sched_getaffinity(0)), O.max_threads())
    p0 = O.matrix_to_pose(guess)
    cores, best = 1, float("inf")
    cands = [args.cpu_threads] if args.cpu_threads else [c for c in (1, 2, 4, 8, 16, 32, 64, 128) if c <= avail]
    for c in cands:  # pick the thread count that is fastest on THIS box (oversubscribed hosts get slower with more)
        O.ndt_derivatives(g, src, p0, resolution=res, num_threads=c)
        tq = time.perf_counter()
        for _ in range(2):
            O.ndt_derivatives(g, src, p0, resolution=res, num_threads=c)
        tq = (time.perf_counter() - tq) / 2
        if tq < best:
            cores, best = c, tq
    # bounded sample: whole registrations of the same workload — a warm-up + 5 at the fastest thread count (median),
    # ONE at a single thread; about 15-25 s of CPU work in all
    def whole(threads):
        tq = time.perf_counter()
        r = O.ndt_align(g, src, guess, resolution=res, trans_eps=0.0, max_iterations=max_iter, num_threads=threads)
        return time.perf_counter() - tq, r
    whole(cores)
    runs = [whole(cores) for _ in range(5)]
    t_all = [t for t, _ in runs]
    ref = runs[-1][1]
    t_one, ref1 = whole(1)
    n_par = ref["n_evals"] + ref["n_evals_grad"]        # passes of the OpenMP-parallel computeDerivatives
    n_hess = ref["n_hessian_recompute"]                 # computeHessian after a line search: fp64 per pair, NOT parallel (as in ndt_omp)
    # the pieces, each on its own: a parallel pass with / without Hessian, the sequential computeHessian
    def piece(with_h, fp64_h, threads, reps=3):
        O.ndt_derivatives(g, src, p0, resolution=res, compute_hessian=with_h, fp64_hessian=fp64_h, num_threads=threads)
        tq = time.perf_counter()
        for _ in range(reps):
            O.ndt_derivatives(g, src, p0, resolution=res, compute_hessian=with_h, fp64_hessian=fp64_h, num_threads=threads)
        return (time.perf_counter() - tq) / reps
    t_pass_h, t_pass_g = piece(True, False, cores), piece(False, False, cores)
    t_hess_seq = max(0.0, piece(True, True, cores) - t_pass_h)
    predicted = ref["n_evals"] * t_pass_h + ref["n_evals_grad"] * t_pass_g + n_hess * t_hess_seq
    med = float(np.median(t_all))
    dt, ang = pose_delta(gpu_final, ref["final"])
    out["cpu_baseline"] = {"value": 1.0 / med, "unit": "registrations/s", "cores": cores, "kind": "port",
                           "sample": f"median of 5 whole registrations (after one warm-up) of the same workload: the last timed scan of the stream "
                                     f"({ref['iterations']} Newton iterations, {n_par} parallel derivative passes + {n_hess} sequential computeHessian each)",
                           "seconds": float(sum(t_all) + t_one), "ms_per_registration": 1e3 * med,
                           "ms_per_registration_p10_p90": [1e3 * pct(t_all, 10), 1e3 * pct(t_all, 90)],
                           "newton_iterations": ref["iterations"], "host_threads_available": avail,
                           "cores_choice": f"the fastest of {cands} threads for one derivative pass on this box (timed above): more threads than "
                                           f"that are slower here (the pass is 30k points; beyond {cores} threads OpenMP's fork/join and the guided "
                                           "schedule cost more than they divide)",
                           "one_thread": {"value": 1.0 / t_one, "ms_per_registration": 1e3 * t_one, "registrations": 1},
                           "reconciliation": {"ms_parallel_pass_with_hessian": 1e3 * t_pass_h, "ms_parallel_pass_gradient_only": 1e3 * t_pass_g,
                                              "ms_sequential_computeHessian": 1e3 * t_hess_seq, "passes_with_hessian": ref["n_evals"],
                                              "passes_gradient_only": ref["n_evals_grad"], "computeHessian_calls": n_hess,
                                              "ms_predicted_from_the_pieces": 1e3 * predicted, "ms_measured": 1e3 * med,
                                              "ms_unexplained": 1e3 * (med - predicted),
                                              "unexplained_is": "the pieces are timed back to back at ONE pose (the guess) with warm caches; the registration "
                                                                "alternates parallel passes with the sequential fp64 computeHessian (which evicts the voxel map "
                                                                "from the cores' caches between them) and visits poses with more pairs per point than the guess",
                                              "note": "ndt_omp's computeHessian (after every line search that took a trial) is a plain fp64 loop over "
                                                      "all points, not OpenMP-parallel; with many threads it is most of a registration"},
                           "ms_per_derivative_pass": 1e3 * best,
                           "note": "C++/OpenMP restatement of ndt_omp (oracle/, built -O2 without -march=native like the reference's own -O2 -g), "
                                   "not ndt_omp itself; a reported baseline, not the target.  Most of a CPU registration at this thread count is "
                                   "ndt_omp's SEQUENTIAL computeHessian (reconciliation): the GPU evaluates the same Hessian inside the parallel pass, "
                                   "so the GPU / CPU ratio of this line says more about that loop than about the kernels"}
    out["parity_vs_cpu"] = {"translation_m": dt, "rotation_rad": ang, "gpu_iterations": out["config"]["newton_iterations"],
                            "cpu_iterations": ref["iterations"]}
    route, lp, edges = stash.get("route"), stash.get("lp"), stash.get("edges")
    if route is not None and "error" not in out.get("loop_gate", {"error": 1}):
        tq = time.perf_counter()
        ref_edges = O.search_loop(route, **lp, ndt_resolution=5.0, trans_eps=0.01, max_iterations=100, num_threads=cores)
        tq = time.perf_counter() - tq
        ldt, lang = pose_delta(edges[0].relative_pose, ref_edges[0]["relative_pose"])
        out["loop_gate"]["cpu_port_ms_per_search"] = 1e3 * tq
        out["loop_gate"]["parity_vs_cpu"] = {"same_edge": list(ref_edges[0]["pair_id"]) == list(edges[0].pair_id), "translation_m": ldt,
                                             "rotation_rad": lang}


if __name__ == "__main__":
    main()

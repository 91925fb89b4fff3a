"""The frontend with registration_method "GICP" (scanmatcher_component.cpp:115-120) on the gfx950 core: every map update puts the
assembled window (newest keyframe first, :448-464) through VoxelGrid(vg_size_for_input) before setInputTarget (:308-316) and the scans
register against that filtered cloud (:329,353).  Here: the filtered-frames target is the composition it claims to be, a prepared
target is prepared (the covariances the reference computes lazily inside align are there at the hand-over), and the whole stream —
preprocessing, registration, map assembly, filter — holds the north_star bar against the CPU oracle on every scan.

trans_for_mapupdate is 1.25 m, not the default 1.5: the drive takes a scan every 0.5 m, so with 1.5 m the keyframe decisions sit
within millimetres of the threshold (-0.0003 .. +0.0017 m on the oracle) and two GICP pipelines that agree to 1e-4 m take different
ones; with 1.25 m every decision has at least 0.24 m of margin.  The oracle runs Gauss-Newton (solver=1), the optimiser the core
runs: the reference's BFGS schedule stops on a gradient tolerance of 1e-2 and is itself up to 7e-3 m away from Gauss-Newton on this
workload, so its difference is printed, not asserted."""
import numpy as np
import pytest

from lidarslam_ros2_amd import synth
from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload, _records
from lidarslam_ros2_amd.posemath import pose_delta

pytestmark = pytest.mark.gpu

N_SCANS = 24   # eight map updates
LEAF = 0.2     # vg_size_for_input


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def drive():
    import multiprocessing as mp
    import os

    with mp.get_context("spawn").Pool(min(32, len(os.sched_getaffinity(0)))) as p:
        return synth.cfg_frontend_drive(N_SCANS, pool=p)


def _gicp():
    from lidarslam_ros2_amd import GeneralizedIterativeClosestPoint

    g = GeneralizedIterativeClosestPoint(device=0)   # its own stream
    g.setMaxCorrespondenceDistance(5.0)              # scanmatcher_component.cpp:118
    g.setTransformationEpsilon(1e-8)                 # :119
    return g


def _params():
    return FrontendParams(registration_method="GICP", trans_for_mapupdate=1.25)


def _replay(reg, drive, device_payloads=False, mapper=None, builder=None, async_update=False, swap_lag=0, prepared=None):
    """-> (FrontendResult, target points after initialise and after every update).  prepared: a list that receives
    reg.targetPrepared() right after every hand-over."""
    import torch

    to_device = (lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()) if device_payloads else None
    fr = FrontendReplay(reg, _params(), to_device=to_device, mapper=mapper, builder=builder, async_update=async_update, swap_lag=swap_lag)
    sizes = []
    set_target = fr._set_target

    def set_target_and_count():
        set_target()
        obj = fr.builder or fr.reg
        sizes.append(int(obj._n_target) if hasattr(obj, "_n_target") else int(obj.target_sizes[-1]))

    fr._set_target = set_target_and_count
    if prepared is not None:
        hand_over = fr._hand_over

        def hand_over_and_look():
            hand_over()
            prepared.append(bool(fr.reg.targetPrepared()))

        fr._hand_over = hand_over_and_look
    fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
    out = FrontendResult()
    for scan in drive["scans"]:
        host = as_pc2_payload(scan)
        payload = torch.from_numpy(host).cuda() if device_payloads else host
        fr.receive_cloud(payload, int(scan.shape[0]), out, payload_host=host)
    fr.finish(out)
    return out, sizes


def _window(drive):
    """The drive's ten keyframes as the frontend hands them over: newest first, (m,8) fp32 records, with their poses."""
    frames = [_records(as_pc2_payload(f)) for f in drive["frames"]][::-1]
    poses = [np.asarray(P, np.float64) for P in drive["frame_poses"]][::-1]
    return frames, poses


def _source(O, drive):
    return O.voxel_grid_filter(np.ascontiguousarray(drive["scans"][0], np.float32), LEAF)


@pytest.mark.parametrize("resident", [False, True], ids=["host_records", "cuda_tensors"])
def test_filtered_frames_target_is_assembly_then_voxelgrid_then_set_input_target(O, drive, resident):
    import torch

    frames, poses = _window(drive)
    assembled = np.concatenate([O.transform_point_cloud(f[:, :3], np.asarray(P, np.float32)) for f, P in zip(frames, poses)])
    given = [torch.from_numpy(f).cuda() for f in frames] if resident else frames
    src, guess = _source(O, drive), np.asarray(drive["guess0"], np.float32)

    a, b = _gicp(), _gicp()
    n_a = a.setInputTargetFramesFiltered(given, poses, LEAF)
    filtered = b.voxelGridFilter(assembled, LEAF)
    b.setInputTarget(filtered)
    assert n_a == filtered.shape[0] == O.voxel_grid_filter(assembled, LEAF).shape[0]
    results = []
    for g in (a, b):
        g.setInputSource(src)
        g.align(guess)
        results.append((g.covariances("target"), g.nearestNeighbors(), g.getFinalTransformation()))
    (cov_a, nn_a, T_a), (cov_b, nn_b, T_b) = results
    assert np.array_equal(cov_a, cov_b)
    assert np.array_equal(nn_a[0], nn_b[0]) and np.array_equal(nn_a[1], nn_b[1])
    assert np.array_equal(T_a, T_b)
    # the same call again on the same object: the one-launch assembly left the bounding box on the device and the first call the
    # key width, so the filter works out its dimensions on the device (one host wait) — and returns the same cloud
    assert a.setInputTargetFramesFiltered(given, poses, LEAF) == n_a
    assert a.voxelFilterForm() == 2
    a.align(guess)
    assert np.array_equal(a.covariances("target"), cov_a) and np.array_equal(a.getFinalTransformation(), T_a)
    nn_again = a.nearestNeighbors()
    assert np.array_equal(nn_again[0], nn_a[0]) and np.array_equal(nn_again[1], nn_a[1])


def test_filtered_frames_target_of_an_ndt_object_is_the_grid_of_the_filtered_cloud(O, drive):
    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform

    frames, poses = _window(drive)
    assembled = np.concatenate([O.transform_point_cloud(f[:, :3], np.asarray(P, np.float32)) for f, P in zip(frames, poses)])
    a, b = NormalDistributionsTransform(device=0), NormalDistributionsTransform(device=0)
    for r in (a, b):
        r.setResolution(5.0); r.setNeighborhoodSearchMethod(DIRECT7)
    n_a = a.setInputTargetFramesFiltered(frames, poses, LEAF)
    filtered = b.voxelGridFilter(assembled, LEAF)
    b.setInputTarget(filtered)
    assert n_a == filtered.shape[0]
    da, db = a.gridDump(), b.gridDump()
    assert np.array_equal(da["idx"], db["idx"]) and np.array_equal(da["n"], db["n"])
    assert np.array_equal(da["mean"], db["mean"]) and np.array_equal(da["icov"], db["icov"])
    a.prepareTarget()   # nothing is left to do for NDT: returns, and says so
    assert a.targetPrepared()


def test_prepared_means_prepared(O, drive):
    from lidarslam_ros2_amd import _capi

    frames, poses = _window(drive)
    src, guess = _source(O, drive), np.asarray(drive["guess0"], np.float32)
    fresh = _gicp()
    assert not fresh.targetPrepared()
    with pytest.raises(_capi.RegistrationError) as ei:
        fresh.prepareTarget()
    assert ei.value.status == -4   # LSR_ERR_NO_TARGET

    builder, reg, lazy = _gicp(), _gicp(), _gicp()
    builder.setInputTargetFramesFiltered(frames, poses, LEAF)
    assert not builder.targetPrepared()           # the covariances are the first align's business ...
    builder.prepareTarget()                       # ... unless they are asked for, and no source was ever set on this object
    assert builder.targetPrepared()
    reg.shareTargetOf(builder)
    assert reg.targetPrepared()                   # same k_correspondences / gicp_epsilon: nothing left for reg's align to build
    reg.setInputSource(src)
    reg.align(guess)
    lazy.setInputTargetFramesFiltered(frames, poses, LEAF)
    lazy.setInputSource(src)
    lazy.align(guess)                             # builds the covariances inside align, as the reference does
    assert lazy.targetPrepared()
    assert np.array_equal(reg.getFinalTransformation(), lazy.getFinalTransformation())
    assert reg.last_result["iterations"] == lazy.last_result["iterations"]
    assert reg.last_result["n_correspondences"] == lazy.last_result["n_correspondences"]

    owner = _gicp()
    owner.setInputTargetFramesFiltered(frames, poses, LEAF)
    owner.prepareTarget()
    assert owner.targetPrepared()
    owner.setCorrespondenceRandomness(15)         # other neighbourhoods: the covariances in place are no longer this object's
    assert not owner.targetPrepared()
    owner.prepareTarget()
    assert owner.targetPrepared()


def test_gicp_frontend_stream_matches_the_oracle_on_every_scan(drive):
    from gicp_frontend_oracle import OracleGicpFrontendRegistration

    gpu, gpu_sizes = _replay(_gicp(), drive, device_payloads=True, mapper=_gicp(), builder=_gicp(), async_update=True, swap_lag=0)
    cpu, cpu_sizes = _replay(OracleGicpFrontendRegistration(solver=1), drive)
    assert gpu.update_at == cpu.update_at and len(gpu.update_at) == 8, (gpu.update_at, cpu.update_at)
    assert gpu.points_kept == cpu.points_kept
    assert gpu_sizes == cpu_sizes and len(gpu_sizes) == 9, (gpu_sizes, cpu_sizes)
    worst = (0.0, 0.0)
    for j, (a, b) in enumerate(zip(gpu.poses, cpu.poses)):
        dt, ang = pose_delta(a, b)
        worst = (max(worst[0], dt), max(worst[1], ang))
    print("GICP frontend stream: worst GPU-vs-oracle (Gauss-Newton) pose difference over %d scans: %.2e m %.2e rad; target sizes %s"
          % (len(gpu.poses), worst[0], worst[1], gpu_sizes))
    print("GICP frontend stream: outer iterations GPU %s oracle %s" % (gpu.iterations, cpu.iterations))
    for j, (a, b) in enumerate(zip(gpu.poses, cpu.poses)):
        dt, ang = pose_delta(a, b)
        assert dt <= 1e-3 and ang <= 1e-4, (j, dt, ang)
    for j, (a, t) in enumerate(zip(gpu.poses, drive["truths"])):
        dt, ang = pose_delta(a, t)
        assert dt <= 0.05 and ang <= 5e-3, (j, dt, ang)
    # reported, not asserted: the reference's BFGS schedule on the same drive (free running, its own maps)
    bfgs, _ = _replay(OracleGicpFrontendRegistration(solver=0), drive)
    worst_b = (0.0, 0.0)
    for a, b in zip(gpu.poses, bfgs.poses[:len(gpu.poses)]):
        dt, ang = pose_delta(a, b)
        worst_b = (max(worst_b[0], dt), max(worst_b[1], ang))
    print("GICP frontend stream: worst GPU-vs-oracle (BFGS, solver=0) pose difference: %.2e m %.2e rad; BFGS updates at %s"
          % (worst_b[0], worst_b[1], bfgs.update_at))


def test_gicp_map_update_on_a_worker_thread_gives_the_serial_replay_bit_for_bit(drive):
    plain, _ = _replay(_gicp(), drive, device_payloads=True, mapper=_gicp())
    for lag in (0, 1):
        serial, serial_sizes = _replay(_gicp(), drive, device_payloads=True, mapper=_gicp(), builder=_gicp(), swap_lag=lag)
        for rep in range(2):   # twice: the second drive recycles the targets of the first (lsr_share_target hands them back)
            thr, thr_sizes = _replay(_gicp(), drive, device_payloads=True, mapper=_gicp(), builder=_gicp(), async_update=True, swap_lag=lag)
            assert thr.update_at == serial.update_at and len(thr.update_at) >= 7
            assert thr.points_kept == serial.points_kept and thr.iterations == serial.iterations and thr_sizes == serial_sizes
            assert all(np.array_equal(a, b) for a, b in zip(thr.poses, serial.poses)), lag
            assert len(thr.update_seconds) == len(thr.update_at) == len(thr.swap_wait_seconds)
        if lag == 0:
            assert all(np.array_equal(a, b) for a, b in zip(serial.poses, plain.poses))
    # host payloads (keyframes through the host, frames staged back to back) and device payloads: the same stream
    host, host_sizes = _replay(_gicp(), drive, device_payloads=False)
    assert host.update_at == plain.update_at and host.points_kept == plain.points_kept
    assert all(np.array_equal(a, b) for a, b in zip(host.poses, plain.poses))


def test_the_target_is_ready_at_every_hand_over(drive):
    seen = []
    eager, _ = _replay(_gicp(), drive, device_payloads=True, mapper=_gicp(), builder=_gicp(), async_update=True, swap_lag=0, prepared=seen)
    assert len(seen) == 1 + len(eager.update_at) == 9 and all(seen), seen
    # the same replay without prepareTarget: the scan that takes a target over builds its covariances inside align — same numbers
    builder = _gicp()
    builder.prepareTarget = lambda: None
    seen_lazy = []
    lazy, _ = _replay(_gicp(), drive, device_payloads=True, mapper=_gicp(), builder=builder, async_update=True, swap_lag=0, prepared=seen_lazy)
    assert len(seen_lazy) == 9 and not any(seen_lazy), seen_lazy
    assert lazy.update_at == eager.update_at
    assert all(np.array_equal(a, b) for a, b in zip(lazy.poses, eager.poses))

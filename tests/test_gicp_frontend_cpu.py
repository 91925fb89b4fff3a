"""The frontend in GICP mode, the parts that need no GPU: which calls FrontendReplay makes on its registration objects (a recording
stand-in), that the C ABI carries the two new entries, and the CPU-oracle run of the drive that tests/test_gicp_frontend_gpu.py
compares the gfx950 core with (scanmatcher_component.cpp:115-120,308-316,329,353)."""
import os
import re
import subprocess

import numpy as np

from lidarslam_ros2_amd import synth
from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload
from lidarslam_ros2_amd.posemath import pose_delta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    """Stands in for a registration object: every call FrontendReplay makes is appended to a log shared by the objects of one
    replay; the "registered" pose advances 0.5 m along x per scan.  Keyframes carry a tag in their first float."""

    def __init__(self, name, log):
        self.name, self.log, self.scans = name, log, 0

    def _tags(self, frames):
        return tuple(int(np.asarray(f).reshape(-1, 8)[0, 0]) for f in frames)

    def setInputSourcePointCloud2(self, data, n_points, point_step, offsets, rmin, rmax, leaf):
        self.log.append((self.name, "setInputSourcePointCloud2", float(leaf)))
        return int(n_points)

    def voxelGridFilterPointCloud2(self, data, n_points, point_step, offsets, leaf, out_point_step=32, out_offsets=(0, 4, 8, 16)):
        self.log.append((self.name, "voxelGridFilterPointCloud2", float(leaf)))
        return np.asarray(data).reshape(-1, point_step)[:2].copy()

    def setInputTargetFrames(self, frames, poses):
        self.log.append((self.name, "setInputTargetFrames", self._tags(frames), tuple(float(P[0, 3]) for P in poses)))

    def setInputTargetFramesFiltered(self, frames, poses, leaf):
        self.log.append((self.name, "setInputTargetFramesFiltered", self._tags(frames), tuple(float(P[0, 3]) for P in poses), float(leaf)))
        return 0

    def prepareTarget(self):
        self.log.append((self.name, "prepareTarget"))

    def shareTargetOf(self, other):
        self.log.append((self.name, "shareTargetOf", other.name))

    def align(self, guess):
        self.log.append((self.name, "align"))
        self.scans += 1

    def getFinalTransformation(self):
        T = np.eye(4)
        T[0, 3] = 0.5 * self.scans
        return T

    def getFinalNumIteration(self):
        return 1


def _record(method, with_builder, async_update=False, trans=1.25, n_scans=7):
    log = []
    reg = Recorder("reg", log)
    builder = Recorder("builder", log) if with_builder else None
    p = FrontendParams(trans_for_mapupdate=trans, num_targeted_cloud=3) if method is None else \
        FrontendParams(trans_for_mapupdate=trans, num_targeted_cloud=3, registration_method=method)
    fr = FrontendReplay(reg, p, builder=builder, async_update=async_update)
    frames = [np.full((4, 3), 10 + k, np.float32) for k in range(3)]                    # tags 10, 11, 12
    poses = [np.eye(4) for _ in range(3)]
    for k in range(3):
        poses[k][0, 3] = float(k - 2)
    fr.initialise(frames, poses, np.eye(4))
    out = FrontendResult()
    for j in range(n_scans):
        scan = np.zeros((8, 3), np.float32)
        scan[:, 0] = 20 + j                                                             # the keyframe made of scan j carries tag 20 + j
        fr.receive_cloud(as_pc2_payload(scan), 8, out)
    fr.finish(out)
    return log, out


# What the FrontendReplay of the commit before the GICP mode recorded with this stand-in (reg + builder, serial, 1.25 m, 7 scans):
# the NDT sequence that registration_method = "NDT" must keep call for call.
NDT_SEQUENCE_BEFORE_GICP_MODE = [
    ("builder", "setInputTargetFrames", (12, 11, 10), (0.0, -1.0, -2.0)),
    ("reg", "shareTargetOf", "builder"),
    ("reg", "setInputSourcePointCloud2", 0.2), ("reg", "align"),
    ("reg", "setInputSourcePointCloud2", 0.2), ("reg", "align"),
    ("reg", "setInputSourcePointCloud2", 0.2), ("reg", "align"),
    ("builder", "voxelGridFilterPointCloud2", 0.1),
    ("builder", "setInputTargetFrames", (22, 12, 11), (1.5, 0.0, -1.0)),
    ("reg", "shareTargetOf", "builder"),
    ("reg", "setInputSourcePointCloud2", 0.2), ("reg", "align"),
    ("reg", "setInputSourcePointCloud2", 0.2), ("reg", "align"),
    ("reg", "setInputSourcePointCloud2", 0.2), ("reg", "align"),
    ("builder", "voxelGridFilterPointCloud2", 0.1),
    ("builder", "setInputTargetFrames", (25, 22, 12), (3.0, 1.5, 0.0)),
    ("reg", "shareTargetOf", "builder"),
    ("reg", "setInputSourcePointCloud2", 0.2), ("reg", "align"),
]


def test_gicp_mode_filters_the_window_and_prepares_the_target_before_the_hand_over():
    for async_update in (False, True):
        log, out = _record("GICP", True, async_update)
        assert out.update_at == [2, 5]
        builds = [e for e in log if e[1] == "setInputTargetFramesFiltered"]
        assert [e[0] for e in builds] == ["builder"] * 3
        # the window newest first (scanmatcher_component.cpp:448-464), each frame with its own pose, leaf = vg_size_for_input (:310)
        assert [e[2] for e in builds] == [(12, 11, 10), (22, 12, 11), (25, 22, 12)]
        assert [e[3] for e in builds] == [(0.0, -1.0, -2.0), (1.5, 0.0, -1.0), (3.0, 1.5, 0.0)]
        assert all(e[4] == FrontendParams().vg_size_for_input for e in builds)
        assert not any(e[1] == "setInputTargetFrames" for e in log)
        # prepareTarget: on the object that built the target, right behind the build, before the hand-over
        for i, e in enumerate(log):
            if e[1] == "setInputTargetFramesFiltered":
                assert log[i + 1] == (e[0], "prepareTarget")
        order = [e[1] for e in log if e[1] in ("setInputTargetFramesFiltered", "prepareTarget", "shareTargetOf")]
        assert order == ["setInputTargetFramesFiltered", "prepareTarget", "shareTargetOf"] * 3
    # without a builder the callback's own object builds and prepares, and nothing is handed over
    log, out = _record("GICP", False)
    assert [e[0] for e in log if e[1] in ("setInputTargetFramesFiltered", "prepareTarget")] == ["reg"] * 6
    assert not any(e[1] == "shareTargetOf" for e in log)


def test_ndt_mode_makes_the_calls_it_made_before_the_gicp_mode():
    for method in (None, "NDT"):
        log, out = _record(method, True)
        assert log == NDT_SEQUENCE_BEFORE_GICP_MODE
        assert out.update_at == [2, 5]
    log, _ = _record("NDT", True, async_update=True)
    assert sorted(map(repr, log)) == sorted(map(repr, NDT_SEQUENCE_BEFORE_GICP_MODE))   # the worker's calls interleave with the scans'
    assert not any(e[1] in ("prepareTarget", "setInputTargetFramesFiltered") for e in log)
    import pytest
    with pytest.raises(ValueError):
        FrontendReplay(Recorder("reg", []), FrontendParams(registration_method="ICP"))


def test_c_abi_declares_and_exports_the_filtered_frames_target_and_prepare_target():
    from lidarslam_ros2_amd import _capi

    new = ("lsr_set_input_target_frames_filtered", "lsr_prepare_target")
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    declared = sorted(set(re.findall(r"\b(lsr_[a-z0-9_]+)\s*\(", hdr)))
    for name in new:
        assert name in declared and name in _capi.EXPORTED_SYMBOLS
    assert "LSR_TARGET_PREPARED = 48" in hdr and _capi.TARGET_PREPARED == 48
    lib = _capi.load()
    assert lib.lsr_set_input_target_frames_filtered.argtypes is not None and len(lib.lsr_set_input_target_frames_filtered.argtypes) == 9
    assert lib.lsr_prepare_target.argtypes is not None and len(lib.lsr_prepare_target.argtypes) == 1
    # what the shared library exports is what the header declares, name for name: every defined function with a plain C name counts
    # (a file-local helper that slips into an extern "C" block would show up here), only _init / _fini and C++-mangled names do not
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r"\sT\s+([A-Za-z][A-Za-z0-9_]*)$", nm, re.M)))
    assert exported == declared, (set(exported) ^ set(declared))
    # without a device the new entries fail like every other one: no handle, an error status, no crash
    assert lib.lsr_prepare_target(None) != 0
    assert lib.lsr_set_input_target_frames_filtered(None, 0, None, None, 32, None, 0, 0.2, None) != 0


def test_oracle_gicp_frontend_over_the_first_nine_scans():
    """The fixture the GPU stream test leans on: the oracle adapter alone (Gauss-Newton) over the first 9 scans of the drive with
    trans_for_mapupdate = 1.25 m — every keyframe decision then has at least 0.24 m of margin (with 1.5 m they sit within
    millimetres of the threshold)."""
    import multiprocessing as mp

    from gicp_frontend_oracle import OracleGicpFrontendRegistration

    with mp.get_context("spawn").Pool(min(32, len(os.sched_getaffinity(0)))) as p:
        drive = synth.cfg_frontend_drive(9, pool=p)
    reg = OracleGicpFrontendRegistration(solver=1)
    fr = FrontendReplay(reg, FrontendParams(registration_method="GICP", trans_for_mapupdate=1.25))
    fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
    out = FrontendResult()
    for scan in drive["scans"]:
        fr.receive_cloud(as_pc2_payload(scan), int(scan.shape[0]), out)
    fr.finish(out)
    assert out.update_at == [2, 5, 8]
    assert reg.target_sizes == [164868, 163095, 161334, 159283]
    worst = (0.0, 0.0)
    for j, (a, t) in enumerate(zip(out.poses, drive["truths"])):
        dt, ang = pose_delta(a, t)
        worst = (max(worst[0], dt), max(worst[1], ang))
        assert dt <= 0.05 and ang <= 5e-3, (j, dt, ang)
    print("oracle GICP frontend, 9 scans: worst distance to the ground truth %.4f m %.2e rad; iterations %s" % (worst[0], worst[1], out.iterations))

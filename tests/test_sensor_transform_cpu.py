"""The device-free half of the cloud callback's head (scanmatcher_component.cpp:188-199) and of the use_odom guess (:333-348):
lsr_sensor_transform_matrix against the numpy restatement of the library's pose matrix (tests/map_numpy.py), lsr_odom_guess against
the float64 numpy product, and the C++ surface / the INTEGRATION.md snippet against the mock PCL headers.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from map_numpy import pose_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _quat_xyzw(roll, pitch, yaw):
    """x y z w of Rz(yaw) Ry(pitch) Rx(roll), in double"""
    cr, sr, cp, sp, cy, sy = math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(yaw / 2), math.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], np.float64)


def _matrix(translation, rotation_xyzw):
    from lidarslam_ros2_amd import sensorTransformMatrix

    return sensorTransformMatrix(translation, rotation_xyzw)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_matrix_of_the_car_mount():
    """mapping_car.launch.py:28 — the LiDAR at 1.2 0 2.0 from base_link, identity rotation"""
    t, q = (1.2, 0.0, 2.0), (0.0, 0.0, 0.0, 1.0)
    got = _matrix(t, q)
    want = pose_matrix(t, q)[:3].astype(F)
    assert got.shape == (3, 4) and got.dtype == F
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(got, np.array([[1, 0, 0, F(1.2)], [0, 1, 0, 0], [0, 0, 1, 2]], F))


def test_matrix_of_a_general_mount():
    t = (0.83, -2.4, 3.1)
    q = _quat_xyzw(0.21, -0.37, 1.9)
    got = _matrix(t, q)
    want = pose_matrix(t, q)[:3].astype(F)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.abs(got[:, :3]).min() > 1e-3   # every rotation entry is in play


def test_matrix_does_not_normalise_the_quaternion():
    t = (0.5, 0.25, -1.0)
    q = _quat_xyzw(-0.4, 0.15, 0.7) * 1.001
    assert abs(np.linalg.norm(q) - 1.001) < 1e-12
    got = _matrix(t, q)
    want = pose_matrix(t, q)[:3].astype(F)
    assert np.array_equal(_bits(got), _bits(want))
    unit = pose_matrix(t, q / np.linalg.norm(q))[:3].astype(F)
    assert not np.array_equal(_bits(got), _bits(unit))   # a normalising implementation would return this one


def test_matrix_refuses_null_pointers():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    out = np.zeros(12, F)
    tf = _capi.SensorTransform((C.c_double * 3)(0, 0, 0), (C.c_double * 4)(0, 0, 0, 1))
    assert lib.lsr_sensor_transform_matrix(None, out.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lib.lsr_sensor_transform_matrix(C.byref(tf), None) == -1


# ---- lsr_odom_guess ------------------------------------------------------------------------------------------------------------------
def _rigid(rng, t_max):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    M = pose_matrix(rng.uniform(-t_max, t_max, 3), q)
    return M.astype(F)


def test_odom_guess_with_the_identity_returns_sim_trans_bit_for_bit():
    from lidarslam_ros2_amd import odomGuess

    rng = np.random.default_rng(11)
    sim, odom = _rigid(rng, 1000.0), _rigid(rng, 1000.0)
    got = odomGuess(sim, np.eye(4, dtype=F), odom)
    assert got.dtype == F and np.array_equal(_bits(got), _bits(sim))


def test_odom_guess_is_the_float64_product_rounded_once():
    """Twenty seeded rigid triples with translations up to 1000 m: every entry within one fp32 unit in the last place of the float64
    numpy product of the fp32 inputs.  The margin: the entry computes in double — an error of a few 1e-16 relative to operands of at
    most a few 1e3, i.e. below 1e-11 absolute, against half an fp32 ulp of >= 3e-8 for a rotation entry near 1 and >= 4e-6 for a
    translation near 100 — and rounds once to fp32: the rounded value is the correctly rounded reference or, when the reference sits
    within that double error of a rounding boundary, its neighbour."""
    from lidarslam_ros2_amd import odomGuess

    rng = np.random.default_rng(20261020)
    for k in range(20):
        sim, prev, odom = _rigid(rng, 1000.0), _rigid(rng, 1000.0), _rigid(rng, 1000.0)
        want64 = sim.astype(np.float64) @ np.linalg.inv(prev.astype(np.float64)) @ odom.astype(np.float64)
        want = want64.astype(F)
        got = odomGuess(sim, prev, odom)
        assert got.dtype == F
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert np.all(err <= np.spacing(np.abs(want)).astype(np.float64)), (k, got, want)
        assert np.array_equal(got[3], np.array([0, 0, 0, 1], F))


def test_odom_guess_identity_test_is_exact():
    """previous_odom equal to the identity in eleven of its twelve free entries, m03 = 1e-7: not the identity (`!=`, :344)"""
    from lidarslam_ros2_amd import odomGuess

    rng = np.random.default_rng(5)
    sim, odom = _rigid(rng, 50.0), _rigid(rng, 50.0)
    prev = np.eye(4, dtype=F)
    prev[0, 3] = F(1e-7)
    got = odomGuess(sim, prev, odom)
    want = (sim.astype(np.float64) @ np.linalg.inv(prev.astype(np.float64)) @ odom.astype(np.float64)).astype(F)
    assert not np.array_equal(_bits(got), _bits(sim))
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def test_odom_guess_refuses_null_pointers():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    m = np.eye(4, dtype=F).reshape(16)
    p = m.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.lsr_odom_guess(*args) == -1


# ---- the layers above ----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    from lidarslam_ros2_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    lib = _capi.load()
    for name, n_args in (("lsr_sensor_transform_matrix", 2), ("lsr_transform_pc2", 7), ("lsr_set_input_source_pc2_tf", 10), ("lsr_odom_guess", 4)):
        assert name + "(" in hdr and name in _capi.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == n_args
    assert "typedef struct lsr_sensor_transform {" in hdr
    assert C.sizeof(_capi.SensorTransform) == 56
    # without a device the two entries that need a handle fail like every other one: an error status, no crash
    assert lib.lsr_transform_pc2(None, None, 0, None, None, 0, None) != 0
    assert lib.lsr_set_input_source_pc2_tf(None, None, 0, None, None, 0.0, 1.0, 0.2, 0, None) != 0


class _RecordingReg:
    """A registration object that records the calls of FrontendReplay and aligns to the guess it is given."""

    def __init__(self):
        self.calls, self.guesses = [], []

    def setInputTargetFrames(self, frames, poses):
        self.calls.append("target")

    def imuReset(self, scan_period):
        self.calls.append("imuReset")

    def transformPointCloud2(self, data, n_points, point_step, offsets, translation, rotation_xyzw, out=None):
        self.calls.append(("transform", tuple(translation), tuple(rotation_xyzw)))
        return np.array(data, copy=True)

    def deskewPointCloud2(self, data, n_points, point_step, offsets, scan_time, out=None):
        self.calls.append(("deskew", out is data))
        return data, {}

    def setInputSourcePointCloud2(self, data, n_points, point_step, offsets, rmin, rmax, leaf, **kw):
        self.calls.append(("source", kw))
        return n_points

    def voxelGridFilterPointCloud2(self, data, n_points, point_step, offsets, leaf):
        self.calls.append(("filter", int(n_points)))
        return np.ascontiguousarray(data)

    def align(self, guess):
        self.guesses.append(np.array(guess, copy=True))
        self._T = np.array(guess, np.float32)
        self._T[0, 3] += 2.0    # every scan moves 2 m: every scan triggers a map update

    def getFinalTransformation(self):
        return self._T

    def getFinalNumIteration(self):
        return 1


def _replay(params, n_scans=2, **kw):
    from lidarslam_ros2_amd.frontend import FrontendReplay, FrontendResult, as_pc2_payload

    reg = _RecordingReg()
    fr = FrontendReplay(reg, params)
    fr.initialise([np.ones((4, 3), F)], [np.eye(4)], np.eye(4))
    out = FrontendResult()
    scan = as_pc2_payload(np.array([[5, 0, 0], [0, 6, 1], [-7, 1, 2]], F))
    for j in range(n_scans):
        fr.receive_cloud(scan, 3, out, **{k: v[j] for k, v in kw.items()})
    fr.finish(out)
    return reg, out


def test_replay_makes_none_of_the_new_calls_with_the_identity_mount():
    from lidarslam_ros2_amd.frontend import FrontendParams

    reg, out = _replay(FrontendParams())
    assert [c for c in reg.calls if c[0] == "transform"] == []
    assert all(c[1] == {} for c in reg.calls if c[0] == "source")
    assert len(out.update_at) == 2


def test_replay_order_of_calls_with_a_mount():
    from lidarslam_ros2_amd.frontend import FrontendParams

    t, q = (1.2, 0.0, 2.0), (0.0, 0.0, 0.0, 1.0)
    # without IMU: the scan side takes the fused entry on the raw payload, the host map path moves its copy before its range mask
    reg, _ = _replay(FrontendParams(sensor_translation=t, sensor_rotation_xyzw=q), n_scans=1)
    calls = [c for c in reg.calls if c != "target"]
    assert calls == [("source", {"sensor_transform": (t, q)}), ("transform", t, q), ("filter", 3)]
    # with IMU: transform -> de-skew (in place, on the transformed copy) -> the rest, which sees robot-frame records
    reg, _ = _replay(FrontendParams(sensor_translation=t, sensor_rotation_xyzw=q, use_imu=True), n_scans=1, scan_time=[100.0])
    calls = [c for c in reg.calls if c not in ("target", "imuReset")]
    assert calls == [("transform", t, q), ("deskew", True), ("source", {}), ("filter", 3)]


def test_replay_use_odom_guess_and_missing_odometry():
    import pytest

    from lidarslam_ros2_amd import odomGuess
    from lidarslam_ros2_amd.frontend import FrontendParams

    rng = np.random.default_rng(3)
    odoms = [_rigid(rng, 30.0).astype(np.float64) for _ in range(3)]
    reg, out = _replay(FrontendParams(use_odom=True), n_scans=3, odom=odoms)
    prev, pose = np.eye(4, dtype=F), np.eye(4, dtype=F)
    for j in range(3):
        want = odomGuess(pose, prev, odoms[j].astype(F))
        assert np.array_equal(_bits(reg.guesses[j]), _bits(want)), j
        prev = odoms[j].astype(F)
        pose = np.asarray(out.poses[j], np.float64).astype(F)
    assert np.array_equal(_bits(reg.guesses[0]), _bits(np.eye(4, dtype=F)))   # the first scan: previous_odom is the identity
    with pytest.raises(ValueError):
        _replay(FrontendParams(use_odom=True), n_scans=1)


def test_header_syntax_and_the_integration_snippet():
    """the new members of the C++ surface compile (-fsyntax-only) against the mock PCL / pclomp headers, and the block INTEGRATION.md
    shows is the block that was just compiled"""
    src = os.path.join(ROOT, "tests", "cpp", "sensor_transform_syntax.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"), src])
    block = open(src).read().split("// [sensor-transform-snippet begin]\n")[1].split("// [sensor-transform-snippet end]")[0].rstrip("\n")
    assert block in open(os.path.join(ROOT, "INTEGRATION.md")).read()

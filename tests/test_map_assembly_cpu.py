"""CPU: the host side of the map assembly — the C ABI's symbol, key and argument check, Eigen's matrix -> quaternion
conversion, and the MapArray / FrontendReplay bookkeeping against a fake registration object whose assembleMap is the numpy
restatement (tests/map_numpy.py).  The kernel itself: tests/test_map_assembly_gpu.py."""
import os
import re

import numpy as np

import map_numpy
from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload
from lidarslam_ros2_amd.map_array import MapArray
from lidarslam_ros2_amd.posemath import matrix_from_pose, quaternion_from_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_key_exist():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    assert hasattr(lib, "lsr_assemble_map") and "lsr_assemble_map" in _capi.EXPORTED_SYMBOLS
    assert _capi.MAP_ASSEMBLY_FORM == 49
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    assert re.search(r"LSR_MAP_ASSEMBLY_FORM\s*=\s*49\b", hdr)
    assert ":529-552" in hdr and ":321-368" in hdr


def test_null_handle_is_refused():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    assert lib.lsr_assemble_map(None, None, 0, None, 0, None, None, 0, None, 0, None, None) == -1
    assert b"null handle" in lib.lsr_last_error()


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def test_quaternion_from_matrix_takes_eigens_four_branches():
    """Closed forms: the identity goes through the trace branch; half turns about x, y, z have trace -1 and the largest diagonal
    element at 0, 1, 2 — the three other branches, each exact."""
    assert np.array_equal(quaternion_from_matrix(np.eye(3)), [0, 0, 0, 1])
    assert np.array_equal(quaternion_from_matrix(np.diag([1.0, -1.0, -1.0])), [1, 0, 0, 0])
    assert np.array_equal(quaternion_from_matrix(np.diag([-1.0, 1.0, -1.0])), [0, 1, 0, 0])
    assert np.array_equal(quaternion_from_matrix(np.diag([-1.0, -1.0, 1.0])), [0, 0, 1, 0])
    assert np.array_equal(quaternion_from_matrix(np.eye(4)), [0, 0, 0, 1])      # a 4x4 pose: its rotation block


def test_quaternion_round_trip_on_random_rotations():
    """The round trip a stored pose makes: unit quaternion -> tf2::fromMsg's matrix -> Eigen's Quaterniond(Matrix3d) gives the quaternion
    back (up to the sign both stand for) to 1e-15 — a handful of roundings of 1.1e-16 on numbers <= 1 — in all four branches."""
    rng = np.random.default_rng(11)
    seen = set()
    for t in range(400):
        q0 = rng.normal(size=4)
        if t % 4 == 0:
            q0[3] = rng.uniform(-1e-3, 1e-3)    # next to a half turn: trace < 0, the largest-diagonal branches
        q0 /= np.linalg.norm(q0)
        R = matrix_from_pose((0, 0, 0), q0)[:3, :3]
        q1 = quaternion_from_matrix(R)
        seen.add("trace" if np.trace(R) > 0 else int(np.argmax(np.diag(R))))
        err = min(np.abs(q1 - q0).max(), np.abs(q1 + q0).max())
        assert err <= 1e-15, (t, err)
    assert seen == {"trace", 0, 1, 2}
    # ... and the library's own pose matrix is that expression: map_numpy restates it independently
    assert np.array_equal(map_numpy.pose_matrix((1, 2, 3), q1), matrix_from_pose((1, 2, 3), q1))


class FakeFrontendRegistration(map_numpy.FakeRegistration):
    """The calls the replay makes, recorded; align() walks a script of poses; the map-side filter is the identity."""

    def __init__(self, poses):
        super().__init__()
        self.script, self.k, self.final = [np.asarray(P, np.float64) for P in poses], 0, np.eye(4)

    def setInputSourcePointCloud2(self, data, n_points, point_step, offsets, rmin, rmax, leaf):
        self.calls.append(("source", int(n_points)))
        return int(n_points)

    def align(self, guess):
        self.calls.append(("align",))
        self.final = self.script[self.k]
        self.k += 1

    def getFinalTransformation(self):
        return self.final

    def getFinalNumIteration(self):
        return 3

    def voxelGridFilterPointCloud2(self, data, n_points, point_step, offsets, leaf, out_point_step=32, out_offsets=(0, 4, 8, 16)):
        self.calls.append(("map_filter", int(n_points)))
        return np.asarray(data).reshape(int(n_points), point_step).copy()

    def setInputTargetFrames(self, frames, poses):
        self.calls.append(("target", len(frames)))


def _pose(x, yaw=0.0):
    T = np.eye(4)
    T[:3, :3] = _rot((0, 0, 1), yaw)
    T[0, 3] = x
    return np.asarray(np.asarray(T, np.float32), np.float64)     # what a registration hands back: float entries


def _drive(map_array=None, every=0, n_scans=9):
    frames = [np.full((4 + k, 3), float(k), np.float32) for k in range(3)]
    frame_poses = [_pose(1.5 * k, 0.01 * k) for k in range(3)]
    truth = [_pose(3.0 + 0.6 * (j + 1), 0.3 * (j + 1)) for j in range(n_scans)]
    reg = FakeFrontendRegistration(truth)
    kw = {} if map_array is None and every == 0 else dict(map_array=map_array, map_publish_every=every)
    fr = FrontendReplay(reg, FrontendParams(num_targeted_cloud=2), **kw)
    fr.initialise(frames, frame_poses, _pose(3.0))
    out = FrontendResult()
    rng = np.random.default_rng(3)
    for j in range(n_scans):
        fr.receive_cloud(as_pc2_payload(rng.uniform(1, 30, (6 + j, 3)).astype(np.float32), rng.uniform(0, 9, 6 + j).astype(np.float32)), 6 + j, out)
    fr.finish(out)
    return fr, reg, out, frame_poses, truth


def test_map_array_and_replay_bookkeeping():
    ma = MapArray()
    fr, reg, out, frame_poses, truth = _drive(ma, every=2)
    # scans 0.6 m apart, an update every third one (>= 1.5 m): scans 2, 5, 8
    assert out.update_at == [2, 5, 8]
    assert len(ma) == 3 + 3 and len(fr.submaps) == 2              # the MapArray keeps the whole map, the window its last two
    # distances: path length over the initial keyframes, then latest_distance_ += trans_ at the triggering scan
    key = [frame_poses[-1][:3, 3]] + [truth[j][:3, 3] for j in out.update_at]
    want = [0.0, 1.5, 3.0]
    for a, b in zip(key[:-1], key[1:]):
        want.append(want[-1] + float(np.linalg.norm(b - a)))
    assert np.allclose([s.distance for s in ma.submaps], want, rtol=0, atol=1e-12)
    # stored poses: the position as given, the quaternion by Eigen's conversion of the rotation block
    for s, P in zip(ma.submaps, frame_poses + [truth[j] for j in out.update_at]):
        assert s.position == tuple(P[:3, 3]) and np.array_equal(s.orientation, quaternion_from_matrix(P[:3, :3]))
        assert s.cloud.dtype == np.float32 and s.cloud.shape[1] == 8
    # record counts: the keyframes as they went in (identity map filter, nothing out of range)
    assert [s.cloud.shape[0] for s in ma.submaps] == [4, 5, 6, 8, 11, 14]
    # publishMap ran at the end of the second update only (every = 2; the fourth would be next): the map as it stood then
    assert len(out.publish_seconds) == 1 and len(out.update_seconds) == 3
    rec, first = fr.published
    assert rec.shape == (4 + 5 + 6 + 8 + 11, 32) and first.tolist() == [0, 4, 9, 15, 23, 34]
    # extend_published moves only what is new, and the resident map equals publish_map from scratch and the restatement
    n_before = len(reg.calls)
    rec2, first2 = ma.extend_published(reg)
    assert reg.calls[n_before:] == [("assembleMap", 1)]
    full, first_full = ma.publish_map(reg)
    want_rec, want_first = map_numpy.assemble_map(ma.submaps)
    assert np.array_equal(rec2, full) and np.array_equal(full, want_rec) and rec2.shape == (48, 32)
    assert np.array_equal(first2, first_full) and np.array_equal(first_full, want_first)
    assert np.array_equal(rec2[:34], rec)                          # the part published earlier is untouched
    rec3, _ = ma.extend_published(reg)                             # nothing new: no call, the same map
    assert reg.calls[n_before:] == [("assembleMap", 1), ("assembleMap", 6)] and np.array_equal(rec3, rec2)
    # the map is moved by the pose the message round trip yields
    M = matrix_from_pose(ma.submaps[4].position, ma.submaps[4].orientation)
    assert np.array_equal(full[first_full[4]:first_full[5]], map_numpy.move_records(ma.submaps[4].cloud, 11, M))
    # modified_map: the optimiser's poses instead
    poses = [np.linalg.inv(_pose(0.1 * k, 0.2)) for k in range(6)]
    mod, first_mod = ma.modified_map(reg, poses)
    assert np.array_equal(first_mod, want_first)
    assert np.array_equal(mod[first_mod[2]:first_mod[3]], map_numpy.move_records(ma.submaps[2].cloud, 6, poses[2]))


def test_default_replay_has_no_map_array_and_makes_the_same_calls():
    fr0, reg0, out0, _, _ = _drive()
    assert fr0.map_array is None and fr0.map_publish_every == 0 and fr0.published is None and out0.publish_seconds == []
    fr1, reg1, out1, _, _ = _drive(MapArray(), every=1)
    assert not any(c[0] == "assembleMap" for c in reg0.calls)
    assert [c for c in reg1.calls if c[0] != "assembleMap"] == reg0.calls      # the map array adds calls, it changes none
    assert [c for c in reg1.calls if c[0] == "assembleMap"] == [("assembleMap", 4), ("assembleMap", 1), ("assembleMap", 1)]
    assert out0.update_at == out1.update_at and all(np.array_equal(a, b) for a, b in zip(out0.poses, out1.poses))
    want = [("target", 2)]
    for j in range(9):
        want += [("source", 6 + j), ("align",)]
        if j in (2, 5, 8):
            want += [("map_filter", 6 + j), ("target", 2)]
    assert reg0.calls == want


def test_integration_md_map_snippets_compile_and_link(tmp_path):
    """the two call sites replaced (publishMap, the map half of doPoseAdjustment) are the blocks of
    tests/cpp/map_snippets.cpp, compiled against include/lidarslam_reg/map_assembly.hpp and linked against the library; the program
    itself shows the adapter refusing a call without a handle (no device needed)."""
    import subprocess
    import textwrap

    src = os.path.join(ROOT, "tests", "cpp", "map_snippets.cpp")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "map_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "MAP_SNIPPETS refused=1 payload=0" in run.stdout, (run.stdout, run.stderr)
    assert "null handle" in run.stderr
    text, doc = open(src).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("helpers", "publish_map", "pose_adjustment"):
        block = text.split(f"// [map-snippet begin: {name}]\n")[1].split(f"// [map-snippet end: {name}]")[0]
        assert textwrap.dedent(block).strip("\n").rstrip() in doc, name
    assert ":529-552" in doc and ":321-368" in doc

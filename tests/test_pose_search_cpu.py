"""CPU: the host side of the NDT pose search (lsr_pose_lattice_poses, lsr_select_poses; csrc/pose_search.hip) through ctypes against the
restatement tests/pose_search_numpy.py, the errors, the exported symbols — and the guard of the GPU search test's inputs: the procedure
run on the CPU oracle finds the truth on every one of them.  The kernel: tests/test_pose_search_gpu.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pose_search_numpy as psn
from lidarslam_ros2_amd import _capi, poseLattice, selectPoses, synth
from lidarslam_ros2_amd._capi import RegistrationError
from lidarslam_ros2_amd.posemath import pose_delta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID_ARGUMENT = -1


def _random_center(rng, tilted):
    roll, pitch = (rng.uniform(-0.6, 0.6, 2) if tilted else (0.0, 0.0))
    x, y, z = rng.uniform(-300, 300, 3)
    return synth.pose_matrix(x, y, z, rng.uniform(-math.pi, math.pi), roll, pitch).astype(np.float32)


# ---- the lattice ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, n_yaw", [((3, 3, 1), 5), ((4, 2, 3), 6), ((1, 1, 1), 1), ((1, 5, 1), 2), ((2, 1, 2), 1), ((9, 9, 1), 13)])
def test_lattice_bits_equal_the_restatement(n, n_yaw):
    rng = np.random.default_rng(sum(n) * 31 + n_yaw)
    for trial in range(4):
        center = _random_center(rng, tilted=trial >= 2)
        step = rng.uniform(0.05, 2.0, 3)
        yaw_step = rng.uniform(0.01, 0.5)
        got = poseLattice(center, n, step, n_yaw, yaw_step)
        want = psn.lattice(center, n, step, n_yaw, yaw_step)
        assert got.shape == want.shape == (n[0] * n[1] * n[2] * n_yaw, 4, 4) and got.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (got.shape[0], 1)))
    if n == (1, 1, 1):     # the lattice of one pose is the centre itself
        assert np.array_equal(got[0], center)


def test_lattice_index_order_and_centring():
    center = synth.pose_matrix(10.0, -4.0, 1.0, 0.3).astype(np.float32)
    P = poseLattice(center, (3, 2, 1), (1.0, 2.0, 1.0), 3, 0.1)
    assert P.shape[0] == 18
    assert np.allclose(P[0, :3, 3], [9.0, -5.0, 1.0]) and np.allclose(P[1, :3, 3], [10.0, -5.0, 1.0]) and np.allclose(P[3, :3, 3], [9.0, -3.0, 1.0])
    assert abs(psn.yaw_of(P[0]) - 0.2) < 1e-6 and abs(psn.yaw_of(P[6]) - 0.3) < 1e-6 and abs(psn.yaw_of(P[12]) - 0.4) < 1e-6


def _lattice_raw(center16, L, out, capacity, count):
    return _capi.load().lsr_pose_lattice_poses(center16, L, out, capacity, count)


def test_lattice_errors_and_count_only():
    fp = C.POINTER(C.c_float)
    c = np.eye(4, dtype=np.float32).reshape(-1)
    cp = c.ctypes.data_as(fp)
    count = C.c_size_t(77)

    def lat(n=(2, 2, 1), step=(1.0, 1.0, 1.0), n_yaw=3, yaw_step=0.1):
        return _capi.PoseLattice((C.c_int32 * 3)(*n), (C.c_double * 3)(*step), n_yaw, yaw_step)

    assert _lattice_raw(cp, C.byref(lat()), None, 0, C.byref(count)) == 0 and count.value == 12      # count only
    out = np.full((12, 16), 7, np.float32)
    count.value = 0
    assert _lattice_raw(cp, C.byref(lat()), out.ctypes.data_as(fp), 11, C.byref(count)) == ERR_INVALID_ARGUMENT   # capacity below the count
    assert count.value == 12 and np.all(out == 7)
    assert _lattice_raw(cp, C.byref(lat()), out.ctypes.data_as(fp), 12, C.byref(count)) == 0 and not np.any(out == 7)
    for bad in (lat(n=(0, 2, 1)), lat(n=(2, 2, -1)), lat(n_yaw=0), lat(n=(1024, 1024, 1), n_yaw=2), lat(step=(1.0, math.nan, 1.0)),
                lat(step=(math.inf, 1.0, 1.0)), lat(yaw_step=math.nan)):
        count.value = 77
        assert _lattice_raw(cp, C.byref(bad), None, 0, C.byref(count)) == ERR_INVALID_ARGUMENT and count.value == 77
    assert _lattice_raw(cp, C.byref(lat(n=(1024, 1024, 1), n_yaw=1)), None, 0, C.byref(count)) == 0 and count.value == 1 << 20   # the limit itself
    bad_c = c.copy()
    bad_c[13] = np.inf
    assert _lattice_raw(bad_c.ctypes.data_as(fp), C.byref(lat()), None, 0, C.byref(count)) == ERR_INVALID_ARGUMENT
    assert _lattice_raw(None, C.byref(lat()), None, 0, C.byref(count)) == ERR_INVALID_ARGUMENT
    assert _lattice_raw(cp, None, None, 0, C.byref(count)) == ERR_INVALID_ARGUMENT
    assert _lattice_raw(cp, C.byref(lat()), None, 0, None) == ERR_INVALID_ARGUMENT
    with pytest.raises(RegistrationError):
        poseLattice(np.eye(4), (0, 1, 1), (1, 1, 1), 1, 0.0)


# ---- the selection -------------------------------------------------------------------------------------------------------------------
def _synthetic(rng, kind):
    center = synth.pose_matrix(5.0, 5.0, 0.0, 0.0).astype(np.float32)
    poses = poseLattice(center, (7, 7, 1), (0.5, 0.5, 1.0), 5, math.radians(4.0))
    n = poses.shape[0]
    score = rng.uniform(0.1, 10.0, n)
    if kind == "ties":
        score = np.round(score)                           # ten distinct values over 245 candidates: exact ties everywhere
    elif kind == "specials":
        score[rng.choice(n, 40, replace=False)] = np.nan
        score[rng.choice(n, 40, replace=False)] = 0.0
        score[rng.choice(n, 40, replace=False)] = -3.0
        score[rng.choice(n, 5, replace=False)] = np.inf
    elif kind == "nothing":
        score[:] = np.where(np.arange(n) % 2 == 0, 0.0, np.nan)
    return score, poses


@pytest.mark.parametrize("kind", ["plain", "ties", "specials", "nothing"])
@pytest.mark.parametrize("top_k", [1, 5, 16])
def test_selection_equals_the_restatement(kind, top_k):
    rng = np.random.default_rng(len(kind) * 100 + top_k)
    score, poses = _synthetic(rng, kind)
    for sep_m, sep_rad in ((0.9, math.radians(7.5)), (0.0, 0.0), (0.51, math.radians(4.1)), (100.0, math.pi)):
        got = selectPoses(score, poses, top_k, sep_m, sep_rad)
        want = psn.select(score, poses, top_k, sep_m, sep_rad)
        assert np.array_equal(got, want), (kind, top_k, sep_m, got, want)
        assert len(got) <= top_k and all(score[c] > 0 for c in got)
        if kind == "nothing":
            assert len(got) == 0
        elif sep_m == 100.0 and sep_rad == math.pi and kind != "specials":
            assert len(got) == 1            # every candidate is closer than the separation to the best one
        elif sep_m == 0.0:
            assert len(got) == top_k        # nothing is closer than zero: the top_k best scores
            assert np.array_equal(score[got], np.sort(score[score > 0])[::-1][:top_k])


def test_selection_errors():
    score, poses = _synthetic(np.random.default_rng(5), "plain")
    for k in (0, 17, -1):
        with pytest.raises(RegistrationError):
            selectPoses(score, poses, k)
    with pytest.raises(RegistrationError):
        selectPoses(score, poses, 4, math.nan, 0.1)
    lib = _capi.load()
    kept = (C.c_int32 * 16)(*([9] * 16))
    n = C.c_int(9)
    s = score.ctypes.data_as(C.POINTER(C.c_double))
    p16 = np.ascontiguousarray(poses.transpose(0, 2, 1)).reshape(-1, 16)
    p = p16.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.lsr_select_poses(None, p, 10, 4, 1.0, 0.1, kept, C.byref(n)) == ERR_INVALID_ARGUMENT
    assert lib.lsr_select_poses(s, None, 10, 4, 1.0, 0.1, kept, C.byref(n)) == ERR_INVALID_ARGUMENT
    assert lib.lsr_select_poses(s, p, 0, 4, 1.0, 0.1, kept, C.byref(n)) == ERR_INVALID_ARGUMENT
    assert lib.lsr_select_poses(s, p, 10, 4, 1.0, 0.1, None, C.byref(n)) == ERR_INVALID_ARGUMENT
    assert lib.lsr_select_poses(s, p, 10, 4, 1.0, 0.1, kept, None) == ERR_INVALID_ARGUMENT
    assert n.value == 9 and list(kept) == [9] * 16


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_keys_and_structs():
    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name, n_args in (("lsr_ndt_score_poses", 5), ("lsr_pose_lattice_poses", 5), ("lsr_select_poses", 8), ("lsr_ndt_search_pose", 6)):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\bint " + name + r"\(", hdr)
        assert len(getattr(lib, name).argtypes) == n_args
    assert _capi.POSE_SEARCH_MS == 23 and re.search(r"LSR_POSE_SEARCH_MS\s*=\s*23\b", hdr)
    assert _capi.POSE_SEARCH_MAX_POSES == 1 << 20 and "#define LSR_POSE_SEARCH_MAX_POSES (1 << 20)" in hdr
    assert _capi.POSE_SEARCH_MAX_KEPT == 16 and "#define LSR_POSE_SEARCH_MAX_KEPT 16" in hdr
    assert C.sizeof(_capi.PoseLattice) == 56 and C.sizeof(_capi.PoseSearchParams) == 80
    assert C.sizeof(_capi.PoseSearchReport) == 16 + 64 + 128 + 1024 + 16 * C.sizeof(_capi.Result)
    assert "typedef struct lsr_pose_lattice { int32_t n[3]; double step[3]; int32_t n_yaw; double yaw_step; } lsr_pose_lattice;" in hdr


def test_null_handle_is_refused():
    lib = _capi.load()
    score = np.full(2, 5.0)
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(-1), (2, 1))
    assert lib.lsr_ndt_score_poses(None, poses.ctypes.data_as(C.POINTER(C.c_float)), 2, score.ctypes.data_as(C.POINTER(C.c_double)), None) == ERR_INVALID_ARGUMENT
    assert b"null handle" in lib.lsr_last_error() and np.all(score == 5.0)
    best = np.full(16, 3.0, np.float32)
    res = _capi.Result()
    prm = _capi.PoseSearchParams(_capi.PoseLattice((C.c_int32 * 3)(1, 1, 1), (C.c_double * 3)(1, 1, 1), 1, 0.0), 4, 1.0, 0.1)
    assert lib.lsr_ndt_search_pose(None, poses.ctypes.data_as(C.POINTER(C.c_float)), C.byref(prm), best.ctypes.data_as(C.POINTER(C.c_float)),
                                   C.byref(res), None) == ERR_INVALID_ARGUMENT
    assert b"null handle" in lib.lsr_last_error() and np.all(best == 3.0)


def test_python_surfaces():
    import inspect

    from lidarslam_ros2_amd import Localizer, NormalDistributionsTransform

    for name in ("scorePoses", "searchPose", "poseLattice", "selectPoses"):
        assert hasattr(NormalDistributionsTransform, name)
    sig = inspect.signature(Localizer.relocalize)
    assert sig.parameters["top_k"].default == 16 and sig.parameters["half_extent"].default == (10.0, 10.0, 0.0)
    assert sig.parameters["yaw_half_range"].default == math.pi and sig.parameters["center"].default is None


# ---- the guard of the GPU search test's inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, d", psn.INPUTS)
def test_oracle_procedure_finds_the_truth_on_the_gpu_inputs(seed, d):
    """tests/test_pose_search_gpu.py asserts that the device's search ends at the truth: that is a statement about the kernel only on
    inputs where the procedure itself — on the CPU oracle — does.  Bars: 0.01 m (trans_eps of the schedule) and 1e-3 rad of heading,
    the angle the lattice searches; measured at most 0.0077 m and 7.4e-4 rad over the six inputs.  (The whole rotation angle of
    pose_delta is printed next to it: 0.9e-3 to 1.1e-3 rad on all six, of which 1.0e-3 is pitch — where NDT's optimum on these scans
    lies for every start inside the true basin, lattice or no lattice; a second, wrong basin would show as metres and degrees.)"""
    from oracle import oracle as O

    case = psn.case(seed)
    grid = O.VoxelGridCovariance(case.target, psn.RES)
    found = psn.oracle_search(O, grid, case.source, psn.displaced_center(case.truth, d))
    assert len(found["kept"]) == psn.TOP_K
    final = found["refined"][found["winner"]]["final"]
    dt, dr = pose_delta(final, case.truth)
    dyaw = abs(psn.yaw_of(final) - psn.yaw_of(case.truth))
    print(f"seed {seed} displacement {d}: oracle winner rank {found['winner']}, {dt:.4f} m, yaw {dyaw:.2e} rad, whole rotation {dr:.2e} rad from the truth")
    assert dt < 0.01 and dyaw < 1e-3 and dr < 2e-3


def test_cpp_snippet_compiles_and_links(tmp_path):
    """the block of tests/cpp/pose_search_snippets.cpp, compiled against include/lidarslam_reg.h and registration.hpp
    (scorePoses, searchPose) and linked against the library; the program runs the lattice, the selection and the refusals that need no
    device."""
    import subprocess
    import textwrap

    src = os.path.join(ROOT, "tests", "cpp", "pose_search_snippets.cpp")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "pose_search_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0 and "POSE_SEARCH_SNIPPETS ok=3 refused=3 surface=1" in run.stdout, (run.stdout, run.stderr)
    text, doc = open(src).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("### 3k.")[1]
    block = text.split("// [pose-search-snippet begin: relocalise]\n")[1].split("  // [pose-search-snippet end: relocalise]")[0]
    assert textwrap.dedent(block).strip("\n").rstrip() in textwrap.dedent(section.split("```c\n")[1].split("```")[0])

"""CPU: the pose-graph optimisation without a GPU — the numpy restatement (tests/pose_graph_numpy.py) against central
differences and a known answer, csrc/pose_graph_edge.hpp built for the host (tools/pose_graph_host_emu) against the restatement, the
host helper lsr_pose_graph_edges against the loop of graph_based_slam_component.cpp:289-303, and the C ABI's symbols and argument
checks.  The kernels themselves: tests/test_pose_graph_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_graph_cases as PC
import pose_graph_numpy as O

ROOT = PC.ROOT


def _random_edges(n=50, seed=7):
    """(Z, X_from, X_to): translations ~ N(0, 3 m), rotation part of the increment ~ N(0, 0.4)"""
    rng = np.random.default_rng(seed)
    return [tuple(PC.rand_pose(rng, 3.0, 0.4) for _ in range(3)) for _ in range(n)]


def _negative_w_edge():
    """an edge whose raw quaternion product q_z (x) q_a has w < 0: the error is turned by more than pi between the two factors"""
    rz = np.eye(4)
    rz[:3, :3] = O.q2R(np.cos(1.3), np.array([0.0, 0.0, np.sin(1.3)]))     # 2.6 rad about z
    Z = O.inv(rz)                                                          # Z^-1 turns by +2.6 rad
    Xi = np.eye(4)
    Xi[:3, 3] = [1.0, -2.0, 0.5]
    Xj = Xi @ rz
    Xj[:3, 3] += [0.3, 0.1, -0.2]
    assert O.raw_product_w(Z, Xi, Xj) < 0
    return Z, Xi, Xj


def test_oracle_jacobians_match_central_differences():
    """The analytic Jacobians of the restatement are the derivatives of its own error under its own update: central differences with
    h = 1e-6 truncate at h^2 * (third derivative) ~ 1e-10 and round at eps * |e| / h ~ 1e-9; the tolerance is 1e-7."""
    worst = 0.0
    for Z, Xi, Xj in _random_edges():
        Ji, Jj = O.jacobians(Z, Xi, Xj)
        Ni, Nj = O.numeric_jacobians(Z, Xi, Xj)
        worst = max(worst, np.abs(Ji - Ni).max(), np.abs(Jj - Nj).max())
    print("analytic vs central differences, max:", worst)
    assert worst < 1e-7


def test_host_emu_error_and_jacobians_match_the_oracle():
    """csrc/pose_graph_edge.hpp on the host against the restatement, 50 random edges and the edge with a negative raw product:
    both are fp64 evaluations of the same formulas in different operation orders -> 1e-12."""
    cases = _random_edges() + [_negative_w_edge()]
    worst = 0.0
    for Z, Xi, Xj in cases:
        e, Jf, Jt = PC.emu_linearize(Z, Xi, Xj)
        Ji, Jj = O.jacobians(Z, Xi, Xj)
        worst = max(worst, np.abs(e - O.error(Z, Xi, Xj)).max(), np.abs(Jf - Ji).max(), np.abs(Jt - Jj).max())
        assert np.array_equal(PC.emu_error(Z, Xi, Xj), e)      # the trial kernel's error is the linearisation's
        assert e[3:] @ e[3:] <= 1.0 and O.R2q(( O.inv(Z) @ O.inv(Xi) @ Xj)[:3, :3])[0] >= 0
    print("host emu vs oracle, max:", worst)
    assert worst < 1e-12


def test_host_emu_update_matches_the_oracle():
    """X (+) delta, including an increment with |dq|^2 > 1 (identity rotation, translation applied) and one exactly on the sphere."""
    rng = np.random.default_rng(9)
    incs = [np.concatenate([rng.normal(size=3), rng.normal(size=3) * 0.3]) for _ in range(20)]
    incs.append(np.array([0.5, -0.25, 2.0, 0.8, 0.7, 0.1]))          # |dq|^2 = 1.14
    incs.append(np.array([0.1, 0.2, 0.3, 0.0, 0.0, 1.0]))            # w = 0: a turn by pi
    assert incs[-2][3:] @ incs[-2][3:] > 1
    for d in incs:
        X = PC.rand_pose(rng, 3.0, 0.4)
        got, want = PC.emu_oplus(X, d), O.oplus(X, d)
        assert np.abs(got - want).max() < 1e-12
        assert np.array_equal(got[3], [0, 0, 0, 1])
    X = PC.rand_pose(rng, 3.0, 0.4)
    big = PC.emu_oplus(X, incs[-2])
    assert np.abs(big[:3, :3] - X[:3, :3]).max() < 1e-15      # identity rotation
    assert np.abs(big[:3, 3] - (X[:3, :3] @ incs[-2][:3] + X[:3, 3])).max() < 1e-12


def _c_edges(lib, poses, k, capacity=None):
    from lidarslam_ros2_amd import _capi

    P = np.ascontiguousarray(np.asarray(poses, np.float64).transpose(0, 2, 1).reshape(len(poses), 16))
    want = max(0, len(poses) - k - 1) * k
    cap = want if capacity is None else capacity
    out = (_capi.PoseEdge * max(cap, 1))()
    n_out = C.c_size_t(12345)
    st = lib.lsr_pose_graph_edges(P.ctypes.data_as(C.POINTER(C.c_double)), len(poses), k, out, cap, C.byref(n_out))
    return st, n_out.value, out


@pytest.mark.parametrize("n", [1, 5, 6, 7, 40])
def test_pose_graph_edges_match_the_reference_loop(n):
    """lsr_pose_graph_edges against the loop of :289-303 restated in the oracle: the same pairs in the same order, measurements within
    1e-12 (two fp64 products of the same matrices); nothing for i <= k."""
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    rng = np.random.default_rng(n)
    poses = [PC.rand_pose(rng, 10.0, 0.4) for _ in range(n)]
    want = O.adjacent_edges(poses, 5)
    st, cnt, out = _c_edges(lib, poses, 5)
    assert st == 0 and cnt == len(want) == max(0, n - 6) * 5
    for e, (a, b, Z) in zip(out[:cnt], want):
        assert (e.from_, e.to) == (a, b) and b > 5
        assert np.abs(np.array(e.measurement[:]).reshape(4, 4, order="F") - Z).max() < 1e-12
    if n <= 6:
        assert cnt == 0


def test_pose_graph_edges_report_a_capacity_overflow_and_bad_arguments():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    poses = [np.eye(4)] * 10
    st, cnt, out = _c_edges(lib, poses, 5, capacity=19)
    assert st == -1 and cnt == 20 and b"capacity" in lib.lsr_last_error()
    assert all(e.from_ == 0 and e.to == 0 for e in out[:19])            # untouched
    n_out = C.c_size_t()
    assert lib.lsr_pose_graph_edges(None, 3, 5, None, 0, C.byref(n_out)) == -1
    P = np.zeros(16)
    dp = P.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.lsr_pose_graph_edges(dp, 0, 5, None, 0, C.byref(n_out)) == -1
    assert lib.lsr_pose_graph_edges(dp, 1, 0, None, 0, C.byref(n_out)) == -1
    assert lib.lsr_pose_graph_edges(dp, 1, 5, None, 0, None) == -1
    assert lib.lsr_pose_graph_edges(dp, 1, 5, None, 0, C.byref(n_out)) == 0 and n_out.value == 0


def test_symbols_argtypes_and_null_handle():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name in ("lsr_pose_graph_edges", "lsr_optimize_pose_graph"):
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr)
        assert getattr(lib, name).argtypes is not None
    assert len(lib.lsr_optimize_pose_graph.argtypes) == 9 and len(lib.lsr_pose_graph_edges.argtypes) == 6
    assert C.sizeof(_capi.PoseEdge) == 8 + 16 * 8 and C.sizeof(_capi.PoseGraphResult) == 48 and C.sizeof(_capi.PoseGraphTrace) == 32
    for key, macro in (("POSE_GRAPH_MAX_VERTICES", "LSR_POSE_GRAPH_MAX_VERTICES"), ("POSE_GRAPH_MAX_BAND", "LSR_POSE_GRAPH_MAX_BAND"),
                       ("POSE_GRAPH_MAX_OFFBAND_EDGES", "LSR_POSE_GRAPH_MAX_OFFBAND_EDGES")):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == getattr(_capi, key)
    assert _capi.POSE_GRAPH_MAX_VERTICES >= 4096 and _capi.POSE_GRAPH_MAX_BAND >= 8 and _capi.POSE_GRAPH_MAX_OFFBAND_EDGES >= 64
    assert ":267-319" in hdr and ":289-303" in hdr
    assert lib.lsr_optimize_pose_graph(None, None, 0, None, 0, None, None, None, None) == -1
    assert b"null handle" in lib.lsr_last_error()


def test_known_answer_the_oracle_returns_the_truth():
    """12 vertices on a radius-5 circle, edges i -> i+1 and 0 -> 11 measured from the true poses, start perturbed by N(0, 0.2 m) /
    N(0, 0.02): the minimum is chi2 = 0 at the truth, and ten iterations reach it within 1e-9."""
    GT, X, E = PC.known_answer_graph()
    assert max(np.abs(a - b).max() for a, b in zip(X[1:], GT[1:])) > 0.05
    Y, trace, res = O.optimize(X, E)
    worst = max(np.abs(a - b).max() for a, b in zip(Y, GT))
    print("known answer: max |pose - truth| =", worst, "chi2", res["chi2_before"], "->", res["chi2_after"])
    assert res["iterations"] == 10 and worst < 1e-9
    assert np.array_equal(Y[0], GT[0])


def test_python_surface_without_a_device():
    """adjacent_edges through the package, and MapArray.pose_adjustment's edge list against a registration object that records it."""
    from lidarslam_ros2_amd import pose_graph
    from lidarslam_ros2_amd.loop_closure import LoopEdge
    from lidarslam_ros2_amd.map_array import MapArray
    from lidarslam_ros2_amd.posemath import matrix_from_pose

    rng = np.random.default_rng(4)
    ma = MapArray()
    for i in range(9):
        ma.append(np.zeros((2, 8), np.float32), PC.rand_pose(rng, 5.0, 0.3), float(i))
    stored = ma.stored_poses()
    assert np.array_equal(stored[3], matrix_from_pose(ma.submaps[3].position, ma.submaps[3].orientation))
    got = pose_graph.adjacent_edges(stored, 5)
    want = O.adjacent_edges(list(stored), 5)
    assert [(a, b) for a, b, _ in got] == [(a, b) for a, b, _ in want] and len(got) == 15

    class Recorder:
        def optimizePoseGraph(self, poses, edges, max_iterations, band):
            self.args = (poses, edges, max_iterations, band)
            return poses + 1.0, "result"

    rec, results = Recorder(), []
    Zl = PC.rand_pose(rng, 1.0, 0.1)
    loops = [LoopEdge((1, 8), Zl, 0.5, True), LoopEdge((2, 8), np.eye(4), 3.0, False)]
    out = ma.pose_adjustment(rec, loops, result=results)
    poses, edges, iters, band = rec.args
    assert np.array_equal(out, stored + 1.0) and results == ["result"] and (iters, band) == (10, 5)
    assert len(edges) == 16 and edges[-1][:2] == (1, 8) and np.array_equal(edges[-1][2], Zl)     # the rejected evaluation is no edge


def test_integration_md_pose_graph_snippet_compiles_and_links(tmp_path):
    """doPoseAdjustment with g2o removed is the block of tests/cpp/pose_graph_snippets.cpp, compiled against
    include/lidarslam_reg/pose_graph.hpp (+ map_assembly.hpp) and linked against the library; the program itself makes the odometry
    edges on the host and shows the adapter refusing a call without a handle (no device needed)."""
    import subprocess
    import textwrap

    src = os.path.join(ROOT, "tests", "cpp", "pose_graph_snippets.cpp")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "pose_graph_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "POSE_GRAPH_SNIPPETS edges=10 shape=1 refused=1 kept=3" in run.stdout, (run.stdout, run.stderr)
    assert "null handle" in run.stderr
    text, doc = open(src).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = text.split("// [pose-graph-snippet begin: do_pose_adjustment]\n")[1].split("// [pose-graph-snippet end: do_pose_adjustment]")[0]
    assert textwrap.dedent(block).strip("\n").rstrip() in doc
    assert ":267-319" in doc and 'optimizer.save("pose_graph.g2o")' in doc

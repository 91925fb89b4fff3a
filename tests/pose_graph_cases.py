"""TEST INFRASTRUCTURE shared by tests/test_pose_graph_cpu.py and tests/test_pose_graph_gpu.py: the host build of
csrc/pose_graph_edge.hpp (tools/pose_graph_host_emu) and the synthetic graphs, each generated from a seed."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import pose_graph_numpy as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def build_emu():
    """g++ -O2 -ffp-contract=off of tools/pose_graph_host_emu/harness.cpp (csrc/pose_graph_edge.hpp for the host)."""
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(ROOT, "tools", "pose_graph_host_emu", "harness.cpp")
    hdr = os.path.join(ROOT, "lidarslam_ros2_amd", "csrc", "pose_graph_edge.hpp")
    out = os.path.join(tempfile.gettempdir(), "lsr_pose_graph_host_emu_%d_%s" % (os.getuid(), hashlib.sha1(ROOT.encode()).hexdigest()[:10]))
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libposegraphemu.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in (src, hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                               src, "-o", so + ".tmp"])
        os.replace(so + ".tmp", so)
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.emu_pg_error.argtypes = [dp, dp, dp, dp]
    L.emu_pg_linearize.argtypes = [dp, dp, dp, dp, dp, dp]
    L.emu_pg_oplus.argtypes = [dp, dp, dp]
    L.emu_pg_quat_from_matrix.argtypes = [dp, dp]
    for f in (L.emu_pg_error, L.emu_pg_linearize, L.emu_pg_oplus, L.emu_pg_quat_from_matrix):
        f.restype = None
    _lib = L
    return L


def _col16(M):
    return np.ascontiguousarray(np.asarray(M, np.float64).T.reshape(16))


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def emu_linearize(Z, Xi, Xj):
    """-> (e (6,), J_from (6, 6), J_to (6, 6)) by the device's arithmetic on the host"""
    L = build_emu()
    z, a, b = _col16(Z), _col16(Xi), _col16(Xj)
    e, jf, jt = np.zeros(6), np.zeros(36), np.zeros(36)
    L.emu_pg_linearize(_p(z), _p(a), _p(b), _p(e), _p(jf), _p(jt))
    return e, jf.reshape(6, 6), jt.reshape(6, 6)


def emu_error(Z, Xi, Xj):
    L = build_emu()
    z, a, b = _col16(Z), _col16(Xi), _col16(Xj)
    e = np.zeros(6)
    L.emu_pg_error(_p(z), _p(a), _p(b), _p(e))
    return e


def emu_oplus(X, d):
    L = build_emu()
    x, dd, out = _col16(X), np.ascontiguousarray(d, np.float64), np.zeros(16)
    L.emu_pg_oplus(_p(x), _p(dd), _p(out))
    return out.reshape(4, 4).T.copy()


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
def rand_pose(rng, sigma_t, sigma_r):
    """translation ~ N(0, sigma_t), rotation part of the increment ~ N(0, sigma_r)"""
    return O.from_mqt(np.concatenate([rng.normal(size=3) * sigma_t, rng.normal(size=3) * sigma_r]))


def circle(n, radius, per_lap, dz):
    out = []
    for i in range(n):
        th = 2 * np.pi * i / per_lap
        T = np.eye(4)
        T[:3, :3] = O.q2R(np.cos(th / 2), np.array([0, 0, np.sin(th / 2)]))
        T[:3, 3] = [radius * np.cos(th) - radius, radius * np.sin(th), dz * i]
        out.append(T)
    return out


def chain_graph(n, sigma_t, sigma_r, seed):
    """n vertices on a radius-5 circle, edges i -> i+1 and 0 -> n-1 measured from the true poses, vertices 1 .. n-1 start perturbed.
    -> (truth, start, edges)"""
    rng = np.random.default_rng(seed)
    GT = circle(n, 5.0, n, 0.1)
    edges = [(i, i + 1, O.inv(GT[i]) @ GT[i + 1]) for i in range(n - 1)] + [(0, n - 1, O.inv(GT[0]) @ GT[n - 1])]
    start = [GT[0]] + [GT[i] @ rand_pose(rng, sigma_t, sigma_r) for i in range(1, n)]
    return GT, start, edges


def known_answer_graph():
    """12 vertices, start error N(0, 0.2 m) / N(0, 0.02): the optimum is the truth"""
    return chain_graph(12, 0.2, 0.02, 1)


def drifted(GT, sigma_t, sigma_r, rng):
    X = [GT[0]]
    for i in range(1, len(GT)):
        X.append(X[-1] @ O.inv(GT[i - 1]) @ GT[i] @ rand_pose(rng, sigma_t, sigma_r))
    return X


REFERENCE_LOOPS = [(0, 100), (3, 104), (3, 104), (50, 151), (97, 199), (195, 199)]


def reference_graph(n=200, loops=REFERENCE_LOOPS, seed=3, k=O.NUM_ADJACENT, per_lap=100):
    """The reference's graph shape: n vertices, two laps round a radius-30 circle, drift N(0, 0.03 m) / N(0, 0.002) composed per step,
    the odometry edges of :289-303 from the drifted poses and loop edges measured from the truth.  -> (truth, start, edges)"""
    rng = np.random.default_rng(seed)
    GT = circle(n, 30.0, per_lap, 0.02)
    X = drifted(GT, 0.03, 0.002, rng)
    return GT, X, O.adjacent_edges(X, k) + [(a, b, O.inv(GT[a]) @ GT[b]) for a, b in loops]


def quirk_graph():
    """40 vertices once round a radius-20 circle, k = 5, one loop edge 1 -> 39: vertex 1 has no odometry edge (i > k is strict), so the
    loop edge drags it"""
    rng = np.random.default_rng(0)
    GT = circle(40, 20.0, 40, 0.1)
    X = drifted(GT, 0.05, 0.004, rng)
    return GT, X, O.adjacent_edges(X, 5) + [(1, 39, O.inv(GT[1]) @ GT[39])]


REJECT_SEED = 2


def rejected_step_graph(seed=REJECT_SEED):
    """16 vertices, start error N(0, 5 m) / N(0, 0.45): far enough for the controller to reject steps"""
    return chain_graph(16, 5.0, 0.45, seed)

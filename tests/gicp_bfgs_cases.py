"""TEST INFRASTRUCTURE shared by tests/test_gicp_bfgs_cpu.py and tests/test_gicp_bfgs_gpu.py: the host build of csrc/gicp_bfgs.hpp
(tools/gicp_bfgs_host_emu), the analytic test functions it carries, and the automaton driven from python."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tools", "gicp_bfgs_host_emu")
HDR = os.path.join(ROOT, "lidarslam_ros2_amd", "csrc", "gicp_bfgs.hpp")
_lib = None

CALLBACK = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)

# branches of the line search (csrc/gicp_bfgs.hpp: BFGS_V_*)
V = dict(bracket_armijo=1, bracket_accept=2, bracket_uphill=4, bracket_extend=8, section_shrink=16, section_accept=32,
         section_move=64, cubic=128, quadratic=256, section_no_progress=512, cap=1024)
REASONS = {0: "running", 1: "no_progress", 2: "gradient_tolerance", 3: "max_inner", 4: "non_finite"}

# the analytic functions of the harness and where each run starts
QUADRATIC, ROSENBROCK, OVERSHOOT, NAN_BEYOND = 0, 1, 2, 3
EMU_C = [0.7, -0.4, 0.25, 0.1, -0.2, 0.05]
STARTS = {QUADRATIC: [0.0] * 6, ROSENBROCK: [-1.2, 1.0, -1.2, 1.0, -1.2, 1.0],
          OVERSHOOT: [c + d for c, d in zip(EMU_C, [0.3, -0.2, 0.25, 0.15, -0.3, 0.2])], NAN_BEYOND: [0.0] * 6}


def out_dir():
    d = os.path.join(tempfile.gettempdir(), "lsr_gicp_bfgs_host_emu_%d_%s" % (os.getuid(), hashlib.sha1(ROOT.encode()).hexdigest()[:10]))
    os.makedirs(d, exist_ok=True)
    return d


def _stale(target, sources):
    return not os.path.exists(target) or os.path.getmtime(target) < max(os.path.getmtime(p) for p in sources)


def build_emu():
    """g++ -O2 -ffp-contract=off of tools/gicp_bfgs_host_emu/harness.cpp (csrc/gicp_bfgs.hpp for the host)."""
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(EMU_DIR, "harness.cpp")
    so = os.path.join(out_dir(), "libgicpbfgsemu.so")
    if _stale(so, (src, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                               src, "-o", so + ".tmp"])
        os.replace(so + ".tmp", so)
    L = C.CDLL(so)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.emu_bfgs_run.argtypes = [dp, C.c_int, C.c_void_p, C.c_void_p, C.c_int, dp, dp, ip, ip, ip, ip, dp, dp, dp]
    L.emu_bfgs_run.restype = C.c_int
    L.emu_bfgs_test_function.argtypes = [dp, dp, dp, C.c_void_p]
    L.emu_bfgs_test_function.restype = None
    L.emu_bfgs_cost_gradient.argtypes = [dp, C.c_int, dp, dp, dp]
    L.emu_bfgs_cost_gradient.restype = None
    _lib = L
    return L


def build_replay():
    """The stand-alone sanitizer program: replay_main.cpp + harness.cpp, -fsanitize=address,undefined.  -> its path"""
    srcs = [os.path.join(EMU_DIR, "replay_main.cpp"), os.path.join(EMU_DIR, "harness.cpp")]
    exe = os.path.join(out_dir(), "gicp_bfgs_replay_san")
    if _stale(exe, srcs + [HDR]):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan",   # the runtimes inside the program: nothing to order at load time
                               "-fno-omit-frame-pointer", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + srcs + ["-o", exe + ".tmp"])
        os.replace(exe + ".tmp", exe)
    return exe


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_function(which):
    """-> fn(x) -> (f, g): analytic function `which` as the harness evaluates it (the automaton's callback computes the same bits)"""
    L = build_emu()
    w = C.c_int(which)

    def fn(x):
        xa, f, g = np.ascontiguousarray(x, np.float64), C.c_double(), np.zeros(6)
        L.emu_bfgs_test_function(_dp(xa), C.byref(f), _dp(g), C.cast(C.byref(w), C.c_void_p))
        return f.value, g.tolist()
    return fn


def run_automaton(fn, x_start, max_inner, capacity=4096):
    """The automaton of csrc/gicp_bfgs.hpp on the host.  fn: an int (analytic function of the harness, called from C) or a python
    callable x -> (f, g).  -> dict(points (e, 6), alphas (e,), inner (e,), n_evals, n_inner, reason, visited, x, f, g)"""
    L = build_emu()
    xs, al, inner = np.zeros((capacity, 6)), np.zeros(capacity), np.zeros(capacity, np.int32)
    ne, ni, vis = C.c_int(), C.c_int(), C.c_int()
    xf, ff, gf = np.zeros(6), C.c_double(), np.zeros(6)
    x0 = np.ascontiguousarray(x_start, np.float64)
    if isinstance(fn, int):
        w = C.c_int(fn)
        cb, user = C.cast(L.emu_bfgs_test_function, C.c_void_p), C.cast(C.byref(w), C.c_void_p)
    else:
        def trampoline(xp, fp, gp, _):
            f, g = fn([xp[k] for k in range(6)])
            fp[0] = f
            for k in range(6):
                gp[k] = g[k]
        keep = CALLBACK(trampoline)
        cb, user = C.cast(keep, C.c_void_p), None
    reason = L.emu_bfgs_run(_dp(x0), int(max_inner), cb, user, capacity, _dp(xs), _dp(al), inner.ctypes.data_as(C.POINTER(C.c_int)),
                            C.byref(ne), C.byref(ni), C.byref(vis), _dp(xf), C.byref(ff), _dp(gf))
    e = min(ne.value, capacity)
    return dict(points=xs[:e].copy(), alphas=al[:e].copy(), inner=inner[:e].copy(), n_evals=ne.value, n_inner=ni.value, reason=int(reason),
                visited=vis.value, x=xf, f=ff.value, g=gf)

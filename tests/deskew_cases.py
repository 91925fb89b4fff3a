"""TEST INFRASTRUCTURE shared by tests/test_deskew_cpu.py and tests/test_deskew_gpu.py: the host build of the de-skew headers
(tools/deskew_host_emu), synthetic scans and IMU streams, and the margins the GPU comparison needs."""
import ctypes as C
import hashlib
import math
import os
import subprocess
import tempfile

import numpy as np

import deskew_numpy as DN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PI = math.pi
T0 = 1000.0          # scan_time of the synthetic scans [s]
_lib = None


def build_emu():
    """g++ -O2 -ffp-contract=off of tools/deskew_host_emu/harness.cpp (csrc/imu_queue.hpp + csrc/deskew_point.hpp for the host)."""
    global _lib
    if _lib is not None:
        return _lib
    src = os.path.join(ROOT, "tools", "deskew_host_emu", "harness.cpp")
    hdrs = [os.path.join(ROOT, "lidarslam_ros2_amd", "csrc", h) for h in ("imu_queue.hpp", "deskew_point.hpp")]
    out = os.path.join(tempfile.gettempdir(), "lsr_deskew_host_emu_%d_%s" % (os.getuid(), hashlib.sha1(ROOT.encode()).hexdigest()[:10]))
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libdeskewemu.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", src, "-o", so + ".tmp"])
        os.replace(so + ".tmp", so)
    L = C.CDLL(so)
    vp, fp, dp, ip, bp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.emu_queue_new.restype = vp
    L.emu_queue_free.argtypes = [vp]
    L.emu_queue_reset.argtypes = [vp, C.c_double]
    L.emu_queue_push.argtypes = [vp, fp, fp, fp, C.c_double]
    L.emu_queue_receive.argtypes = [vp, dp, dp, dp, C.c_double, fp]
    L.emu_queue_info.argtypes = [vp, ip]
    L.emu_queue_dump.argtypes = [vp, dp, fp]
    L.emu_queue_table.argtypes = [vp, dp, fp]
    L.emu_deskew.argtypes = [vp, fp, C.c_int, C.c_double, fp, fp, ip, bp, ip]
    _lib = L
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class EmuQueue:
    """csrc/imu_queue.hpp + the prefix-maximum de-skew of csrc/deskew_point.hpp, on the host."""

    def __init__(self, scan_period=0.1):
        self.L = build_emu()
        self.q = self.L.emu_queue_new()
        self.L.emu_queue_reset(self.q, scan_period)

    def push(self, ang_vel, acc, quat, stamp) -> bool:
        a, b, c = (np.ascontiguousarray(v, F) for v in (ang_vel, acc, quat))
        return self.L.emu_queue_push(self.q, _p(a, C.c_float), _p(b, C.c_float), _p(c, C.c_float), float(stamp)) == 0

    def receive(self, orientation_xyzw, ang_vel, lin_acc, stamp):
        """-> (accepted, ang_vel (3,), acc (3,) with gravity removed, quat w x y z (4,)) as lsr_imu_receive forms them"""
        a, b, c = (np.ascontiguousarray(v, np.float64) for v in (orientation_xyzw, ang_vel, lin_acc))
        s = np.zeros(10, F)
        ok = self.L.emu_queue_receive(self.q, _p(a, C.c_double), _p(b, C.c_double), _p(c, C.c_double), float(stamp), _p(s, C.c_float)) == 0
        return ok, s[0:3].copy(), s[3:6].copy(), s[6:10].copy()

    def info(self):
        i = np.zeros(4, np.int32)
        self.L.emu_queue_info(self.q, _p(i, C.c_int32))
        return dict(count=int(i[0]), last=int(i[1]), last_iter=int(i[2]))

    def dump(self):
        s, f = np.zeros(200), np.zeros((200, 18), F)
        self.L.emu_queue_dump(self.q, _p(s, C.c_double), _p(f, C.c_float))
        return s, f

    def table(self):
        s, f = np.zeros(201), np.zeros((201, 9), F)
        m = self.L.emu_queue_table(self.q, _p(s, C.c_double), _p(f, C.c_float))
        return m, s[: m + 1], f[: m + 1]

    def deskew(self, xyz, scan_time):
        xyz = np.ascontiguousarray(xyz, F)
        n = xyz.shape[0]
        out, rel, slot, sk, info = np.zeros((n, 3), F), np.zeros(n, F), np.full(n, -1, np.int32), np.zeros(n, np.uint8), np.zeros(4, np.int32)
        self.L.emu_deskew(self.q, _p(xyz, C.c_float), n, float(scan_time), _p(out, C.c_float), _p(rel, C.c_float), _p(slot, C.c_int32),
                          _p(sk, C.c_uint8), _p(info, C.c_int32))
        return dict(out=out, rel=rel, slot=slot, skipped=sk, n_skipped=int(info[0]), start_missing=int(info[1]), half_index=int(info[2]),
                    last_iter=int(info[3]))

    def __del__(self):
        try:
            self.L.emu_queue_free(self.q)
        except Exception:
            pass


def ring_fields(ring: DN.ImuRing):
    return ring.stamp.copy(), np.concatenate([ring.rpy, ring.acc, ring.ang_vel, ring.shift, ring.velo, ring.ang_rot], axis=1)


# ---- IMU streams ---------------------------------------------------------------------------------------------------------
def euler_quat(roll, pitch, yaw):
    """w x y z of Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2), math.cos(yaw / 2), math.sin(yaw / 2)
    return np.array([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], F)


def imu_samples(stamps, rng, t_ref=T0):
    """A smooth motion sampled at `stamps`: -> list of (ang_vel, acc, quat, stamp)."""
    w = rng.uniform(-0.6, 0.6, 3)
    a = rng.uniform(-1.5, 1.5, 3)
    out = []
    for s in stamps:
        dt = s - t_ref
        q = euler_quat(0.05 + w[0] * dt, -0.03 + w[1] * dt, 0.4 + w[2] * dt)
        out.append((w.astype(F), (a * (1 + 0.3 * math.sin(7 * dt))).astype(F), q, float(s)))
    return out


def stamps_200hz(t_first, t_last, phase=0.00123):
    k = int(math.floor((t_last - t_first) / 0.005)) + 1
    return t_first + phase + 0.005 * np.arange(k)


# ---- scans ---------------------------------------------------------------------------------------------------------------
def scan_from_delta(delta, start_ori, rng_r, z):
    """points whose -atan2(y, x) is start_ori + delta"""
    az = -(start_ori + delta)
    return np.stack([rng_r * np.cos(az), rng_r * np.sin(az), z], axis=1).astype(F)


def times(xyz, scan_time, period):
    """vectorised f32 / f64 evaluation of ori_h, rel_time and t per point (numpy's arctan2) — used to place points, never as a reference"""
    with np.errstate(all="ignore"):
        ori = (-np.arctan2(xyz[:, 1], xyz[:, 0])).astype(F)
        n = len(ori)
        start, end = ori[0], ori[-1]
        if float(end - start) > 3 * PI:
            end = F(float(end) - 2 * PI)
        elif float(end - start) < PI:
            end = F(float(end) + 2 * PI)
        o64 = ori.astype(np.float64)
        h1 = np.where(o64 < float(start) - PI / 2, (o64 + 2 * PI).astype(F), np.where(o64 > float(start) + 1.5 * PI, (o64 - 2 * PI).astype(F), ori)).astype(F)
        flag = (h1 - start).astype(np.float64) > PI
        H = int(np.argmax(flag)) if flag.any() else n
        b = (o64 + 2 * PI).astype(F)
        b64 = b.astype(np.float64)
        h2 = np.where(b64 < float(end) - 1.5 * PI, (b64 + 2 * PI).astype(F), np.where(b64 > float(end) + 0.5 * PI, (b64 - 2 * PI).astype(F), b)).astype(F)
        h = np.where(np.arange(n) <= H, h1, h2).astype(F)
        rel = (((h - start) / F(end - start)).astype(np.float64) * period).astype(F)
    return dict(ori=ori, start=start, end=end, h1=h1, b=b, h=h, H=H, rel=rel, t=scan_time + rel.astype(np.float64))


def angle_margin(ori, start, end, H):
    """per point: distance of every operand the branch logic compares from its threshold, on the branch the point takes"""
    o = np.asarray(ori, np.float64)
    n = len(o)
    s, e = float(start), float(end)
    with np.errstate(all="ignore"):
        h1 = np.where(o < s - PI / 2, o + 2 * PI, np.where(o > s + 1.5 * PI, o - 2 * PI, o))
        first = np.minimum(np.minimum(np.abs(o - (s - PI / 2)), np.abs(o - (s + 1.5 * PI))), np.abs(h1 - s - PI))
        b = o + 2 * PI
        second = np.minimum(np.abs(b - (e - 1.5 * PI)), np.abs(b - (e + 0.5 * PI)))
    m = np.where(np.arange(n) <= H, first, second)
    return np.where(np.isnan(m), np.inf, m)       # a NaN point takes no branch on either side


def time_margin(t, stamps, period):
    """per point: distance of t from every stamp and every stamp +- period"""
    th = np.sort(np.concatenate([stamps, stamps - period, stamps + period]))
    t = np.asarray(t, np.float64)
    k = np.clip(np.searchsorted(th, t), 1, len(th) - 1)
    with np.errstate(all="ignore"):
        m = np.minimum(np.abs(t - th[k - 1]), np.abs(t - th[k]))
    return np.where(np.isnan(m), np.inf, m)


def make_scan(n, rng, stamps, scan_time=T0, period=0.1, jitter=0.02, sweep=2 * PI * 0.98, start_ori=None, nan_at=None):
    """n points in payload order sweeping `sweep` radians of azimuth with jitter; every point keeps 2e-3 rad from the branch thresholds
    and 2e-6 s from every stamp and stamp +- period (points that do not are moved along the sweep until they do)."""
    start_ori = float(rng.uniform(-3.0, 3.0)) if start_ori is None else start_ori
    delta = sweep * (np.arange(n) / max(n - 1, 1)) + rng.uniform(-jitter, jitter, n)
    delta = np.clip(delta, 1e-2, sweep - 1e-2)
    delta[0] = 0.0
    if n > 1:
        delta[-1] = sweep
    r = rng.uniform(2.0, 60.0, n)
    z = rng.uniform(-2.0, 6.0, n)
    stamps = np.asarray(stamps, np.float64)
    for _ in range(200):
        xyz = scan_from_delta(delta, start_ori, r, z)
        tm = times(xyz, scan_time, period)
        bad = (angle_margin(tm["ori"], tm["start"], tm["end"], tm["H"]) < 2e-3)
        if len(stamps):
            bad |= time_margin(tm["t"], stamps, period) < 2e-6
        bad[0] = False
        if n > 1:
            bad[-1] = False
        if not bad.any():
            break
        delta[bad] += 3.1e-4
    else:
        raise RuntimeError("could not place the points clear of the thresholds")
    if nan_at is not None:
        xyz[nan_at, 0] = np.nan
    return xyz

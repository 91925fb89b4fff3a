"""TEST INFRASTRUCTURE: the frontend's IMU de-skew (LidarUndistortion, scanmatcher/include/scanmatcher/lidar_undistortion.hpp, called
at scanmatcher_component.cpp:204-208 and fed at :501-527) as a literal SEQUENTIAL restatement — a ring of 200 slots, a pointer that
walks forward from where the previous point left it, one loop over the points with a `half_passed` flag — in the number formats the
reference uses: f32 angles / poses / rel_time, f64 stamps, mixed expressions in f64 rounded to f32 when stored.  The device (csrc/
deskew.hip) and its host emulation (tools/deskew_host_emu) compute the same thing as a minimum index and a prefix maximum; the tests
compare them with this walk.  Two definitions the reference leaves open: a fresh ring is zeros, an out-of-order stamp is refused."""
import ctypes as C
import ctypes.util
import math

import numpy as np

F = np.float32
QLEN = 200
PI = math.pi

_m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _n, _k in (("atan2f", 2), ("asinf", 1), ("sinf", 1), ("cosf", 1)):
    getattr(_m, _n).restype = C.c_float
    getattr(_m, _n).argtypes = [C.c_float] * _k


def atan2f(y, x):
    """the C library's float atan2 (what the host build of the headers calls), element by element"""
    y, x = np.asarray(y, F), np.asarray(x, F)
    if y.ndim == 0:
        return F(_m.atan2f(float(y), float(x)))
    return np.array([_m.atan2f(float(a), float(b)) for a, b in zip(y, x)], F)


def quat_to_matrix(q):
    w, x, y, z = (F(v) for v in q)
    tx, ty, tz = F(2) * x, F(2) * y, F(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[F(1) - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, F(1) - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, F(1) - (txx + tyy)]], F)


class ImuRing:
    def __init__(self, scan_period=0.1):
        self.reset(scan_period)

    def reset(self, scan_period=0.1):
        self.scan_period = float(scan_period)
        self.last, self.last_iter, self.count = -1, 0, 0
        self.stamp = np.zeros(QLEN, np.float64)
        self.rpy, self.acc, self.ang_vel = np.zeros((QLEN, 3), F), np.zeros((QLEN, 3), F), np.zeros((QLEN, 3), F)
        self.shift, self.velo, self.ang_rot = np.zeros((QLEN, 3), F), np.zeros((QLEN, 3), F), np.zeros((QLEN, 3), F)

    def push(self, ang_vel, acc, quat_wxyz, stamp) -> bool:
        """False: refused (stamp smaller than the previous push's)"""
        stamp = float(stamp)
        if self.last >= 0 and stamp < self.stamp[self.last]:
            return False
        m = quat_to_matrix(quat_wxyz)
        roll = F(_m.atan2f(float(m[2, 1]), float(m[2, 2])))
        pitch = F(_m.asinf(float(-m[2, 0])))
        yaw = F(_m.atan2f(float(m[1, 0]), float(m[0, 0])))
        self.last = (self.last + 1) % QLEN
        self.count += 1
        L = self.last
        acc, ang_vel = np.asarray(acc, F), np.asarray(ang_vel, F)
        self.stamp[L] = stamp
        self.rpy[L] = (roll, pitch, yaw)
        self.acc[L], self.ang_vel[L] = acc, ang_vel
        aw = [(m[r, 0] * acc[0] + m[r, 1] * acc[1]) + m[r, 2] * acc[2] for r in range(3)]
        back = (L + QLEN - 1) % QLEN
        dt = float(self.stamp[L] - self.stamp[back])
        if dt < self.scan_period:
            for k in range(3):
                self.shift[L, k] = F(float(self.shift[back, k]) + float(self.velo[back, k]) * dt + float(aw[k]) * dt * dt * 0.5)
                self.velo[L, k] = F(float(self.velo[back, k]) + float(aw[k]) * dt)
                self.ang_rot[L, k] = F(float(self.ang_rot[back, k]) + float(ang_vel[k]) * dt)
        return True

    def table(self):
        """-> (m, stamp[m + 1], fields[m + 1, 9] = rpy, shift, velo); row 0 is entry -1"""
        if self.last < 0:
            m = 0
        else:
            m = (self.last - self.last_iter) % QLEN + 1
        slots = [(self.last_iter + QLEN - 1) % QLEN] + [(self.last_iter + k) % QLEN for k in range(m)]
        return m, self.stamp[slots].copy(), np.concatenate([self.rpy[slots], self.shift[slots], self.velo[slots]], axis=1)


def rotation(rpy):
    sr, cr = F(_m.sinf(float(rpy[0]))), F(_m.cosf(float(rpy[0])))
    sp, cp = F(_m.sinf(float(rpy[1]))), F(_m.cosf(float(rpy[1])))
    sy, cy = F(_m.sinf(float(rpy[2]))), F(_m.cosf(float(rpy[2])))
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]], F)


def deskew(ring: ImuRing, xyz, scan_time, coords=True, ori=None):
    """One scan through the sequential walk; advances ring.last_iter.  xyz: (n, 3) f32 in payload order.  `ori` (optional): the
    points' -atan2f(y, x) when the caller has them already.  coords=False: only the discrete results and rel_time (a 146k-point scan
    in a Python loop).  -> dict(out, rel, slot, skipped, half_index, n_skipped, start_missing, last_iter, ori_h, t)"""
    xyz = np.ascontiguousarray(xyz, F)
    n = xyz.shape[0]
    out = xyz.copy()
    rel_a, slot_a, skip_a = np.zeros(n, F), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    orih_a, t_a = np.zeros(n, F), np.zeros(n, np.float64)
    res = dict(out=out, rel=rel_a, slot=slot_a, skipped=skip_a, half_index=-1, n_skipped=0, start_missing=0, last_iter=ring.last_iter,
               ori_h=orih_a, t=t_a, ran=False)
    if n == 0 or ring.last <= 0:
        return res
    res["ran"] = True
    period = ring.scan_period
    if ori is None:
        ori = -atan2f(xyz[:, 1], xyz[:, 0])
    ori = np.asarray(ori, F)
    start, end = ori[0], ori[n - 1]
    if float(end - start) > 3 * PI:
        end = F(float(end) - 2 * PI)
    elif float(end - start) < PI:
        end = F(float(end) + 2 * PI)
    diff = F(end - start)
    res.update(ori=ori, start=start, end=end)
    half_passed, half_index = False, n
    front = ring.last_iter
    have_start = False
    stamp = ring.stamp
    with np.errstate(all="ignore"):
        for i in range(n):
            h = ori[i]
            if not half_passed:
                if float(h) < float(start) - PI * 0.5:
                    h = F(float(h) + 2 * PI)
                elif float(h) > float(start) + PI * 1.5:
                    h = F(float(h) - 2 * PI)
                if float(F(h - start)) > PI:
                    half_passed, half_index = True, i
            else:
                h = F(float(h) + 2 * PI)
                if float(h) < float(end) - 1.5 * PI:
                    h = F(float(h) + 2 * PI)
                elif float(h) > float(end) + 0.5 * PI:
                    h = F(float(h) - 2 * PI)
            rel = F(float(F(F(h - start) / diff)) * period)
            t = scan_time + float(rel)
            orih_a[i], rel_a[i], t_a[i] = h, rel, t
            front = ring.last_iter
            while front != ring.last:
                if t < stamp[front]:
                    break
                front = (front + 1) % QLEN
            slot_a[i] = front
            if abs(t - stamp[front]) > period:
                skip_a[i] = 1
                continue
            if coords or i == 0:
                if t > stamp[front]:
                    rpy, shift, velo = ring.rpy[front].copy(), ring.shift[front].copy(), ring.velo[front].copy()
                else:
                    back = (front + QLEN - 1) % QLEN
                    rf = F((t - stamp[back]) / (stamp[front] - stamp[back]))
                    rb = F(1.0 - float(rf))
                    rpy = ring.rpy[front] * rf + ring.rpy[back] * rb
                    shift = ring.shift[front] * rf + ring.shift[back] * rb
                    velo = ring.velo[front] * rf + ring.velo[back] * rb
                if i == 0:
                    have_start = True
                    shift_s, velo_s, Rs = shift, velo, rotation(rpy)
                elif have_start:
                    Rc = rotation(rpy)
                    d = shift - shift_s - velo_s * rel
                    p = xyz[i]
                    v = [((Rc[r, 0] * p[0] + Rc[r, 1] * p[1]) + Rc[r, 2] * p[2]) + d[r] for r in range(3)]
                    out[i] = [(Rs[0, c] * v[0] + Rs[1, c] * v[1]) + Rs[2, c] * v[2] for c in range(3)]
            ring.last_iter = front
    res.update(half_index=half_index, n_skipped=int(skip_a.sum()), start_missing=int(skip_a[0]), last_iter=ring.last_iter)
    return res


def ref64(xyz, rel, entry, skipped, table_stamp, table_fields, scan_time, start_missing):
    """The coordinates in f64 from the same f32 table and the given rel_time / table entries (vectorised): what a GPU result is
    compared with.  entry: table entry per point (row entry + 1 of the table arrays).  -> (out (n,3) f64, bound scale terms)."""
    xyz64 = np.asarray(xyz, np.float64)
    n = xyz64.shape[0]
    out = xyz64.copy()
    if start_missing or n == 0:
        return out, np.zeros(n), np.zeros(n)
    t = scan_time + np.asarray(rel, np.float64)
    e = np.asarray(entry, np.int64) + 1
    st, fl = np.asarray(table_stamp, np.float64), np.asarray(table_fields, np.float64)
    with np.errstate(all="ignore"):
        direct = t > st[e]
        rf = (t - st[e - 1]) / (st[e] - st[e - 1])
        rf = np.where(direct, 1.0, rf)
        pose = fl[e] * rf[:, None] + fl[e - 1] * (1.0 - rf)[:, None]
        pose[direct] = fl[e][direct]
        r, p, y = pose[:, 0], pose[:, 1], pose[:, 2]
        sr, cr, sp, cp, sy, cy = np.sin(r), np.cos(r), np.sin(p), np.cos(p), np.sin(y), np.cos(y)
        R = np.empty((n, 3, 3))
        R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr
        R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr
        R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -sp, cp * sr, cp * cr
        shift, velo = pose[:, 3:6], pose[:, 6:9]
        d = shift - shift[0] - velo[0] * np.asarray(rel, np.float64)[:, None]
        v = np.einsum("nij,nj->ni", R, xyz64) + d
        moved = v @ R[0]          # R_s^T v, row by row
    keep = np.asarray(skipped, bool).copy()
    keep[0] = True
    out = np.where(keep[:, None], xyz64, moved)
    return out, np.linalg.norm(shift - shift[0], axis=1), np.full(n, np.linalg.norm(velo[0]))

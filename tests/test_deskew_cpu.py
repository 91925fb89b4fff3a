"""IMU de-skew without a GPU: csrc/imu_queue.hpp and csrc/deskew_point.hpp built for the host (tools/deskew_host_emu) against the
sequential restatement tests/deskew_numpy.py, the convention of the whole chain against a rigid-motion model, and the syntax of the
C++ surface."""
import math
import os
import subprocess

import numpy as np

import deskew_cases as DC
import deskew_numpy as DN

ROOT = DC.ROOT
F = np.float32
T0 = DC.T0


def _push_both(emu, ring, sample):
    a, b = emu.push(*sample), ring.push(*sample)
    assert a == b
    return a


def _same_ring(emu, ring):
    s, f = emu.dump()
    rs, rf = DC.ring_fields(ring)
    assert np.array_equal(s, rs)
    assert np.array_equal(f.view(np.uint32), rf.view(np.uint32))
    i = emu.info()
    assert (i["count"], i["last"], i["last_iter"]) == (ring.count, ring.last, ring.last_iter)


def test_queue_parity_wrap_refusal_and_table():
    """(a) 450 pushes wrap the ring twice; a push with a smaller stamp is refused by both and stored nowhere; a gap >= scan_period leaves
    the integrals of the slot as they were; the linearised table is the ring slots last_iter .. last with entry -1 in front."""
    rng = np.random.default_rng(11)
    emu, ring = DC.EmuQueue(0.1), DN.ImuRing(0.1)
    assert emu.table()[0] == 0 and ring.table()[0] == 0
    stamps = T0 + 0.005 * np.arange(450) + np.where(np.arange(450) >= 300, 0.25, 0.0)   # one gap of more than scan_period
    samples = DC.imu_samples(stamps, rng)
    for k, s in enumerate(samples):
        assert _push_both(emu, ring, s)
        if k in (0, 1, 199, 200, 201, 299, 300, 301, 449):
            _same_ring(emu, ring)
        if k == 120:
            stale = (s[0], s[1], s[2], s[3] - 1e-3)
            assert not _push_both(emu, ring, stale)
            _same_ring(emu, ring)
            assert _push_both(emu, ring, (s[0], s[1], s[2], s[3]))      # an equal stamp is in order
    _same_ring(emu, ring)
    assert ring.count == 451 and ring.last == 450 % 200
    for last_iter in (0, 17, ring.last, ring.last + 1, 199):
        ring.last_iter = last_iter
        m, st, fl = ring.table()
        assert m == (ring.last - last_iter) % 200 + 1
        assert st[0] == ring.stamp[(last_iter + 199) % 200] and st[1] == ring.stamp[last_iter] and st[m] == ring.stamp[ring.last]
    ring.last_iter = 0
    m, st, fl = emu.table()
    rm, rst, rfl = ring.table()
    assert m == rm and np.array_equal(st, rst) and np.array_equal(fl.view(np.uint32), rfl.view(np.uint32))


def _gap_stream(rng, t0):
    """dense stamps up to t0 + 0.02, then the next stamp at t0 + 0.2: a gap of more than scan_period inside the table"""
    st = np.concatenate([DC.stamps_200hz(t0 - 0.06, t0 + 0.02 - 0.00123), [t0 + 0.2, t0 + 0.205]])
    return DC.imu_samples(st, rng, t0)


def _compare(e, r):
    assert e["half_index"] == r["half_index"]
    assert np.array_equal(e["slot"], r["slot"])
    assert np.array_equal(e["skipped"], r["skipped"])
    assert (e["n_skipped"], e["start_missing"], e["last_iter"]) == (r["n_skipped"], r["start_missing"], r["last_iter"])
    assert np.array_equal(e["rel"].view(np.uint32), r["rel"].view(np.uint32))
    assert np.array_equal(e["out"].view(np.uint32), r["out"].view(np.uint32))


def test_prefix_maximum_equals_the_sequential_walk():
    """(b) H as a minimum index and the pointer as a prefix maximum of f' give, exactly, the half index, the slot per point, the skip
    mask and the final last_iter of the walk — on random non-decreasing tables, the gap table, azimuth jitter of several IMU periods (a
    skipped point with a high f in front of a valid point with a lower one), a NaN point in mid-scan, and two scans on one queue."""
    seen_inversion = False
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        emu, ring = DC.EmuQueue(0.1), DN.ImuRing(0.1)
        if seed % 3 == 0:
            samples = _gap_stream(rng, T0)
        else:
            st = np.sort(T0 + rng.uniform(-0.15, 0.3, int(rng.integers(2, 150))))
            if seed % 3 == 2:
                st[len(st) // 2:] = np.maximum(st[len(st) // 2:], st[len(st) // 2 - 1])   # repeated stamps are in order too
            samples = DC.imu_samples(st, rng)
        for s in samples:
            assert _push_both(emu, ring, s)
        for scan, t0 in enumerate((T0, T0 + 0.1)):
            n = int(rng.integers(300, 700))
            xyz = DC.make_scan(n, rng, [], scan_time=t0, jitter=0.9, nan_at=(n // 2 if seed % 2 else None))
            if scan == 1:
                for s in DC.imu_samples(T0 + 0.31 + 0.005 * np.arange(int(rng.integers(0, 30))), rng):
                    assert _push_both(emu, ring, s)
            m, st, fl = ring.table()
            r = DN.deskew(ring, xyz, t0)
            e = emu.deskew(xyz, t0)
            _compare(e, r)
            assert r["ran"] and 0 <= r["half_index"] <= n
            # the case the f' construction exists for: a skipped point whose f lies beyond the pointer, then a moved point behind it
            f = np.array([next((k for k in range(m) if t < st[1 + k]), m - 1) if not math.isnan(t) else m - 1 for t in r["t"]])
            sk = r["skipped"].astype(bool)
            for i in np.nonzero(sk)[0]:
                later = np.nonzero(~sk[i + 1:])[0]
                if len(later) and f[i + 1 + later[0]] < f[i]:
                    seen_inversion = True
    assert seen_inversion


def test_short_queue_moves_nothing():
    """n == 0 and last <= 0 (no sample, one sample): the reference's loop body never runs."""
    rng = np.random.default_rng(3)
    xyz = DC.make_scan(100, rng, [])
    for pushes in (0, 1):
        emu, ring = DC.EmuQueue(0.1), DN.ImuRing(0.1)
        for s in DC.imu_samples(T0 + 0.005 * np.arange(pushes), rng):
            _push_both(emu, ring, s)
        e, r = emu.deskew(xyz, T0), DN.deskew(ring, xyz, T0)
        _compare(e, r)
        assert np.array_equal(e["out"].view(np.uint32), xyz.view(np.uint32)) and e["last_iter"] == 0 and not r["ran"]
    e = DC.EmuQueue(0.1).deskew(np.zeros((0, 3), F), T0)
    assert e["out"].shape == (0, 3)


def test_convention_pure_rotation():
    """(c) A sensor turning at constant yaw and pitch rates in front of fixed world points.  The IMU reports its orientation at 200 Hz;
    point i is measured at t_i (from its azimuth, by the de-skew's own formula) as p_i = R(t_i)^-1 P_w.  De-skewing must return every
    point in the frame of the scan's first instant: R(t_0)^-1 P_w.  Bound per point: 64 * 2^-24 * |p| (the rounding of the f32
    sines, cosines and the two rotations; the rpy interpolation is exact for constant rates up to the f32 ratio)."""
    rng = np.random.default_rng(5)
    yaw_rate, pitch_rate = 0.9, -0.35

    def Rw(t):
        y, p = 0.3 + yaw_rate * (t - T0), 0.1 + pitch_rate * (t - T0)
        Rz = np.array([[math.cos(y), -math.sin(y), 0], [math.sin(y), math.cos(y), 0], [0, 0, 1]])
        Ry = np.array([[math.cos(p), 0, math.sin(p)], [0, 1, 0], [-math.sin(p), 0, math.cos(p)]])
        return Rz @ Ry

    emu = DC.EmuQueue(0.1)
    stamps = DC.stamps_200hz(T0 - 0.05, T0 + 0.15)
    for s in stamps:
        q = DC.euler_quat(0.0, 0.1 + pitch_rate * (s - T0), 0.3 + yaw_rate * (s - T0))
        assert emu.push(np.array([0, pitch_rate, yaw_rate], F), np.zeros(3, F), q, s)
    n = 2000
    xyz = DC.make_scan(n, rng, stamps, jitter=0.02)
    e = emu.deskew(xyz, T0)
    assert e["n_skipped"] == 0 and e["start_missing"] == 0 and 0 < e["half_index"] < n
    t = T0 + e["rel"].astype(np.float64)
    assert t.max() - t.min() > 0.09
    R0 = Rw(t[0])
    want = np.stack([R0.T @ (Rw(t[i]) @ xyz[i].astype(np.float64)) for i in range(n)])
    err = np.linalg.norm(e["out"].astype(np.float64) - want, axis=1)
    bound = 64 * 2.0 ** -24 * np.linalg.norm(xyz.astype(np.float64), axis=1)
    print("convention: max err / bound = %.3f, max err %.2e m, skew removed up to %.2f m" %
          ((err[1:] / bound[1:]).max(), err.max(), np.linalg.norm(xyz.astype(np.float64) - want, axis=1).max()))
    assert (err <= bound).all()
    assert np.linalg.norm(xyz.astype(np.float64) - want, axis=1).max() > 1.0      # the test would notice a de-skew that does nothing


def test_receive_removes_gravity_in_the_sensor_frame():
    """receiveImu's gravity removal (scanmatcher_component.cpp:505-511), the one copy every surface calls: an IMU at orientation R that
    accelerates by a (sensor frame) reports a + R^T (0, 0, 9.81); what reaches the queue must be a, to float rounding of |a| + 9.81 (a
    few ulps of 16: 1e-5), for orientations all round the roll and yaw circles and pitch short of the gimbal lock.  The sample's other
    fields pass through, the quaternion reordered to w x y z, and the same refusal applies as for a raw push."""
    rng = np.random.default_rng(9)
    emu = DC.EmuQueue(0.1)
    for k in range(400):
        roll, pitch, yaw = rng.uniform(-3.1, 3.1), rng.uniform(-1.5, 1.5), rng.uniform(-3.1, 3.1)
        w, x, y, z = (float(v) for v in DC.euler_quat(roll, pitch, yaw).astype(np.float64))
        cr, sr, cp, sp = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch)
        g_body = 9.81 * np.array([-sp, cp * sr, cp * cr])          # third row of Rz Ry Rx = R^T e_z
        a = rng.uniform(-3, 3, 3)
        scale = 1.0 + (k % 3)                                          # a quaternion that is not normalised gives the same rotation
        ok, ang, acc, quat = emu.receive(np.array([x, y, z, w]) * scale, (0.1, -0.2, 0.3), a + g_body, T0 + 0.005 * k)
        assert ok
        assert np.abs(acc.astype(np.float64) - a).max() <= 1e-5, (k, roll, pitch, yaw, acc, a)
        assert np.array_equal(ang, np.array([0.1, -0.2, 0.3], F))
        assert np.array_equal(quat, (np.array([w, x, y, z]) * scale).astype(F))
    assert not emu.receive((0, 0, 0, 1), (0, 0, 0), (0, 0, 9.81), T0 - 1.0)[0] and emu.info()["count"] == 400


def test_header_syntax_through_the_mock_adapters():
    """(d) the de-skew members of the C++ surface compile (-fsyntax-only) against the mock PCL / pclomp headers the adapter tests use."""
    src = os.path.join(ROOT, "tests", "cpp", "deskew_syntax.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-Werror", "-I" + os.path.join(ROOT, "tests", "cpp", "mock"), src])
    # the block INTEGRATION.md shows is the block that was just compiled
    block = open(src).read().split("// [deskew-snippet begin]\n")[1].split("// [deskew-snippet end]")[0].rstrip("\n")
    assert block in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name in ("lsr_imu_reset", "lsr_imu_push", "lsr_imu_receive", "lsr_imu_info", "lsr_deskew_pc2", "lsr_deskew_trace"):
        assert name + "(" in hdr

"""IMU de-skew on the device (csrc/deskew.hip through lsr_deskew_pc2) against the sequential restatement tests/deskew_numpy.py.

Discrete results — half index, ring slot per point, skip mask, skip count, start_missing, the new last_iter — must be EXACT.  The
device's atan2f may differ from the C library's by a few ulps, so the generators keep every azimuth 2e-3 rad from the branch
thresholds and every point time 2e-6 s from every stamp and stamp +- scan_period; each test asserts 1e-3 rad / 1e-6 s on the numpy side
and compares every point.  Coordinates: |out - ref64| <= 64 * 2^-24 * (|p| + |shift_c - shift_s| + |velo_s| * scan_period) per point,
ref64 = the same formulas in f64 from the same f32 table, the device's own rel_time and the (exact) table entries: the rounding of
about 30 f32 operations plus sinf / cosf.  A point whose input is not finite must come out not finite.  Skipped points, point 0 and
every byte outside x / y / z are bit-identical to the input."""
import ctypes as C

import numpy as np
import pytest

import deskew_cases as DC
import deskew_numpy as DN

pytestmark = pytest.mark.gpu
F = np.float32
T0 = DC.T0
WG = 256                      # DESKEW_WG: points per workgroup = fan-in of the prefix maximum
N_FULL = 146_000              # the frontend's raw scan


@pytest.fixture(scope="module")
def reg():
    from lidarslam_ros2_amd import NormalDistributionsTransform

    return NormalDistributionsTransform(device=0)


def _push(reg, ring, samples):
    fp = C.POINTER(C.c_float)
    for ang, acc, quat, stamp in samples:
        a, b, c = (np.ascontiguousarray(v, F) for v in (ang, acc, quat))
        ok = reg._lib.lsr_imu_push(reg._h, a.ctypes.data_as(fp), b.ctypes.data_as(fp), c.ctypes.data_as(fp), float(stamp)) == 0
        assert ok == ring.push(ang, acc, quat, stamp)


def _fresh(reg, samples, period=0.1):
    reg.imuReset(period)
    ring = DN.ImuRing(period)
    _push(reg, ring, samples)
    i = reg.imuInfo()
    assert (i["count"], i["last"], i["last_iter"]) == (ring.count, ring.last, ring.last_iter)
    return ring


def _payload(xyz, step, rng):
    """records of `step` bytes: x@0 y@4 z@8, every other byte random (step 32: an intensity at 16 among them)"""
    n = xyz.shape[0]
    rec = rng.integers(0, 256, (n, step), dtype=np.uint8)
    rec[:, :12] = np.ascontiguousarray(xyz, F).view(np.uint8).reshape(n, 12)
    return rec


def _run(reg, payload, n, step, scan_time, path):
    offs = (0, 4, 8, 16 if step == 32 else None)
    if path.startswith("device"):
        import torch

        d = torch.from_numpy(payload.copy()).cuda()
        out, info = reg.deskewPointCloud2(d, n, step, offs, scan_time, out=d if path == "device_inplace" else None)
        if path == "device":
            assert np.array_equal(d.cpu().numpy(), payload)        # the input was not written
        return out.cpu().numpy(), info
    buf = payload.copy()
    out, info = reg.deskewPointCloud2(buf, n, step, offs, scan_time, out=buf if path == "host_inplace" else None)
    if path == "host":
        assert np.array_equal(buf, payload)
    return out, info


def _check(reg, ring, xyz, scan_time, step=32, path="device", seed=0, expect=None):
    n = xyz.shape[0]
    rng = np.random.default_rng(seed)
    payload = _payload(xyz, step, rng)
    base = ring.last_iter
    m, st, fl = ring.table()
    r = DN.deskew(ring, xyz, scan_time, coords=False)
    out, info = _run(reg, payload, n, step, scan_time, path)
    tr = reg.deskewTrace()
    assert out.shape == payload.shape
    assert np.array_equal(out[:, 12:], payload[:, 12:])                       # non-xyz bytes
    oxyz = np.ascontiguousarray(out[:, :12]).view(F).reshape(n, 3)
    if not r["ran"]:
        assert np.array_equal(out, payload) and (info["n_skipped"], info["start_missing"], info["half_index"]) == (0, 0, -1)
        assert info["cursor"] == ring.last_iter and (tr["slot"] == -1).all()
        return r, info
    # the margins that make the discrete comparison meaningful, on the numpy side
    am = DC.angle_margin(r["ori"], r["start"], r["end"], r["half_index"])
    tm = DC.time_margin(r["t"], st, ring.scan_period)
    print("n=%d step=%d %s: angle margin %.2e rad, time margin %.2e s, skipped %d, H %d, cursor %d" %
          (n, step, path, am.min(), tm.min(), r["n_skipped"], r["half_index"], r["last_iter"]))
    assert am.min() >= 1e-3 and tm.min() >= 1e-6
    # discrete results: exact, every point
    assert info["half_index"] == r["half_index"]
    assert np.array_equal(tr["slot"], r["slot"])
    assert np.array_equal(tr["skipped"], r["skipped"])
    assert (info["n_skipped"], info["start_missing"], info["cursor"]) == (r["n_skipped"], r["start_missing"], r["last_iter"])
    assert reg.imuInfo()["last_iter"] == ring.last_iter
    # rel_time: 16 ulps of the largest angle (|ori_h| < 16 rad: ulp 2^-20) through / diff * scan_period
    fin = np.isfinite(r["rel"])
    tol = 16 * 2.0 ** -20 / abs(float(r["end"] - r["start"])) * ring.scan_period
    assert np.array_equal(np.isfinite(tr["rel_time"]), fin)
    assert np.abs(tr["rel_time"][fin].astype(np.float64) - r["rel"][fin].astype(np.float64)).max() <= tol
    # coordinates
    entry = (r["slot"].astype(np.int64) - base) % 200
    ref, dshift, vs = DN.ref64(xyz, tr["rel_time"], entry, r["skipped"], st, fl, scan_time, r["start_missing"])
    same = r["skipped"].astype(bool) | bool(r["start_missing"])
    same[0] = True
    assert np.array_equal(oxyz[same].view(np.uint32), xyz[same].view(np.uint32))
    moved = ~same
    if moved.any():
        finite = np.isfinite(ref).all(axis=1)
        assert not np.isfinite(oxyz[moved & ~finite]).all(axis=1).any()
        k = moved & finite
        err = np.linalg.norm(oxyz[k].astype(np.float64) - ref[k], axis=1)
        bound = 64 * 2.0 ** -24 * (np.linalg.norm(xyz[k].astype(np.float64), axis=1) + dshift[k] + vs[k] * ring.scan_period)
        print("   coordinates: %d moved, max err %.2e m, max err / bound %.3f, displacement up to %.3f m" %
              (int(k.sum()), err.max(), (err / bound).max(), np.linalg.norm(oxyz[k].astype(np.float64) - xyz[k], axis=1).max()))
        assert (err <= bound).all()
    if expect is not None:
        expect(r)
    return r, info


def _covering(rng, t0=T0):
    return DC.imu_samples(DC.stamps_200hz(t0 - 0.05, t0 + 0.15), rng, t0)


SIZES = [(1, 32, "device"), (2, 16, "host"), (63, 32, "host_inplace"), (64, 16, "device_inplace"), (65, 32, "device"),
         (WG - 1, 16, "device"), (WG, 32, "device_inplace"), (WG + 1, 16, "host"), (WG * WG + WG, 32, "device_inplace")]


@pytest.mark.parametrize("n,step,path", SIZES)
def test_sizes_with_a_200hz_imu_covering_the_scan(reg, n, step, path):
    """1, 2, around a wave, around a workgroup, and one workgroup above the square of the prefix maximum's fan-in (a workgroup folds
    more than 256 workgroup maxima: every level of the prefix maximum is crossed)."""
    rng = np.random.default_rng(1000 + n)
    samples = _covering(rng)
    ring = _fresh(reg, samples)
    xyz = DC.make_scan(n, rng, [s[3] for s in samples])
    r, _ = _check(reg, ring, xyz, T0, step, path, seed=n)
    assert r["n_skipped"] == 0 and r["start_missing"] == 0
    if n >= 63:
        assert 0 < r["half_index"] < n and len(np.unique(r["slot"])) >= 15


@pytest.mark.parametrize("step", [16, 32])
@pytest.mark.parametrize("path", ["host", "host_inplace", "device", "device_inplace"])
def test_paths_and_layouts(reg, step, path):
    rng = np.random.default_rng(77)
    samples = _covering(rng)
    ring = _fresh(reg, samples)
    xyz = DC.make_scan(3 * WG + 17, rng, [s[3] for s in samples])
    _check(reg, ring, xyz, T0, step, path, seed=5)


def test_full_scan_146k_points_once(reg):
    rng = np.random.default_rng(146)
    samples = _covering(rng)
    ring = _fresh(reg, samples)
    xyz = DC.make_scan(N_FULL, rng, [s[3] for s in samples])
    r, _ = _check(reg, ring, xyz, T0, 32, "device", seed=146)
    assert r["n_skipped"] == 0 and 0 < r["half_index"] < N_FULL


def test_wrapped_ring_with_last_in_the_middle(reg):
    rng = np.random.default_rng(21)
    stamps = T0 + 0.15 - 0.005 * np.arange(330)[::-1] + 0.00123
    samples = DC.imu_samples(stamps, rng)
    ring = _fresh(reg, samples)
    assert ring.count == 330 and ring.last == 129
    xyz = DC.make_scan(1500, rng, stamps)
    r, _ = _check(reg, ring, xyz, T0, 32, "device", seed=21)
    assert r["n_skipped"] == 0 and 90 < r["slot"].min() < r["slot"].max() < 129      # table entries 90.. of a ring that has wrapped


def test_ring_whose_newest_slot_is_zero_moves_nothing(reg):
    rng = np.random.default_rng(22)
    samples = DC.imu_samples([T0 - 0.001], rng)
    ring = _fresh(reg, samples)
    assert ring.last == 0
    xyz = DC.make_scan(700, rng, [])
    for path in ("device", "host", "device_inplace"):
        r, _ = _check(reg, ring, xyz, T0, 32, path, seed=22)
        assert not r["ran"]


def test_stale_imu_skips_every_point(reg):
    rng = np.random.default_rng(23)
    stamps = DC.stamps_200hz(T0 - 1.0, T0 - 0.5)
    ring = _fresh(reg, DC.imu_samples(stamps, rng))
    xyz = DC.make_scan(1000, rng, stamps)
    r, info = _check(reg, ring, xyz, T0, 16, "device", seed=23)
    assert r["n_skipped"] == 1000 and info["start_missing"] == 1 and info["cursor"] == 0


def test_imu_that_ends_before_the_scan_does(reg):
    rng = np.random.default_rng(24)
    stamps = DC.stamps_200hz(T0 - 0.3, T0 - 0.05 - 0.00123)
    ring = _fresh(reg, DC.imu_samples(stamps, rng))
    xyz = DC.make_scan(1200, rng, stamps)
    r, _ = _check(reg, ring, xyz, T0, 32, "device_inplace", seed=24)
    sk = r["skipped"].astype(bool)
    assert r["start_missing"] == 0 and 300 < sk.sum() < 900 and not sk[:200].any() and sk[-200:].all()


def test_first_stamp_after_the_scan_start_sets_start_missing(reg):
    rng = np.random.default_rng(25)
    stamps = DC.stamps_200hz(T0 + 0.15, T0 + 0.3)
    ring = _fresh(reg, DC.imu_samples(stamps, rng))
    xyz = DC.make_scan(1200, rng, stamps)
    r, info = _check(reg, ring, xyz, T0, 32, "device", seed=25)
    assert info["start_missing"] == 1 and 0 < r["n_skipped"] < 1200      # later points are not skipped, yet nothing moves


def test_gap_of_more_than_scan_period_inside_the_table(reg):
    """The gap table of tests/test_deskew_cpu.py: dense stamps up to scan_time + 0.02, then nothing until scan_time + 0.2.  The stamp
    behind the gap sits 0.4 ms later than there: the scan's last point always has rel_time = scan_period exactly, so a stamp at
    scan_time + 0.2 sharp would put it ON the skip threshold, inside the 1e-6 s margin this comparison keeps."""
    rng = np.random.default_rng(26)
    stamps = np.concatenate([DC.stamps_200hz(T0 - 0.06, T0 + 0.02 - 0.00123), [T0 + 0.2004, T0 + 0.2054]])
    ring = _fresh(reg, DC.imu_samples(stamps, rng))
    xyz = DC.make_scan(2 * WG + 100, rng, stamps, jitter=0.5)
    r, _ = _check(reg, ring, xyz, T0, 32, "device", seed=26)
    sk = r["skipped"].astype(bool)
    assert sk.any() and (~sk).any() and (~sk[np.nonzero(sk)[0][0]:]).any()      # moved points behind skipped ones


def test_nan_point_in_mid_scan(reg):
    rng = np.random.default_rng(27)
    samples = _covering(rng)
    ring = _fresh(reg, samples)
    n = 2 * WG + 40
    xyz = DC.make_scan(n, rng, [s[3] for s in samples], nan_at=WG + 3)
    r, _ = _check(reg, ring, xyz, T0, 32, "device", seed=27)
    assert not r["skipped"][WG + 3] and (r["slot"][WG + 3:] == ring.last).all()     # the pointer runs to the newest sample and stays


def test_two_scans_in_a_row_carry_the_cursor(reg):
    rng = np.random.default_rng(28)
    samples = DC.imu_samples(DC.stamps_200hz(T0 - 0.05, T0 + 0.1), rng)
    ring = _fresh(reg, samples)
    xyz = DC.make_scan(900, rng, [s[3] for s in samples])
    r1, i1 = _check(reg, ring, xyz, T0, 32, "device", seed=28)
    assert i1["cursor"] > 10
    more = DC.imu_samples(DC.stamps_200hz(T0 + 0.1 + 0.005, T0 + 0.25), rng)
    _push(reg, ring, more)
    stamps = [s[3] for s in samples + more]
    xyz2 = DC.make_scan(1100, rng, stamps, scan_time=T0 + 0.1)
    r2, i2 = _check(reg, ring, xyz2, T0 + 0.1, 16, "host", seed=29)
    assert r2["slot"].min() >= i1["cursor"] and i2["cursor"] > i1["cursor"] and r2["n_skipped"] == 0


def test_arguments_are_validated_before_any_device_use(reg):
    from lidarslam_ros2_amd import _capi

    lay = _capi.Pc2Layout(10, 0, 4, 8, -1)
    buf = np.zeros(64, np.uint8)
    L = reg._lib
    assert L.lsr_deskew_pc2(reg._h, C.c_void_p(buf.ctypes.data), 2, C.byref(lay), 0.0, 0, C.c_void_p(buf.ctypes.data), None) == -1
    lay = _capi.Pc2Layout(16, 0, 4, 8, -1)
    assert L.lsr_deskew_pc2(reg._h, None, 2, C.byref(lay), 0.0, 0, C.c_void_p(buf.ctypes.data), None) == -1
    assert L.lsr_deskew_pc2(None, C.c_void_p(buf.ctypes.data), 2, C.byref(lay), 0.0, 0, C.c_void_p(buf.ctypes.data), None) == -1
    assert L.lsr_imu_push(reg._h, None, None, None, 0.0) == -1 and L.lsr_imu_reset(reg._h, 0.0) == -1
    assert L.lsr_imu_receive(reg._h, None, None, None, 0.0) == -1
    # data / out_data: equal or disjoint; ranges that overlap otherwise are refused (2 records of 16 bytes, 16 bytes apart)
    assert L.lsr_deskew_pc2(reg._h, C.c_void_p(buf.ctypes.data), 2, C.byref(lay), 0.0, 0, C.c_void_p(buf.ctypes.data + 16), None) == -1
    assert L.lsr_deskew_pc2(reg._h, C.c_void_p(buf.ctypes.data + 16), 2, C.byref(lay), 0.0, 0, C.c_void_p(buf.ctypes.data), None) == -1
    reg.imuReset(0.1)
    assert L.lsr_deskew_pc2(reg._h, C.c_void_p(buf.ctypes.data), 2, C.byref(lay), 0.0, 0, C.c_void_p(buf.ctypes.data + 32), None) == 0
    reg.imuReset(0.1)
    assert reg.receiveImu((0, 0, 0, 1), (0, 0, 0), (0, 0, 9.81), 5.0) and not reg.receiveImu((0, 0, 0, 1), (0, 0, 0), (0, 0, 9.81), 4.0)
    assert reg.imuInfo() == dict(count=1, last=0, last_iter=0)


# ---- the frontend ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_drive():
    from lidarslam_ros2_amd import synth

    sensor = synth.Sensor(16, -20.0, 12.0, 600)
    base = synth.make_case(sensor=sensor, n_keyframes=3, vg_map=0.2, vg_input=0.4, n_source=2000, name="small", keep_parts=True)
    world = synth.make_world()
    rng = np.random.default_rng(4)
    xs = [1.5 * 2 + 0.5 * (1 + j) for j in range(6)]
    scans = [synth.raycast(world, sensor, synth.trajectory_pose(x), rng) for x in xs]
    return dict(frames=base.frames, frame_poses=base.frame_poses, scans=scans, guess0=np.asarray(synth.trajectory_pose(3.0), np.float64))


def _ndt():
    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform

    r = NormalDistributionsTransform(device=0)
    r.setResolution(5.0); r.setTransformationEpsilon(0.01); r.setMaximumIterations(35); r.setNeighborhoodSearchMethod(DIRECT7)
    return r


def _imu_msgs(j):
    """sensor_msgs/Imu fields for scan j (scan_time T0 + 0.1 j): a gentle turn, 200 Hz, gravity in the acceleration"""
    import math

    out = []
    for s in DC.stamps_200hz(T0 + 0.1 * j - (0.05 if j == 0 else 0.0) + (0.005 if j else 0.0), T0 + 0.1 * (j + 1)):
        yaw, pitch = 0.15 * (s - T0), 0.05 * math.sin(3 * (s - T0))
        w, x, y, z = (float(v) for v in DC.euler_quat(0.0, pitch, yaw))
        out.append(((x, y, z, w), (0.0, 0.15 * math.cos(3 * (s - T0)), 0.15), (0.3 - 9.81 * math.sin(pitch), 0.0, 9.81 * math.cos(pitch)), float(s)))
    return out


def _drive(small_drive, use_imu, pre_deskew=None, feed_imu=True):
    import torch

    from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload

    reg = _ndt()
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    fr = FrontendReplay(reg, FrontendParams(vg_size_for_input=0.4, vg_size_for_map=0.2, num_targeted_cloud=3, use_imu=use_imu), to_device=to_dev,
                        mapper=_ndt())
    fr.initialise(small_drive["frames"], small_drive["frame_poses"], small_drive["guess0"])
    if pre_deskew is not None:
        pre_deskew.imuReset(0.1)
    out, moved = FrontendResult(), 0.0
    for j, scan in enumerate(small_drive["scans"]):
        payload = torch.from_numpy(as_pc2_payload(scan)).cuda()
        n = int(scan.shape[0])
        for msg in _imu_msgs(j):
            if feed_imu:
                assert fr.receive_imu(*msg) == use_imu
            if pre_deskew is not None:
                assert pre_deskew.receiveImu(*msg)
        if pre_deskew is not None:
            raw = payload
            payload, info = pre_deskew.deskewPointCloud2(payload, n, 32, (0, 4, 8, 16), T0 + 0.1 * j)
            assert info["start_missing"] == 0 and info["n_skipped"] < n // 2
            moved = max(moved, float((payload.view(torch.float32) - raw.view(torch.float32)).abs().max()))
        fr.receive_cloud(payload, n, out, scan_time=T0 + 0.1 * j)
    fr.finish(out)
    return out, reg, moved


def test_frontend_with_use_imu_equals_a_frontend_fed_with_deskewed_payloads(small_drive):
    a, reg_a, _ = _drive(small_drive, use_imu=True)
    b, reg_b, moved = _drive(small_drive, use_imu=False, pre_deskew=_ndt(), feed_imu=False)
    assert moved > 0.02                                              # the de-skew did move the scans
    assert len(a.poses) == 6 and len(a.update_at) >= 1 and a.update_at == b.update_at
    assert a.points_kept == b.points_kept and a.iterations == b.iterations
    assert all(np.array_equal(p, q) for p, q in zip(a.poses, b.poses))
    assert reg_a.imuInfo()["count"] > 100 and reg_b.imuInfo()["count"] == 0
    # and it differs from the drive that ignores the IMU: the flag is not a no-op
    c, reg_c, _ = _drive(small_drive, use_imu=False)
    assert not all(np.array_equal(p, q) for p, q in zip(a.poses, c.poses))


def test_frontend_without_use_imu_ignores_the_imu(small_drive):
    """use_imu = False: IMU messages are dropped (scanmatcher_component.cpp:503), no de-skew entry is called, and the replay is the
    one an object that never heard of an IMU gives, bit for bit."""
    a, reg_a, _ = _drive(small_drive, use_imu=False, feed_imu=True)
    b, reg_b, _ = _drive(small_drive, use_imu=False, feed_imu=False)
    assert reg_a.imuInfo()["count"] == 0 and reg_a.deskewTrace()["rel_time"].size == 0
    assert a.points_kept == b.points_kept and a.iterations == b.iterations and a.update_at == b.update_at
    assert all(np.array_equal(p, q) for p, q in zip(a.poses, b.poses))

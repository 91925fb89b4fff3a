"""Localising in a saved map on the device (lsr_crop_map, lsr_set_input_target_window, lidarslam_ros2_amd.localization; csrc/map_window.hip)
against the numpy restatement tests/map_window_numpy.py, and the window target against the whole map as target.  Every comparison is
np.array_equal — on the raw bytes of records, on leaves, on final transformations: there is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import map_window_numpy as mwn
from lidarslam_ros2_amd import (DIRECT1, DIRECT7, GeneralizedIterativeClosestPoint, Localizer, LocalizerParams, MapArray, MapWindow,
                                NormalDistributionsTransform, _capi, mapWindowAround, synth)
from lidarslam_ros2_amd._capi import RegistrationError
from lidarslam_ros2_amd.frontend import as_pc2_payload

pytestmark = pytest.mark.gpu

XYZI = (32, (0, 4, 8, 16))
L16 = (16, (0, 4, 8, None))       # packed xyzw, no intensity
L48 = (48, (8, 12, 16, 4))        # fields in the middle of a longer record, intensity first
ERR_INVALID_ARGUMENT = -1


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(device=0)


def _records(rng, n, layout, extent=60.0):
    """n records of `layout`: every word a finite float in +-extent, padding words included (the output must not carry them)."""
    return rng.uniform(-extent, extent, (n, layout[0] // 4)).astype(np.float32)


def _xyzi(xyz, rng=None):
    rec = np.zeros((xyz.shape[0], 8), np.float32)
    rec[:, :3] = xyz
    rec[:, 3] = 7.0                                    # a padding word that must come out zero
    rec[:, 4] = np.arange(xyz.shape[0], dtype=np.float32) if rng is None else rng.uniform(0, 255, xyz.shape[0])
    return rec


# ---- 1. the cut, against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [XYZI, L16, L48], ids=["xyzi", "packed16", "wide48"])
def test_cut_equals_the_restatement(reg, layout):
    """5 000 records in +-60 m at leaf 0.5, a window of about +-20 cells off-centre, 1 % of the records with a NaN or an inf coordinate:
    host and device input, the same and another output layout, count only, and a capacity one below the count."""
    rng = np.random.default_rng(401)
    rec = _records(rng, 5000, layout)
    step, offs = layout
    bad = rng.choice(5000, 50, replace=False)
    for k, i in enumerate(bad):
        rec[i, offs[k % 3] // 4] = [np.nan, np.inf, -np.inf][(k // 3) % 3]
    w = MapWindow(0.5, (-5, -31, -22), (36, 10, 19))
    want, mask = mwn.crop(rec, w, layout, layout, return_mask=True)
    assert 10 < want.shape[0] < 2000 and not mask[bad].any()   # (42^3 of 240^3 cells: some twenty records)
    got_host = reg.cropMap(rec, w, layout, layout)
    assert isinstance(got_host, np.ndarray) and got_host.shape == want.shape and np.array_equal(got_host, want)
    got_dev = reg.cropMap(_cuda(rec), w, layout, layout)
    assert got_dev.is_cuda and np.array_equal(_host(got_dev), want)
    for other in (XYZI, L16, L48):
        want_o = mwn.crop(rec, w, layout, other)
        assert np.array_equal(_host(reg.cropMap(_cuda(rec), w, layout, other)), want_o)
        assert np.array_equal(reg.cropMap(rec, w, layout, other), want_o)
    assert reg.countMapWindow(rec, w, layout) == want.shape[0] == reg.countMapWindow(_cuda(rec), w, layout)
    # a caller's buffer: a capacity one below the count is refused untouched, the exact capacity is filled, identically twice
    small = np.full((want.shape[0] - 1, step), 0xCD, np.uint8)
    with pytest.raises(RegistrationError) as e:
        reg.cropMap(rec, w, layout, layout, out=small)
    assert e.value.status == ERR_INVALID_ARGUMENT and bool((small == 0xCD).all())
    exact = np.full((want.shape[0], step), 0xCD, np.uint8)
    assert np.array_equal(reg.cropMap(rec, w, layout, layout, out=exact), want)
    assert np.array_equal(reg.cropMap(rec, w, layout, layout), reg.cropMap(rec, w, layout, layout))


def test_wide_form_and_general_form_give_the_same_bytes(reg):
    """{32; 0,4,8,16} records on a 16-byte boundary take the wide form; the same records 4 bytes further on take the general one."""
    import torch

    rng = np.random.default_rng(402)
    rec = _records(rng, 3000, XYZI)
    w = MapWindow(0.5, (-40, -40, -40), (39, 39, 39))
    want = mwn.crop(rec, w, XYZI, XYZI)
    buf = torch.zeros(3000 * 32 + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for shift in (0, 4):
        view = buf[shift: shift + 3000 * 32]
        view.copy_(_cuda(rec.view(np.uint8).reshape(-1)))
        out = torch.full((want.shape[0] * 32 + 16,), 0xCD, dtype=torch.uint8, device="cuda")
        for oshift in (0, 4):
            o = out[oshift: oshift + want.shape[0] * 32].view(-1, 32)
            assert np.array_equal(_host(reg.cropMap(view, w, XYZI, XYZI, out=o)), want)


# ---- 2. seams ---------------------------------------------------------------------------------------------------------------------
def _inside_outside(keep):
    """Records whose x is 0.25 (cell 0 at leaf 0.5: kept by the window below) where keep is set and 100.25 elsewhere."""
    xyz = np.zeros((keep.shape[0], 3), np.float32)
    xyz[:, 0] = np.where(keep, 0.25, 100.25)
    xyz[:, 1] = 0.25
    xyz[:, 2] = 0.25
    return _xyzi(xyz)


SEAM_WINDOW = MapWindow(0.5, (0, 0, 0), (0, 0, 0))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 + 17])
def test_workgroup_seams(reg, n):
    """All kept, none kept, every other one, a whole workgroup outside between two inside, one workgroup fully inside: the intensity
    carries the input index, so the order is checked with the bytes."""
    i = np.arange(n)
    patterns = [np.ones(n, bool), np.zeros(n, bool), i % 2 == 0, (i < 256) | (i >= 512), (i >= 256) & (i < 512)]
    for keep in patterns:
        rec = _inside_outside(keep)
        want = mwn.crop(rec, SEAM_WINDOW, XYZI, XYZI)
        assert want.shape[0] == int(keep.sum())
        for src in (rec, _cuda(rec)):
            got = _host(reg.cropMap(src, SEAM_WINDOW, XYZI, XYZI))
            assert got.shape == want.shape and np.array_equal(got, want)
        assert np.array_equal(reg.cropMap(rec, SEAM_WINDOW, XYZI, L16), mwn.crop(rec, SEAM_WINDOW, XYZI, L16))


def test_more_workgroup_counts_than_the_scan_is_wide(reg):
    """300 001 records, every third kept: 1 172 workgroup counts for a scan of 1 024 threads, so every thread walks two."""
    n = 300001
    rec = _inside_outside(np.arange(n) % 3 == 0)
    want = mwn.crop(rec, SEAM_WINDOW, XYZI, XYZI)
    assert want.shape[0] == 100001
    assert np.array_equal(_host(reg.cropMap(_cuda(rec), SEAM_WINDOW, XYZI, XYZI)), want)
    assert np.array_equal(_host(reg.cropMap(_cuda(rec[:, :4].copy()), SEAM_WINDOW, L16, L48)), mwn.crop(rec[:, :4].copy(), SEAM_WINDOW, L16, L48))


# ---- 3. borders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [np.float32(0.1), 0.5, 2.0])
def test_cell_borders(reg, leaf):
    """Points exactly at k * leaf and one float either side, k = -40 .. 40, on each axis in turn; windows of one cell (lo == hi) and
    of a few."""
    leaf = float(np.float32(leaf))
    k = np.arange(-40, 41)
    edge = (k.astype(np.float32) * np.float32(leaf)).astype(np.float32)
    vals = np.concatenate([edge, np.nextafter(edge, np.float32(-np.inf)), np.nextafter(edge, np.float32(np.inf))]).astype(np.float32)
    mid = np.float32(0.5) * np.float32(leaf)
    xyz = np.concatenate([np.column_stack([vals if a == b else np.full(vals.shape, mid, np.float32) for b in range(3)]) for a in range(3)])
    rec = _xyzi(xyz.astype(np.float32))
    dev = _cuda(rec)
    windows = [MapWindow(leaf, (c, 0, 0), (c, 0, 0)) for c in (-40, -1, 0, 1, 7, 39)]
    windows += [MapWindow(leaf, (0, c, 0), (0, c, 0)) for c in (-3, 0, 12)] + [MapWindow(leaf, (0, 0, c), (0, 0, c)) for c in (-17, 0, 40)]
    windows += [MapWindow(leaf, (-3, -3, -3), (2, 2, 2)), MapWindow(leaf, (-41, 0, 0), (-40, 0, 0)), MapWindow(leaf, (-40, -40, -40), (40, 40, 40))]
    seen = 0
    for w in windows:
        want = mwn.crop(rec, w, XYZI, XYZI)
        seen += want.shape[0]
        assert np.array_equal(_host(reg.cropMap(dev, w, XYZI, XYZI)), want), w
    assert seen > 300


# ---- 4. contract ------------------------------------------------------------------------------------------------------------------
def _call(reg, rec, window, out, capacity, n_out, lay_in=(32, 0, 4, 8, 16), lay_out=(32, 0, 4, 8, 16), data=None):
    li, lo = _capi.Pc2Layout(*lay_in), _capi.Pc2Layout(*lay_out)
    w = None if window is None else C.byref(_capi.MapWindow(window[0], (C.c_int32 * 3)(*window[1]), (C.c_int32 * 3)(*window[2])))
    return reg._lib.lsr_crop_map(reg._h, C.c_void_p(rec.ctypes.data if data is None else data), rec.shape[0], C.byref(li), 0, w,
                                 None if out is None else C.c_void_p(out.ctypes.data), capacity, C.byref(lo), 0,
                                 None if n_out is None else C.byref(n_out))


def test_contract(reg):
    rng = np.random.default_rng(407)
    rec = _records(rng, 500, XYZI)
    target = _records(rng, 800, XYZI)[:, :3].copy()
    reg.setInputTarget(target)
    T_before = reg.getFinalTransformation().copy()
    good = (0.5, (-30, -30, -30), (29, 29, 29))
    n_out = C.c_size_t(777)
    out = np.full((500, 32), 0xCD, np.uint8)
    bad_windows = [(0.0, good[1], good[2]), (-0.5, good[1], good[2]), (float("nan"), good[1], good[2]), (0.5, (1, 0, 0), (0, 0, 0)),
                   (0.5, (0, 0, 3), (0, 0, 2)), (0.5, (-(1 << 24), 0, 0), (0, 0, 0)), (0.5, (0, 0, 0), (0, 1 << 24, 0)),
                   (0.5, (-(1 << 31), 0, 0), (0, 0, 0)), None]
    for w in bad_windows:
        assert _call(reg, rec, w, out, 500, n_out) == ERR_INVALID_ARGUMENT, w
    assert _call(reg, rec, good, out, 500, None) == ERR_INVALID_ARGUMENT
    assert _call(reg, rec, good, out, 500, n_out, lay_in=(30, 0, 4, 8, 16)) == ERR_INVALID_ARGUMENT
    assert _call(reg, rec, good, out, 500, n_out, lay_out=(32, 0, 0, 8, 16)) == ERR_INVALID_ARGUMENT       # output fields overlap
    assert _call(reg, rec, good, out, 500, n_out, data=rec.ctypes.data + 2) == ERR_INVALID_ARGUMENT        # not 4-byte aligned
    assert _call(reg, rec, good, out, 500, n_out, data=0) == ERR_INVALID_ARGUMENT                          # null with records
    assert reg._lib.lsr_crop_map(None, None, 0, None, 0, None, None, 0, None, 0, None) == ERR_INVALID_ARGUMENT
    # an output range that overlaps the input
    inplace = rec.view(np.uint8).reshape(-1, 32)
    before = inplace.copy()
    assert _call(reg, rec, good, inplace, 500, n_out) == ERR_INVALID_ARGUMENT and b"overlaps" in reg._lib.lsr_last_error()
    assert _call(reg, rec, good, inplace[1:], 499, n_out) == ERR_INVALID_ARGUMENT
    assert np.array_equal(inplace, before)
    assert n_out.value == 777 and bool((out == 0xCD).all())
    # out_data = NULL: the count; a capacity one short: the count, and the buffer untouched
    want = mwn.crop(rec, good, XYZI, XYZI)
    assert 0 < want.shape[0] < 500
    assert _call(reg, rec, good, None, 0, n_out) == 0 and n_out.value == want.shape[0]
    n_out = C.c_size_t(777)
    assert _call(reg, rec, good, out, want.shape[0] - 1, n_out) == ERR_INVALID_ARGUMENT
    assert n_out.value == want.shape[0] and bool((out == 0xCD).all())
    assert _call(reg, rec, good, out, want.shape[0], n_out) == 0
    assert np.array_equal(out[: want.shape[0]], want) and bool((out[want.shape[0]:] == 0xCD).all())
    # nothing kept, and no records: LSR_OK with a count of zero
    out[:] = 0xCD
    assert _call(reg, rec, (0.5, (500, 500, 500), (501, 501, 501)), out, 500, n_out) == 0 and n_out.value == 0
    n_out = C.c_size_t(777)
    assert _call(reg, rec[:0], good, out, 500, n_out) == 0 and n_out.value == 0 and bool((out == 0xCD).all())
    # what the object otherwise answers is unchanged
    assert np.array_equal(reg.getFinalTransformation(), T_before)
    reg.setInputSource(target[:100].copy())
    assert reg.getFitnessScore() < 1e-6                  # the target is still those 800 points
    # the window target: a window that keeps nothing is refused and the previous target stays
    n_kept = C.c_size_t(777)
    li = _capi.Pc2Layout(32, 0, 4, 8, 16)
    far = _capi.MapWindow(0.5, (C.c_int32 * 3)(500, 500, 500), (C.c_int32 * 3)(501, 501, 501))
    assert reg._lib.lsr_set_input_target_window(reg._h, C.c_void_p(rec.ctypes.data), 500, C.byref(li), 0, C.byref(far),
                                                C.byref(n_kept)) == ERR_INVALID_ARGUMENT and n_kept.value == 0
    assert reg._lib.lsr_set_input_target_window(reg._h, C.c_void_p(rec.ctypes.data), 500, C.byref(li), 0, None, C.byref(n_kept)) == ERR_INVALID_ARGUMENT
    assert reg._lib.lsr_set_input_target_window(reg._h, C.c_void_p(rec.ctypes.data), 500, C.byref(li), 0, C.byref(far), None) == ERR_INVALID_ARGUMENT
    assert reg.getFitnessScore() < 1e-6


def test_profile_key(reg):
    rng = np.random.default_rng(408)
    rec = _cuda(_records(rng, 4000, XYZI))
    w = MapWindow(0.5, (-30, -30, -30), (29, 29, 29))
    assert reg.mapWindowMs() >= 0.0
    reg._seti(_capi.PROFILE, 1, "profile")
    try:
        reg.cropMap(rec, w)
        assert 0.0 < reg.mapWindowMs() < 1000.0
    finally:
        reg._seti(_capi.PROFILE, 0, "profile")
    reg.cropMap(rec, w)
    assert reg.mapWindowMs() == 0.0


# ---- 5. offsets past 2 GiB --------------------------------------------------------------------------------------------------------
def test_records_behind_two_gib(reg):
    """2^26 + 4096 records of 32 bytes: the byte offset of the last 4 096 passes 2^31; the records in front have a NaN x, the window
    lies over the tail.  The result is the restatement's of those 4 096 records alone."""
    import torch

    rng = np.random.default_rng(409)
    tail = _xyzi(rng.uniform(-30.0, 30.0, (4096, 3)).astype(np.float32), rng)
    n = (1 << 26) + 4096
    rec = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    rec[: 1 << 26, 0] = float("nan")
    rec[1 << 26:] = torch.from_numpy(tail).cuda()
    w = MapWindow(2.0, (-10, -10, -10), (9, 9, 9))
    want = mwn.crop(tail, w, XYZI, XYZI)
    got = reg.cropMap(rec, w)
    assert 500 < want.shape[0] < 4096 and np.array_equal(_host(got), want)


# ---- 6. the target ----------------------------------------------------------------------------------------------------------------
def _grid(r):
    return r.gridInfo(), r.gridDump()


def _same_grid(a, b):
    ia, da = a
    ib, db = b
    return (all(np.array_equal(ia[k], ib[k]) for k in ("min_b", "max_b")) and ia["n_leaves"] == ib["n_leaves"] and ia["n_valid"] == ib["n_valid"]
            and all(np.array_equal(da[k], db[k], equal_nan=True) for k in ("idx", "n", "mean", "icov")))


def test_window_target_equals_the_two_steps(reg):
    rng = np.random.default_rng(410)
    rec = _xyzi(rng.uniform(-40.0, 40.0, (20000, 3)).astype(np.float32) * np.float32([1, 1, 0.1]), rng)
    w = mapWindowAround((5.0, -3.0, 0.0), (15.0, 15.0, 6.0), 1.0)
    cut, mask = mwn.crop(rec, w, XYZI, XYZI, return_mask=True)
    assert 1000 < cut.shape[0] < 10000
    a, b = NormalDistributionsTransform(device=0), NormalDistributionsTransform(device=0)
    for r in (a, b):
        r.setResolution(1.0)
    assert a.setInputTargetWindow(_cuda(rec), w) == cut.shape[0]
    b.setInputTarget(rec[mask][:, :3].copy())
    assert _same_grid(_grid(a), _grid(b))
    assert a.setInputTargetWindow(rec, w) == cut.shape[0] and _same_grid(_grid(a), _grid(b))     # a host map, staged
    ga, gb = GeneralizedIterativeClosestPoint(device=0), GeneralizedIterativeClosestPoint(device=0)
    assert ga.setInputTargetWindow(_cuda(rec), w) == cut.shape[0]
    gb.setInputTarget(rec[mask][:, :3].copy())
    for g in (ga, gb):
        g.setInputSource(rec[mask][:100, :3].copy())       # (the inspection entry wants a source on the object)
        g.prepareTarget()
    assert np.array_equal(ga.covariances("target"), gb.covariances("target"))


# ---- 7. / 8. window == whole map ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """The small case's target plus 3 000 clutter points 200 - 400 m out, shuffled in with a fixed seed: PointXYZI records.  The
    window: the guess position +- (the largest source range + 3 m + 2 cells) at resolution 1.0.  Shared, never modified."""
    case = synth.small_case()
    rng = np.random.default_rng(411)
    ang, rad = rng.uniform(0, 2 * np.pi, 3000), rng.uniform(200.0, 400.0, 3000)
    clutter = np.column_stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-10.0, 10.0, 3000)]).astype(np.float32)
    xyz = np.concatenate([case.target, clutter])[rng.permutation(case.target.shape[0] + 3000)]
    reach = float(np.linalg.norm(case.source.astype(np.float64), axis=1).max()) + 3.0 + 2.0
    w = mapWindowAround(case.guess[:3, 3], (reach, reach, reach), 1.0)
    return case, _xyzi(xyz, rng), w


def _ndt(method):
    r = NormalDistributionsTransform(device=0)
    r.setResolution(1.0)
    r.setNeighborhoodSearchMethod(method)
    r.setMaximumIterations(30)
    r.setTransformationEpsilon(0.01)
    return r


def _leaves_by_cell(r):
    info, d = _grid(r)
    div = info["max_b"].astype(np.int64) - info["min_b"] + 1
    idx = d["idx"].astype(np.int64)
    cells = np.column_stack([idx % div[0], (idx // div[0]) % div[1], idx // (div[0] * div[1])]) + info["min_b"]
    return {tuple(c): (int(d["n"][j]), d["mean"][j].tobytes(), d["icov"][j].tobytes()) for j, c in enumerate(cells)}


def _align(r, case):
    r.setInputSource(case.source)
    r.align(case.guess)
    return r.getFinalTransformation(), r.getFinalNumIteration(), r.getFitnessScore()


@pytest.fixture(scope="module")
def window_arm(scene):
    """Final transformation, iterations and fitness of the window arm for DIRECT7 and DIRECT1."""
    case, rec, w = scene
    out = {}
    for method in (DIRECT7, DIRECT1):
        r = _ndt(method)
        r.setInputTargetWindow(_cuda(rec), w)
        out[method] = _align(r, case)
    return out


def test_window_leaves_are_the_whole_maps_leaves(scene):
    case, rec, w = scene
    whole, cut = _ndt(DIRECT7), _ndt(DIRECT7)
    whole.setInputTarget(rec[:, :3].copy())
    n = cut.setInputTargetWindow(_cuda(rec), w)
    assert case.target.shape[0] * 0.5 < n <= case.target.shape[0]          # the clutter is outside, the scene (mostly) inside
    lw, lc = _leaves_by_cell(whole), _leaves_by_cell(cut)
    inside = {c: v for c, v in lw.items() if all(w.lo[k] <= c[k] <= w.hi[k] for k in range(3))}
    assert len(inside) > 500 and len(lw) > len(inside)
    assert set(lc) == set(inside)                                          # the window grid has no other leaf
    assert all(lc[c] == inside[c] for c in inside)                         # npts, mean and icov, bit for bit


@pytest.mark.parametrize("method", [DIRECT7, DIRECT1], ids=["direct7", "direct1"])
def test_align_in_the_window_equals_align_in_the_whole_map(scene, window_arm, method):
    case, rec, w = scene
    whole = _ndt(method)
    whole.setInputTarget(rec[:, :3].copy())
    T, it, fit = _align(whole, case)
    Tw, itw, fitw = window_arm[method]
    assert it >= 2 and np.isfinite(T).all()
    assert np.array_equal(T, Tw) and it == itw and fit == fitw


def test_a_map_the_whole_target_refuses(scene, window_arm):
    """The same scene plus eight points at (+-3000, +-3000, +-300): 6000 x 6000 x 600 cells at resolution 1.0."""
    case, rec, w = scene
    corners = np.array([[sx * 3000.0, sy * 3000.0, sz * 300.0] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    big = np.concatenate([rec, _xyzi(corners)])
    whole = _ndt(DIRECT7)
    with pytest.raises(RegistrationError) as e:
        whole.setInputTarget(big[:, :3].copy())
        whole.setInputSource(case.source)
        whole.align(case.guess)
    assert e.value.status == _capi.ERR_INDEX_OVERFLOW
    cut = _ndt(DIRECT7)
    cut.setInputTargetWindow(_cuda(big), w)
    T, it, fit = _align(cut, case)
    Tw, itw, fitw = window_arm[DIRECT7]
    assert np.array_equal(T, Tw) and it == itw and fit == fitw


# ---- 9. / 10. a drive ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive():
    """30 scans of a 16-beam x 600-azimuth sensor, 0.5 m apart along trajectory_pose, in the sensor frame, with their true poses."""
    world, sensor = synth.make_world(), synth.Sensor(16, -20.0, 12.0, 600)
    poses = [synth.trajectory_pose(0.5 * i) for i in range(30)]
    scans = synth.raycast_many(world, sensor, poses, np.random.default_rng(412))
    return scans, poses


DRIVE_PARAMS = dict(scan_min_range=0.5, scan_max_range=60.0, vg_size_for_input=0.4, reach=(62.0, 62.0, 30.0))


def _keyframes(scans, poses, every):
    ma = MapArray()
    for i in range(0, len(scans), every):
        ma.append(synth.as_pointxyzi(scans[i]), poses[i], 0.5 * i)
    return ma


def _localise(localizer, scans, poses, first, which):
    """The scans `which` registered one after the other from the pose of scan `first`; the guess of every align is the previous
    estimate moved on by the odometry between the two scans (the caller's guess of receive_cloud), formed the same way in every arm."""
    localizer.set_initial_pose(poses[first].astype(np.float32))
    out, last = [], first
    for i in which:
        odom = np.linalg.inv(poses[last]) @ poses[i]
        guess = (localizer.pose.astype(np.float64) @ odom).astype(np.float32)
        out.append(localizer.receive_cloud(as_pc2_payload(scans[i]), scans[i].shape[0], guess).copy())
        assert not localizer.lost
        last = i
    return out


def test_drive_with_recuts_equals_the_whole_map(reg, drive):
    scans, poses = drive
    world_map, _ = _keyframes(scans, poses, 3).publish_map(reg, leaf=0.2)
    world_map = _cuda(_host(world_map))
    arms = []
    for window in (True, False):
        loc = Localizer(_ndt(DIRECT7), LocalizerParams(slack=(6.0, 6.0, 6.0), **DRIVE_PARAMS), window=window)
        loc.set_map(world_map)
        arms.append((loc, _localise(loc, scans, poses, 0, range(len(scans)))))
    (lw, pw), (lf, pf) = arms
    assert lw.n_recuts >= 2 and lf.n_recuts == 0 and 0 < lw.n_target < lf.n_target
    assert all(np.array_equal(a, b) for a, b in zip(pw, pf))
    assert np.abs(pw[-1][:3, 3] - poses[-1][:3, 3]).max() < 0.5            # and it is a localisation: the drive ends where it ended


def test_saved_map_round_trip(reg, drive, tmp_path):
    scans, poses = drive
    ma = _keyframes(scans[:9], poses[:9], 4)
    assert len(ma) == 3
    path = str(tmp_path / "map.pcd")
    ma.save_map(reg, path, data="binary_compressed", leaf=0.2)
    arms = []
    for from_file in (True, False):
        r = _ndt(DIRECT7)
        loc = Localizer(r, LocalizerParams(slack=(6.0, 6.0, 6.0), **DRIVE_PARAMS))
        if from_file:
            r.pcdReadCompressed(True)
            loc.load_map(path)
        else:
            loc.set_map(ma.publish_map(reg, leaf=0.2)[0])
        arms.append(_localise(loc, scans, poses, 1, range(1, 6)))
    assert all(np.array_equal(a, b) for a, b in zip(*arms)) and np.isfinite(arms[0][-1]).all()

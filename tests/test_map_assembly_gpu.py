"""The whole map from its submaps on the device (lsr_assemble_map): ScanMatcherComponent::publishMap
(scanmatcher_component.cpp:529-552) and the map half of doPoseAdjustment (graph_based_slam_component.cpp:321-368) against the numpy
restatement tests/map_numpy.py.  Every comparison is np.array_equal on the raw bytes of the records: there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import map_numpy
from map_numpy import XYZI
from lidarslam_ros2_amd import (GeneralizedIterativeClosestPoint, LoopClosureParams, MapArray, NormalDistributionsTransform, SubMap,
                                _capi, search_loop, synth)

pytestmark = pytest.mark.gpu

L16 = (16, (0, 4, 8, None))       # packed xyzw, no intensity
L48 = (48, (8, 12, 16, 4))        # fields in the middle of a longer record, intensity first
L20 = (20, (0, 4, 8, 12))         # packed x y z intensity + one spare word


def _cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)


def _records(rng, n, step):
    """n records of `step` bytes: every word a finite float of moderate size, padding words included (the output must not carry them)."""
    return rng.uniform(-60.0, 60.0, (n, step // 4)).astype(np.float32)


def _pose(rng):
    """A pose with rotations about all axes: (position, unit quaternion x y z w)."""
    q = rng.normal(size=4)
    return tuple(rng.uniform(-200.0, 200.0, 3)), tuple(q / np.linalg.norm(q))


def _submaps(rng, sizes, step=32):
    return [SubMap(_records(rng, n, step), *_pose(rng)) for n in sizes]


def _on_device(submaps, shift=0):
    """The same submaps with their clouds in HBM; shift: bytes by which every base pointer is moved off its 16-byte boundary."""
    import torch

    out = []
    for s in submaps:
        raw = torch.from_numpy(np.ascontiguousarray(s.cloud).reshape(-1).view(np.uint8))
        buf = torch.empty(raw.numel() + shift, dtype=torch.uint8, device="cuda")
        buf[shift:] = raw
        out.append(SubMap(buf[shift:], s.position, s.orientation, s.distance))
    return out


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(device=0)


SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025, 3000, 0]


@pytest.fixture(scope="module")
def edge_case():
    """Submaps around the slice length (1024 records) and the workgroup width (256), empty ones at both ends; shared, never modified."""
    sm = _submaps(np.random.default_rng(101), SIZES)
    return sm, map_numpy.assemble_map(sm)


def test_slice_and_table_edges(reg, edge_case):
    sm, (want, want_first) = edge_case
    rec, first = reg.assembleMap(_on_device(sm))
    assert rec.is_cuda and rec.shape == (sum(SIZES), 32)
    assert np.array_equal(first, want_first) and first.tolist() == np.concatenate([[0], np.cumsum(SIZES)]).tolist()
    assert np.array_equal(_host(rec), want)
    assert reg.mapAssemblyForm() == 1


def test_many_submaps(reg):
    """600 submaps of 1-40 records, some empty: the binary search runs over a table far longer than a wave."""
    rng = np.random.default_rng(102)
    sizes = rng.integers(1, 41, 600)
    sizes[rng.choice(600, 60, replace=False)] = 0
    sm = _submaps(rng, [int(v) for v in sizes])
    want, want_first = map_numpy.assemble_map(sm)
    rec, first = reg.assembleMap(_on_device(sm))
    assert np.array_equal(first, want_first) and np.array_equal(_host(rec), want)
    assert reg.mapAssemblyForm() == 1


@pytest.mark.parametrize("in_layout,shift", [(L16, 0), (L48, 0), (XYZI, 4)], ids=["in16", "in48", "xyzi_unaligned"])
def test_general_form_and_layouts(reg, edge_case, in_layout, shift):
    rng = np.random.default_rng(103)
    sm = edge_case[0] if in_layout == XYZI else _submaps(rng, [0, 1, 257, 1025, 700], in_layout[0])
    dev = _on_device(sm, shift)
    for out_layout in (XYZI, L20, L16):
        want, want_first = map_numpy.assemble_map(sm, None, in_layout, out_layout)
        rec, first = reg.assembleMap(dev, None, in_layout, out_layout)
        assert reg.mapAssemblyForm() == 2, (in_layout, out_layout)
        assert rec.shape == want.shape and np.array_equal(first, want_first)
        assert np.array_equal(_host(rec), want), (in_layout, out_layout)
        if in_layout == XYZI and out_layout == XYZI:
            # the same data through the wide form (aligned base pointers): the same bytes
            wide, _ = reg.assembleMap(_on_device(sm))
            assert reg.mapAssemblyForm() == 1 and np.array_equal(_host(wide), _host(rec))


def test_unaligned_output_takes_the_general_form(reg, edge_case):
    import torch

    sm, (want, _) = edge_case
    buf = torch.empty(want.size + 4, dtype=torch.uint8, device="cuda")
    rec, _ = reg.assembleMap(_on_device(sm), out=buf[4:])
    assert reg.mapAssemblyForm() == 2 and np.array_equal(_host(rec), want)


@pytest.mark.parametrize("big", [False, True], ids=["edges", "staged_in_pieces"])
def test_residency(reg, edge_case, big):
    """Host or device in, host or device out: identical bytes.  `big`: more records than one staged piece holds (64 MiB of 32-byte
    records), the boundary falling inside a submap."""
    import torch

    if big:
        sm = _submaps(np.random.default_rng(104), [5, (64 << 20) // 32 + 700, 300])
        want, want_first = map_numpy.assemble_map(sm)
    else:
        sm, (want, want_first) = edge_case
    dev = _on_device(sm)
    for src in (sm, dev):
        for out_dev in (False, True):
            out = torch.empty(want.size, dtype=torch.uint8, device="cuda") if out_dev else np.zeros(want.size, np.uint8)
            rec, first = reg.assembleMap(src, out=out)
            assert bool(getattr(rec, "is_cuda", False)) == out_dev and reg.mapAssemblyForm() == 1
            assert np.array_equal(first, want_first) and np.array_equal(_host(rec), want), (src is dev, out_dev)
    rec, _ = reg.assembleMap(sm)          # no buffer given: a numpy array for host submaps
    assert isinstance(rec, np.ndarray) and np.array_equal(rec, want)


def test_pose_sources(reg, edge_case):
    sm, (want, _) = edge_case
    rng = np.random.default_rng(105)
    dev = _on_device(sm)
    # the backend: the optimiser's fp64 estimates replace the stored poses
    poses = [map_numpy.pose_matrix(*_pose(rng)) for _ in sm]
    rec, _ = reg.assembleMap(dev, poses)
    assert np.array_equal(_host(rec), map_numpy.assemble_map(sm, poses)[0])
    # the frontend: each submap's own position / orientation, here quaternions that are NOT normalised (tf2::fromMsg does not either)
    odd = [SubMap(s.cloud, s.position, tuple(1.0007 * np.asarray(s.orientation)), s.distance) for s in sm]
    rec, _ = reg.assembleMap(_on_device(odd))
    got = _host(rec)
    assert np.array_equal(got, map_numpy.assemble_map(odd)[0]) and not np.array_equal(got, want)


def test_xyz_are_the_bits_of_set_input_target_frames(edge_case):
    """The same frames and poses through lsr_set_input_target_frames: every point of the assembled map finds itself in that target at
    distance zero, in order."""
    sm, (want, _) = edge_case
    g = GeneralizedIterativeClosestPoint(device=0)
    rec, _ = g.assembleMap(_on_device(sm))
    xyz = np.ascontiguousarray(_host(rec).view(np.float32).reshape(-1, 8)[:, :3])
    frames = [np.ascontiguousarray(s.cloud) for s in sm if s.cloud.shape[0]]
    poses = [map_numpy.pose_matrix(s.position, s.orientation) for s in sm if s.cloud.shape[0]]
    g.setInputTargetFrames(frames, poses)
    g.setInputSource(xyz)
    idx, d2 = g.nearestNeighbors()
    assert np.array_equal(d2, np.zeros_like(d2)) and np.array_equal(idx, np.arange(xyz.shape[0], dtype=np.int32))


def test_append(reg, edge_case):
    """The call keeps no state: submaps [0, k) and then [k, n) at out + first_record[k] give the map of one call over [0, n)."""
    import torch

    sm, (want, want_first) = edge_case
    dev = _on_device(sm)
    n = len(sm)
    poses = [map_numpy.pose_matrix(*_pose(np.random.default_rng(106 + i))) for i in range(n)]
    for k in (1, 4, n - 1):
        for P, full in ((None, want), (poses, map_numpy.assemble_map(sm, poses)[0])):
            buf = torch.full((want.size,), 0xAB, dtype=torch.uint8, device="cuda")
            _, first_a = reg.assembleMap(dev[:k], None if P is None else P[:k], out=buf)
            assert np.array_equal(first_a, want_first[: k + 1])
            _, first_b = reg.assembleMap(dev[k:], None if P is None else P[k:], out=buf[int(want_first[k]) * 32:])
            assert np.array_equal(first_b + want_first[k], want_first[k:])
            assert np.array_equal(_host(buf).reshape(-1, 32), full), k


def test_non_finite_input(reg):
    """NaN and infinite coordinates are moved and written like any others: the record count is exact and the bytes are numpy's.  The
    non-finite values are NaNs (which every operation hands on) and ONE infinity per point: an infinity minus an infinity would MAKE a
    NaN, whose sign IEEE 754 leaves to the implementation."""
    rng = np.random.default_rng(107)
    sm = _submaps(rng, [300, 1100])
    for s in sm:
        c = s.cloud
        c[3, 0] = np.nan; c[7, 1] = np.nan; c[11, 2] = np.nan; c[12, :3] = np.nan
        c[20, 0] = np.inf; c[21, 1] = -np.inf; c[22, 2] = np.inf
        c[30, 0] = np.nan; c[30, 1] = np.inf
        c[40, 4] = np.nan; c[41, 4] = -np.inf      # intensity: carried bit for bit
    want, want_first = map_numpy.assemble_map(sm)
    assert np.isnan(want.view(np.float32)).any() and np.isinf(want.view(np.float32)).any()
    for layouts in ((XYZI, XYZI), (XYZI, L20)):
        ref = want if layouts[1] == XYZI else map_numpy.assemble_map(sm, None, *layouts)[0]
        rec, first = reg.assembleMap(_on_device(sm), None, *layouts)
        assert rec.shape[0] == 1400 and np.array_equal(first, want_first)
        assert np.array_equal(_host(rec).view(np.uint8), ref.view(np.uint8))


def _raw(reg, arr, n, li, on_device, out_ptr, cap, lo, out_on_device):
    first = (C.c_size_t * 3)(77, 77, 77)
    n_out = C.c_size_t(99)
    st = reg._lib.lsr_assemble_map(reg._h, arr, n, C.byref(li) if li is not None else None, on_device, None, C.c_void_p(out_ptr), cap,
                                   C.byref(lo) if lo is not None else None, out_on_device, first, C.byref(n_out))
    return st, list(first), n_out.value


def test_errors_leave_the_outputs_and_the_handle_alone():
    import torch

    reg = NormalDistributionsTransform(device=0)
    rng = np.random.default_rng(108)
    clouds = [_cuda(_records(rng, n, 32)) for n in (10, 20)]
    arr = (_capi.SubMap * 2)()
    for a, c in zip(arr, clouds):
        a.position[:] = [1.0, 2.0, 3.0]
        a.orientation[:] = [0.0, 0.0, 0.0, 1.0]
        a.cloud, a.n_points = c.data_ptr(), c.shape[0]
    out = torch.full((40 * 32,), 0xAB, dtype=torch.uint8, device="cuda")
    good = _capi.Pc2Layout(32, 0, 4, 8, 16)
    untouched = ([77, 77, 77], 99)

    def refused(status, *args):
        st, first, n_out = _raw(reg, *args)
        assert st == status, (st, reg._lib.lsr_last_error())
        assert (first, n_out) == untouched and bool((out == 0xAB).all())

    refused(-1, arr, 2, good, 1, out.data_ptr(), 29, good, 1)                                    # capacity below the total
    refused(-1, arr, 2, good, 1, clouds[1].data_ptr() + 32, 40, good, 1)                         # the output range overlaps an input cloud
    refused(-1, arr, 2, good, 1, clouds[0].data_ptr() - 30 * 32 + 32, 40, good, 1)               # ... from below, by one record
    refused(-1, arr, 2, _capi.Pc2Layout(30, 0, 4, 8, 16), 1, out.data_ptr(), 40, good, 1)        # point_step not a multiple of 4
    refused(-1, arr, 2, good, 1, out.data_ptr(), 40, _capi.Pc2Layout(32, 0, 4, 8, 30), 1)        # a field that does not fit
    refused(-1, arr, 2, good, 1, out.data_ptr(), 40, _capi.Pc2Layout(32, 0, 4, 8, 8), 1)         # output fields overlap
    refused(-1, arr, 2, None, 1, out.data_ptr(), 40, good, 1)                                    # no layout
    refused(-1, arr, 0, good, 1, out.data_ptr(), 40, good, 1)                                    # no submaps
    arr[1].cloud = None
    refused(-1, arr, 2, good, 1, out.data_ptr(), 40, good, 1)                                    # points and no cloud
    arr[1].cloud = clouds[1].data_ptr()
    arr[1].n_points = 2**31                                                                       # refused before anything is read
    refused(-7, arr, 2, good, 1, out.data_ptr(), 2**32, good, 1)
    arr[1].n_points = 0
    arr[0].n_points = 0
    st, first, n_out = _raw(reg, arr, 2, good, 1, out.data_ptr(), 0, good, 1)                    # a total of zero is fine
    assert st == 0 and first == [0, 0, 0] and n_out == 0 and bool((out == 0xAB).all())
    assert reg.mapAssemblyForm() == 0
    # the handle still registers
    from lidarslam_ros2_amd import DIRECT7

    case = synth.small_case(n_source=4000, n_keyframes=3)
    reg.setResolution(3.0); reg.setTransformationEpsilon(0.01); reg.setNeighborhoodSearchMethod(DIRECT7)
    reg.setInputTarget(synth.as_pointxyzi(case.target)); reg.setInputSource(synth.as_pointxyzi(case.source))
    reg.align(case.guess)
    assert reg.hasConverged()


# ---- end to end: the frontend with its MapArray, then the backend's two uses of it -----------------------------------------------
N_SCANS = 25


@pytest.fixture(scope="module")
def drive():
    import multiprocessing as mp
    import os

    with mp.get_context("spawn").Pool(min(16, len(os.sched_getaffinity(0)))) as p:
        return synth.cfg_frontend_drive(N_SCANS, pool=p)


def _ndt():
    from lidarslam_ros2_amd import DIRECT7

    r = NormalDistributionsTransform(device=0)
    r.setResolution(5.0); r.setTransformationEpsilon(0.01); r.setMaximumIterations(35); r.setNeighborhoodSearchMethod(DIRECT7)
    return r


def _replay(reg, drive, **kw):
    import torch

    from lidarslam_ros2_amd.frontend import FrontendParams, FrontendReplay, FrontendResult, as_pc2_payload

    fr = FrontendReplay(reg, FrontendParams(), to_device=lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda(),
                        mapper=_ndt(), **kw)
    fr.initialise(drive["frames"], drive["frame_poses"], drive["guess0"])
    out = FrontendResult()
    for scan in drive["scans"]:
        host = as_pc2_payload(scan)
        fr.receive_cloud(torch.from_numpy(host).cuda(), int(scan.shape[0]), out, payload_host=host)
    fr.finish(out)
    return fr, out


def test_end_to_end_frontend_and_backend(drive):
    plain_fr, plain = _replay(_ndt(), drive)
    ma = MapArray()
    reg = _ndt()
    fr, out = _replay(reg, drive, map_array=ma, map_publish_every=2)
    # attaching the MapArray changes nothing the frontend computes
    assert plain_fr.map_array is None and plain.publish_seconds == []
    assert out.update_at == plain.update_at and out.iterations == plain.iterations and out.points_kept == plain.points_kept
    assert all(np.array_equal(a, b) for a, b in zip(out.poses, plain.poses))
    n_updates = len(out.update_at)
    # Scans come every 0.5 m and a keyframe is due 1.5 m after the last one, by the ESTIMATED pose, so some triggers fall a scan late:
    # 25 scans give at most eight updates.  The test needs four: two publishes, the first creating the resident map, the second
    # growing and extending it.
    assert 4 <= n_updates <= 8, out.update_at
    assert len(ma) == len(drive["frames"]) + n_updates and len(out.publish_seconds) == n_updates // 2
    assert all(s.cloud.is_cuda for s in ma.submaps)
    assert np.all(np.diff([s.distance for s in ma.submaps]) > 0)
    # the resident published map, brought up to date, is publish_map from scratch, is numpy
    host_sm = [SubMap(_host(s.cloud), s.position, s.orientation, s.distance) for s in ma.submaps]
    want, want_first = map_numpy.assemble_map(host_sm)
    rec, first = fr.published
    held = first.shape[0] - 1
    assert held == len(drive["frames"]) + 2 * (n_updates // 2) and rec.is_cuda
    assert np.array_equal(_host(rec), want[: want_first[held]])
    rec, first = ma.extend_published(reg)
    full, full_first = ma.publish_map(reg)
    assert np.array_equal(first, want_first) and np.array_equal(full_first, want_first)
    assert np.array_equal(_host(rec), want) and np.array_equal(_host(full), want)
    assert reg.mapAssemblyForm() == 1
    # the backend takes the same objects: the loop gate, then the map moved by the optimiser's poses (a fixed small transform stands in)
    edges = search_loop(reg, ma.submaps, LoopClosureParams(distance_loop_closure=5.0, range_of_searching_loop_closure=30.0))
    assert len(edges) == 1 and np.isfinite(edges[0].fitness_score)
    D = synth.pose_matrix(0.03, -0.02, 0.01, 0.002, 0.001, -0.0015)
    poses = [D @ map_numpy.pose_matrix(s.position, s.orientation) for s in host_sm]
    mod, mod_first = ma.modified_map(reg, poses)
    want_mod, _ = map_numpy.assemble_map(host_sm, poses)
    assert np.array_equal(mod_first, want_first) and np.array_equal(_host(mod), want_mod) and not np.array_equal(want_mod, want)

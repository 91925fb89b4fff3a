"""Scan Context on the device: the descriptors and the comparison bit for bit against the numpy float32 restatement
(tests/scan_context_numpy.py), and the appearance loop gate `lsr_search_loop_appearance` against the public entries made by hand and
against the gate restated on the CPU oracle — on a route whose drift defeats the reference's range gate."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from lidarslam_ros2_amd import (AppearanceLoopParams, GeneralizedIterativeClosestPoint, LoopClosureParams, MapArray,
                                NormalDistributionsTransform, ScanContextParams, SubMap, _capi, poseLattice, scanContextGuess, search_loop,
                                search_loop_appearance, synth, DIRECT7)
from lidarslam_ros2_amd.posemath import pose_delta
from oracle import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_context_numpy as SC  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
TOL_T, TOL_R = 1e-3, 1e-4   # the project's bar: metres / radians
XYZI16 = (16, (0, 4, 8, 12))
XYZI32 = (32, (0, 4, 8, 16))


def _params(R, S, L=80.0):
    return ScanContextParams(R, S, L, 2.0)


def _backend_ndt():
    ndt = NormalDistributionsTransform(0)  # graph_based_slam_component.cpp:64-72
    ndt.setMaximumIterations(100)
    ndt.setResolution(5.0)
    ndt.setTransformationEpsilon(0.01)
    ndt.setNeighborhoodSearchMethod(DIRECT7)
    return ndt


@pytest.fixture(scope="module")
def reg():
    return NormalDistributionsTransform(0)


class _Cloud:
    def __init__(self, cloud):
        self.cloud, self.position, self.orientation, self.distance = cloud, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), 0.0


def _hand_points(R, S, L):
    """The corner cases of the CPU tests for one parameter set: ring edges, both half-plane rules, signed zeros, the origin, the sector
    boundaries themselves, the rim, non-finite coordinates, heights at and below -z_offset."""
    pts = [(0.0, 0.0, 1.0), (-0.0, -0.0, 1.5), (0.0, -0.0, 0.5), (1.0, -0.0, 1.0), (-1.0, 0.0, 1.0), (-1.0, -0.0, 2.0), (0.0, 3.0, 1.0),
           (-0.0, 3.0, 0.2), (0.0, -3.0, 1.0), (L, 0.0, 1.0), (0.0, -L, 1.0), (3e38, 3e38, 1.0), (math.nan, 1.0, 1.0), (1.0, math.inf, 1.0),
           (1.0, 1.0, -math.inf), (1.0, 1.0, math.nan), (1.0, 1.0, -2.0), (1.5, 1.0, -7.5), (2.0, 1.0, -1.9999999)]
    for k in range(1, R):
        e = k * L / R
        pts += [(e, 0.0, 1.0 + k), (0.0, e, 0.5), (-e, 0.0, 0.25), (float(np.nextafter(F(e), F(0))), 0.0, 3.0)]
    for k in range(1, S // 2):
        a = 2.0 * math.pi * k / S
        c, s = float(F(math.cos(a))), float(F(math.sin(a)))
        pts += [(5 * c, 5 * s, 1.0 + 0.01 * k), (-7 * c, -7 * s, 2.0 + 0.01 * k)]
    return np.array(pts, F)


def _cloud(n, R, S, L, seed=0):
    """n points: the hand cases first (as many as fit), then random ones over and beyond the disc."""
    rng = np.random.default_rng(100 + seed)
    hand = _hand_points(R, S, L)
    rnd = np.concatenate([rng.uniform(-1.1 * L, 1.1 * L, (n, 2)), rng.uniform(-3.0, 8.0, (n, 1))], axis=1).astype(F)
    return np.concatenate([hand, rnd])[:n] if n > hand.shape[0] else np.concatenate([rnd[: n // 2], hand])[:n]


def _records(pts, layout):
    step = layout[0] // 4
    out = np.full((pts.shape[0], step), 9.0, F)   # every other field holds something that must not be read
    for k in range(3):
        out[:, layout[1][k] // 4] = pts[:, k]
    return out


# ---- build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", SC.SHAPES)
def test_descriptor_bits(reg, R, S):
    import torch

    L = 80.0 if (R, S) != (7, 10) else 37.3
    prm = _params(R, S, L)
    sizes = (0, 1, 63, 64, 65, 257, 5000, 9000)    # 9000: more than two workgroups' slices, merged in the output
    clouds = [_cloud(n, R, S, L, seed=n) for n in sizes]
    ref = np.stack([SC.descriptor(c, R, S, L, 2.0) for c in clouds])
    assert np.count_nonzero(ref[-2]) > min(R * S, 200) // 2
    for layout in (XYZI32, XYZI16):
        host = [_Cloud(_records(c, layout)) for c in clouds]
        got = reg.scanContext(host, prm, layout)
        assert got.dtype == np.float32 and got.shape == (len(sizes), R, S)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), layout
        dev = [_Cloud(torch.from_numpy(h.cloud).cuda()) for h in host]
        got_dev = reg.scanContext(dev, prm, layout)
        assert got_dev.is_cuda and np.array_equal(got_dev.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        out_host = np.full((len(sizes), R, S), 5.0, F)     # device input, host output, into a buffer that held something
        assert reg.scanContext(dev, prm, layout, out_host) is not None and np.array_equal(out_host.view(np.uint32), ref.view(np.uint32))
        out_dev = torch.full((len(sizes), R, S), 5.0, dtype=torch.float32, device="cuda")   # host input, device output
        reg.scanContext(host, prm, layout, out_dev)
        assert np.array_equal(out_dev.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    # the same points in reversed order: the same bytes
    rev = reg.scanContext([_Cloud(_records(c[::-1].copy(), XYZI32)) for c in clouds], prm, XYZI32)
    assert np.array_equal(rev.view(np.uint32), ref.view(np.uint32))


def test_nine_submaps_two_empty_and_the_appended_call(reg):
    import torch

    R, S, L = 20, 60, 80.0
    prm = _params(R, S, L)
    sizes = (300, 0, 4097, 65, 0, 5000, 1, 8193, 64)
    clouds = [_cloud(n, R, S, L, seed=50 + i) for i, n in enumerate(sizes)]
    ref = np.stack([SC.descriptor(c, R, S, L, 2.0) for c in clouds])
    assert not ref[1].any() and not ref[4].any()
    for device in (False, True):
        subs = [_Cloud(torch.from_numpy(_records(c, XYZI32)).cuda() if device else _records(c, XYZI32)) for c in clouds]
        whole = reg.scanContext(subs, prm)
        whole = whole.cpu().numpy() if device else whole
        assert np.array_equal(whole.view(np.uint32), ref.view(np.uint32))
        for k in (1, 4, 8):   # a call over submaps + k writing at descriptor k: the bytes the whole call writes there
            table = (torch.zeros((9, R, S), dtype=torch.float32, device="cuda") if device else np.zeros((9, R, S), F))
            reg.scanContext(subs[:k], prm, XYZI32, table)
            reg.scanContext(subs[k:], prm, XYZI32, table[k:])
            table = table.cpu().numpy() if device else table
            assert np.array_equal(table.view(np.uint32), ref.view(np.uint32)), (device, k)


# ---- match ---------------------------------------------------------------------------------------------------------------------------
_match_cases = {}


def _match_case(R, S):
    """257 candidate descriptors of one shape — the route's clouds, an all-zero one, rolled copies — 3 queries among them, and the
    restated answer, computed once."""
    if (R, S) not in _match_cases:
        route = SC.drifted_route()
        base = [SC.descriptor(sm["cloud"], R, S, 80.0, 2.0) for sm in route] + [np.zeros((R, S), F)]
        cand = list(base)
        k = 0
        while len(cand) < 257:
            cand.append(np.roll(base[k % len(base)], 1 + (7 * k) % S, axis=1))
            k += 1
        Cd = np.stack(cand)
        Q = np.stack([Cd[20], Cd[21], Cd[3]])      # the latest submap (its exact copy is candidate 20), the all-zero one, another
        _match_cases[(R, S)] = (Q, Cd) + SC.match(Q, Cd, R, S)
    return _match_cases[(R, S)]


@pytest.mark.parametrize("R,S", SC.SHAPES)
def test_match_bits(reg, R, S):
    import torch

    prm = _params(R, S)
    Q, Cd, dist, shift = _match_case(R, S)
    assert dist[0, 20] <= 1e-6 and (R == 1 or shift[0, 20] == 0) and np.all(dist[1] == 1.0) and not shift[1].any()
    for nq, nc in ((1, 1), (1, 65), (3, 257)):
        d, s = reg.matchScanContext(Q[:nq], Cd[:nc], prm)
        assert d.shape == (nq, nc) and d.dtype == np.float32 and s.dtype == np.int32
        assert np.array_equal(d.view(np.uint32), dist[:nq, :nc].view(np.uint32)), (nq, nc)
        assert np.array_equal(s, shift[:nq, :nc]), (nq, nc)
    d, s = reg.matchScanContext(torch.from_numpy(Q).cuda(), torch.from_numpy(Cd).cuda(), prm)     # descriptors resident in HBM
    assert np.array_equal(d.view(np.uint32), dist.view(np.uint32)) and np.array_equal(s, shift)
    d1, s1 = reg.matchScanContext(Q[0], Cd, prm)                                                  # one query = row 0 of Q x N
    assert np.array_equal(d1[0].view(np.uint32), d[0].view(np.uint32)) and np.array_equal(s1[0], s[0])
    if S >= 4:    # a rolled copy is found at its roll
        dr, sr = reg.matchScanContext(Cd[0], np.roll(Cd[0], S // 4 + 1, axis=1), prm)
        assert abs(float(dr[0, 0])) <= 1e-6 and sr[0, 0] == S // 4 + 1


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
LOOP = dict(threshold_loop_closure_score=1.0, distance_loop_closure=20.0, range_of_searching_loop_closure=20.0, search_submap_num=3,
            voxel_leaf_size=0.2)


@pytest.fixture(scope="module")
def route():
    return SC.drifted_route()


def _submaps(route, device=False):
    out = []
    for sm in route:
        cloud = synth.as_pointxyzi(sm["cloud"])
        if device:
            import torch
            cloud = torch.from_numpy(cloud).cuda()
        out.append(SubMap(cloud, sm["position"], sm["orientation"], sm["distance"]))
    return out


@pytest.fixture(scope="module")
def descriptors(route):
    D = NormalDistributionsTransform(0).scanContext(_submaps(route))
    assert np.array_equal(D.view(np.uint32), SC.route_descriptors().view(np.uint32))
    return D


@pytest.fixture(scope="module")
def lattice_edges(route, descriptors):
    ndt = _backend_ndt()
    edges = search_loop_appearance(ndt, _submaps(route), descriptors, AppearanceLoopParams(loop=LoopClosureParams(**LOOP, top_k=2)))
    return ndt, edges


def test_the_range_gate_never_sees_the_revisit(route):
    edges = search_loop(_backend_ndt(), _submaps(route), LoopClosureParams(**LOOP, top_k=16))
    assert edges and not any(e.accepted for e in edges)
    assert all(e.pair_id[0] not in (0, 1) for e in edges)


def test_appearance_gate_closes_the_loop(route, descriptors, lattice_edges):
    ndt, edges = lattice_edges
    assert [e.pair_id for e in edges] == [(0, 20), (1, 20)] and edges[0].shift == 0 and edges[1].shift == 0
    dist, _ = SC.match(descriptors[-1], descriptors)
    assert edges[0].sc_distance == dist[0, 0] and edges[1].sc_distance == dist[0, 1]
    # candidate_distance stays the (drifted) position distance
    assert edges[0].candidate_distance == pytest.approx(np.linalg.norm(np.array(route[0]["position"]) - np.array(route[-1]["position"])), rel=1e-12)
    assert edges[0].candidate_distance > 20.0
    for e in edges:
        truth = np.linalg.inv(route[e.pair_id[0]]["truth"]) @ route[-1]["truth"]
        dt, dr = pose_delta(e.relative_pose, truth)
        print("device appearance gate", e.pair_id, e.sc_distance, e.shift, e.fitness_score, dt, dr)
        assert e.accepted and dt < 0.03 and dr < 2e-3, (e.pair_id, dt, dr)
    # the object is left as after one candidate: the FIRST candidate's pose and window
    assert np.array_equal(ndt.getFinalTransformation(), edges[0].final_transformation)
    assert ndt.getFitnessScore() == pytest.approx(edges[0].fitness_score, rel=1e-12)


def _by_hand(route, sub, G, prm):
    """The first candidate's evaluation through the public entries on a fresh object."""
    fresh = _backend_ndt()
    init = oracle.pose_msg_to_matrix(route[-1]["position"], route[-1]["orientation"])
    window = [i for i in range(0 - LOOP["search_submap_num"], 0 + LOOP["search_submap_num"] + 1) if 0 <= i < len(route)]
    n_target = fresh.setInputTargetFramesFiltered([sub[i].cloud for i in window],
                                                  [oracle.pose_msg_to_matrix(route[i]["position"], route[i]["orientation"]) for i in window],
                                                  LOOP["voxel_leaf_size"])
    fresh.setInputSource(oracle.transform_point_cloud(route[-1]["cloud"], init.astype(F)))
    pose, res, report = fresh.searchPose(G, prm.lattice_n, prm.lattice_step, prm.n_yaw, prm.yaw_step, prm.search_top_k, prm.min_sep_m,
                                         prm.min_sep_rad)
    return dict(final=pose, fitness=fresh.getFitnessScore(), n_target=n_target, report=report, result=res, init=init)


def _mul(A, B):
    """4x4 fp64 product, every entry summed k ascending from 0 — the entry's own loop."""
    out = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            acc = 0.0
            for k in range(4):
                acc += float(A[r, k]) * float(B[k, c])
            out[r, c] = acc
    return out


def _relative_pose(final, init, frm):
    """from^-1 (final init) as the entry evaluates it: Isometry3d::inverse() = [R^T | -(R^T t)], two 4x4 products."""
    inv = np.eye(4)
    inv[:3, :3] = frm[:3, :3].T
    for r in range(3):
        inv[r, 3] = -(inv[r, 0] * frm[0, 3] + inv[r, 1] * frm[1, 3] + inv[r, 2] * frm[2, 3])
    return _mul(inv, _mul(np.asarray(final, np.float64), init))


def test_appearance_gate_equals_the_public_entries_by_hand(route, descriptors, lattice_edges):
    _, edges = lattice_edges
    e = edges[0]
    sub = _submaps(route)
    G = scanContextGuess(sub[0], sub[-1], e.shift, 60)
    assert np.array_equal(G, SC.guess64(route[0], route[-1], 0, 60).astype(F))
    prm = AppearanceLoopParams()
    hand = _by_hand(route, sub, G, prm)
    assert hand["n_target"] == e.n_target_points
    assert np.array_equal(hand["final"], e.final_transformation)
    assert hand["fitness"] == pytest.approx(e.fitness_score, rel=1e-12)
    rel = _relative_pose(hand["final"], hand["init"], oracle.pose_msg_to_matrix(route[0]["position"], route[0]["orientation"]))
    assert np.array_equal(rel, e.relative_pose)
    assert e.iterations == hand["result"]["iterations"] and e.converged == hand["result"]["converged"]
    # the oracle's NDT started from the device winner's coarse candidate lands on the device's winner
    rep = hand["report"]
    start = poseLattice(G, prm.lattice_n, prm.lattice_step, prm.n_yaw, prm.yaw_step)[rep["kept"][rep["winner"]]]
    ref = SC.appearance_gate(route, SC.route_descriptors(), **{k: v for k, v in LOOP.items() if k != "range_of_searching_loop_closure"},
                             starts={0: start}, num_threads=min(32, oracle.max_threads()))[0]
    dt, dr = pose_delta(e.final_transformation, ref["final"])
    assert dt <= TOL_T and dr <= TOL_R, (dt, dr)
    assert e.fitness_score == pytest.approx(ref["fitness_score"], rel=1e-3) and e.n_target_points == ref["n_target_points"]


def test_guess_alone_equals_the_restated_gate(route, descriptors):
    prm = AppearanceLoopParams(loop=LoopClosureParams(**LOOP), lattice_n=(1, 1, 1), search_top_k=1)
    edges = search_loop_appearance(_backend_ndt(), _submaps(route), descriptors, prm)
    ref = SC.appearance_gate(route, SC.route_descriptors(), **{k: v for k, v in LOOP.items() if k != "range_of_searching_loop_closure"},
                             lattice_n=(1, 1, 1), search_top_k=1, num_threads=min(32, oracle.max_threads()))
    assert len(edges) == len(ref) == 1
    e, o = edges[0], ref[0]
    assert e.pair_id == o["pair_id"] == (0, 20) and e.shift == o["shift"] and e.sc_distance == F(o["sc_distance"])
    assert e.n_target_points == o["n_target_points"] and e.iterations == o["iterations"] and e.accepted == o["accepted"]
    dt, dr = pose_delta(e.final_transformation, o["final"])
    assert dt <= TOL_T and dr <= TOL_R, (dt, dr)
    dt, dr = pose_delta(e.relative_pose, o["relative_pose"])
    assert dt <= TOL_T and dr <= TOL_R, (dt, dr)
    assert e.fitness_score == pytest.approx(o["fitness_score"], rel=1e-3)
    assert e.candidate_distance == pytest.approx(o["candidate_distance"], rel=1e-12)


def test_device_resident_clouds_and_descriptors_give_the_same_edge(route, descriptors, lattice_edges):
    import torch

    _, host = lattice_edges
    reg = _backend_ndt()
    sub = _submaps(route, device=True)
    D = reg.scanContext(sub)
    assert D.is_cuda and np.array_equal(D.cpu().numpy().view(np.uint32), descriptors.view(np.uint32))
    dev = search_loop_appearance(reg, sub, D, AppearanceLoopParams(loop=LoopClosureParams(**LOOP, top_k=2)))
    assert len(dev) == len(host) == 2
    for e, d in zip(host, dev):
        assert e.pair_id == d.pair_id and e.shift == d.shift and e.sc_distance == d.sc_distance
        assert np.array_equal(e.final_transformation, d.final_transformation)
        assert e.fitness_score == d.fitness_score
        assert np.array_equal(e.relative_pose, d.relative_pose)
    torch.cuda.synchronize()


def test_gicp_object_aligns_once_from_the_guess(route, descriptors):
    gicp = GeneralizedIterativeClosestPoint(0)  # graph_based_slam_component.cpp:74-82
    gicp.setMaxCorrespondenceDistance(30)
    gicp.setMaximumIterations(100)
    gicp.setTransformationEpsilon(1e-8)
    gicp.setEuclideanFitnessEpsilon(1e-6)
    gicp.setRANSACIterations(0)
    edges = search_loop_appearance(gicp, _submaps(route), descriptors, AppearanceLoopParams(loop=LoopClosureParams(**LOOP)))
    assert len(edges) == 1 and edges[0].pair_id == (0, 20) and edges[0].shift == 0
    e = edges[0]
    assert np.all(np.isfinite(e.final_transformation)) and np.all(np.isfinite(e.relative_pose)) and math.isfinite(e.fitness_score)
    assert e.n_target_points > 0 and e.iterations > 0


def test_no_candidate_is_ok_with_nothing_evaluated(route, descriptors):
    sub = _submaps(route)
    far = AppearanceLoopParams(loop=LoopClosureParams(**dict(LOOP, distance_loop_closure=1e6)))
    assert search_loop_appearance(_backend_ndt(), sub, descriptors, far) == []
    assert search_loop_appearance(_backend_ndt(), sub, descriptors, AppearanceLoopParams(loop=LoopClosureParams(**LOOP), sc_distance_threshold=0.05)) == []


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(route, descriptors):
    reg = _backend_ndt()
    lib = _capi.load()
    n = len(route)
    sub = _submaps(route)
    arr = (_capi.SubMap * n)()
    for i, sm in enumerate(sub):
        arr[i].position[:] = sm.position
        arr[i].orientation[:] = sm.orientation
        arr[i].distance = sm.distance
        arr[i].cloud = sm.cloud.ctypes.data
        arr[i].n_points = sm.cloud.shape[0]
    D = np.ascontiguousarray(descriptors)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def prm(R=20, S=60, L=80.0, zo=2.0, thr=0.4, top_k=16):
        return _capi.AppearanceLoopParams(_capi.LoopParams(1.0, 20.0, 20.0, 3, 0.2, 1, 0), _capi.ScanContextParams(R, S, L, zo), thr,
                                          _capi.PoseSearchParams(_capi.PoseLattice((C.c_int32 * 3)(7, 7, 1), (C.c_double * 3)(1, 1, 1), 1, 0.0),
                                                                 top_k, 0.9, 0.13))

    edges = (_capi.LoopEdge * 2)()
    C.memset(edges, 0x5A, C.sizeof(edges))
    before = bytes(edges)
    shifts, scd = np.full(2, 77, np.int32), np.full(2, 7.0, F)
    n_eval = C.c_int32(-5)

    def call(p, submaps=arr, num=n, desc=D.ctypes.data, nd=n, stride=32, e=edges):
        return lib.lsr_search_loop_appearance(reg._h, submaps, num, stride, 0, C.c_void_p(desc), nd, 0, C.byref(p) if p is not None else None,
                                              e, shifts.ctypes.data_as(ip), scd.ctypes.data_as(fp), 2, C.byref(n_eval))

    bad = [prm(S=61), prm(R=0), prm(R=41), prm(S=0), prm(S=122), prm(L=0.0), prm(L=-3.0), prm(L=math.nan), prm(thr=math.nan), prm(top_k=0),
           prm(top_k=17)]
    for p in bad:
        assert call(p) == -1
    assert call(prm(), desc=None) == -1                 # a null table
    assert call(prm(), nd=n - 1) == -1                  # a descriptor count that does not match
    assert call(prm(), nd=n + 1) == -1
    assert call(None) == -1 and call(prm(), submaps=None) == -1 and call(prm(), num=0) == -1 and call(prm(), stride=10) == -1
    assert call(prm(), e=None) == -1
    assert bytes(edges) == before and n_eval.value == -5 and np.all(shifts == 77) and np.all(scd == 7.0)

    # build and match
    lay = _capi.Pc2Layout(32, 0, 4, 8, 16)
    out = np.full((n, 20, 60), 5.0, F)
    for p in (_capi.ScanContextParams(20, 61, 80.0, 2.0), _capi.ScanContextParams(41, 60, 80.0, 2.0), _capi.ScanContextParams(20, 60, 0.0, 2.0)):
        assert lib.lsr_scan_context_build(reg._h, arr, n, C.byref(lay), 0, C.byref(p), out.ctypes.data, 0) == -1
    good = _capi.ScanContextParams(20, 60, 80.0, 2.0)
    assert lib.lsr_scan_context_build(reg._h, arr, n, None, 0, C.byref(good), out.ctypes.data, 0) == -1
    assert lib.lsr_scan_context_build(reg._h, arr, n, C.byref(lay), 0, None, out.ctypes.data, 0) == -1
    assert lib.lsr_scan_context_build(reg._h, arr, 0, C.byref(lay), 0, C.byref(good), out.ctypes.data, 0) == -1
    assert lib.lsr_scan_context_build(reg._h, arr, n, C.byref(lay), 0, C.byref(good), None, 0) == -1
    assert lib.lsr_scan_context_build(reg._h, arr, n, C.byref(_capi.Pc2Layout(32, 0, 4, 30, 16)), 0, C.byref(good), out.ctypes.data, 0) == -1
    assert lib.lsr_scan_context_build(None, arr, n, C.byref(lay), 0, C.byref(good), out.ctypes.data, 0) == -1
    assert np.all(out == 5.0)
    dist, shift = np.full(n, 7.0, F), np.full(n, 77, np.int32)
    dp, sp = dist.ctypes.data_as(fp), shift.ctypes.data_as(ip)
    assert lib.lsr_scan_context_match(reg._h, D.ctypes.data, 1, D.ctypes.data, n, 0, C.byref(_capi.ScanContextParams(20, 59, 80.0, 2.0)), dp, sp) == -1
    assert lib.lsr_scan_context_match(reg._h, None, 1, D.ctypes.data, n, 0, C.byref(good), dp, sp) == -1
    assert lib.lsr_scan_context_match(reg._h, D.ctypes.data, 0, D.ctypes.data, n, 0, C.byref(good), dp, sp) == -1
    assert lib.lsr_scan_context_match(reg._h, D.ctypes.data, 1, D.ctypes.data, n, 0, None, dp, sp) == -1
    assert lib.lsr_scan_context_match(reg._h, D.ctypes.data, 1, D.ctypes.data, n, 0, C.byref(good), None, sp) == -1
    assert np.all(dist == 7.0) and np.all(shift == 77)


# ---- the resident table of a MapArray ------------------------------------------------------------------------------------------------
def test_map_array_table_grows_keyframe_by_keyframe(route, descriptors):
    import torch

    for device in (False, True):
        reg = NormalDistributionsTransform(0)
        ma = MapArray()
        assert ma.scan_contexts(reg).shape == (0, 20, 60)
        for k, sm in enumerate(route[:7]):
            rec = synth.as_pointxyzi(sm["cloud"])
            ma.append(torch.from_numpy(rec).cuda() if device else rec, oracle.pose_msg_to_matrix(sm["position"], sm["orientation"]), sm["distance"])
            if k in (0, 1, 4, 6):        # one new keyframe, then several at once, across two growths of the table
                T = ma.scan_contexts(reg)
                T = T.cpu().numpy() if device else T
                assert T.shape == (k + 1, 20, 60) and np.array_equal(T.view(np.uint32), descriptors[: k + 1].view(np.uint32)), (device, k)
        other = ma.scan_contexts(reg, ScanContextParams(7, 10, 37.3, 2.0))     # other parameters: the table starts again
        other = other.cpu().numpy() if device else other
        assert np.array_equal(other, np.stack([SC.descriptor(sm["cloud"], 7, 10, 37.3, 2.0) for sm in route[:7]]))

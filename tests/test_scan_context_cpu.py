"""Scan Context without a device: the definition's corner cases on the numpy restatement (tests/scan_context_numpy.py), the two host
entries of the C ABI against it, and the appearance loop gate as a procedure on the CPU oracle — on a route whose drift defeats the
reference's range gate."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_context_numpy as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("lsr_scan_context_tables", "lsr_scan_context_guess", "lsr_scan_context_build", "lsr_scan_context_match",
       "lsr_search_loop_appearance")


def _cell_centre(r, s, R, S, L):
    rad = (r + 0.5) * L / R
    a = (s + 0.5) * 2.0 * math.pi / S
    return rad * math.cos(a), rad * math.sin(a)


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", SC.SHAPES)
def test_one_point_per_cell_lands_in_its_cell(R, S):
    L = 80.0
    pts = np.array([[*_cell_centre(r, s, R, S, L), 0.01 * (r * S + s)] for r in range(R) for s in range(S)], F)
    d = SC.descriptor(pts, R, S, L, 2.0)
    assert np.array_equal(d.reshape(-1), pts[:, 2] + F(2.0))
    kept, ring, sector, _ = SC.cells_of(pts, R, S, L, 2.0)
    assert kept.all() and np.array_equal(ring * S + sector, np.arange(R * S))


def test_ring_edges_and_half_plane_rules():
    R, S, L = 4, 8, 8.0     # edges at 2, 4, 6 (squares exact in float), sectors of 45 degrees
    z = F(1.0)
    cases = [  # (x, y) -> (ring, sector)
        ((2.0, 0.0), (1, 0)),            # exactly on a ring edge: the outer ring
        ((np.nextafter(F(2.0), F(0.0)), 0.0), (0, 0)),
        ((6.0, 0.0), (3, 0)),
        ((-2.0, 0.0), (1, 4)),           # y == 0, x < 0: the lower half's first sector
        ((-2.0, -0.0), (1, 4)),
        ((0.0, 3.0), (1, 2)),            # x == 0: cos(pi / 2) rounds to a positive float, the boundary counts
        ((0.0, -3.0), (1, 6)),
        ((-0.0, 3.0), (1, 2)),
        ((1.0, 1.0), (0, 1)),            # on the 45 degree boundary: cos == sin in float, the difference is +0
        ((1.0, -0.0), (0, 0)),           # y == -0 with x >= 0 is the upper half
        ((0.0, 0.0), (0, 3)),            # the origin: every boundary test is 0 >= 0
        ((-0.0, -0.0), (0, 3)),
        ((5.0, -5.0), (3, 7)),           # r2 = 50 < 64
    ]
    for (x, y), (ring, sector) in cases:
        d = SC.descriptor(np.array([[x, y, z]], F), R, S, L, 2.0)
        want = np.zeros((R, S), F)
        want[ring, sector] = F(3.0)
        assert np.array_equal(d, want), ((x, y), np.argwhere(d > 0))


def test_skipped_points_and_the_floor_of_a_cell():
    R, S, L = 4, 8, 8.0
    inf, nan = np.inf, np.nan
    gone = np.array([[nan, 1, 1], [1, inf, 1], [1, 1, -inf], [1, 1, nan], [8.0, 0.0, 1], [0.0, -8.0, 1], [6.0, 6.0, 1], [3e38, 3e38, 1],
                     [1.0, 1.0, -2.0], [1.0, 1.0, -7.5]], F)     # non-finite, r2 >= L2 (on the rim, beyond, overflowing), z + z_offset <= 0
    assert not SC.descriptor(gone, R, S, L, 2.0).any()
    d = SC.descriptor(np.array([[1.0, 0.5, -2.0], [1.0, 0.5, -1.5], [1.0, 0.5, -1.75]], F), R, S, L, 2.0)
    assert d[0, 0] == F(0.5) and np.count_nonzero(d) == 1                      # the maximum, whatever the order
    assert np.signbit(SC.descriptor(np.array([[1.0, 0.5, -2.0]], F), R, S, L, 2.0)).sum() == 0   # +0, never -0
    assert not SC.descriptor(np.zeros((0, 3), F), R, S, L, 2.0).any()


# ---- exact rotations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,S", [(20, 60), (7, 12), (40, 120)])
def test_exact_rotation_rolls_the_descriptor(R, S):
    rng = np.random.default_rng(7)
    pts = np.concatenate([rng.uniform(-70, 70, (5000, 2)), rng.uniform(-1.5, 6.0, (5000, 1))], axis=1).astype(F)
    prm = dict(num_rings=R, num_sectors=S, max_radius=80.0, z_offset=2.0)
    d0 = SC.descriptor(pts, **prm)
    r90 = np.stack([-pts[:, 1], pts[:, 0], pts[:, 2]], axis=1)       # (x, y) -> (-y, x): exact
    r180 = np.stack([-pts[:, 0], -pts[:, 1], pts[:, 2]], axis=1)
    d90, d180 = SC.descriptor(r90, **prm), SC.descriptor(r180, **prm)
    assert np.array_equal(d90, np.roll(d0, S // 4, axis=1))
    assert np.array_equal(d180, np.roll(d0, S // 2, axis=1))
    dist, shift = SC.match(d0, np.stack([d0, d90, d180]), R, S)
    assert list(shift[0]) == [0, S // 4, S // 2]
    assert np.all(np.abs(dist[0]) < 1e-6)
    # the same points in another order: the same bits
    assert np.array_equal(SC.descriptor(pts[::-1], **prm), d0)


def test_distance_corner_cases():
    R, S = 3, 4
    z = np.zeros((R, S), F)
    a = z.copy()
    a[:, 1] = (1.0, 2.0, 2.0)
    dist, shift = SC.match(np.stack([z, a]), np.stack([z, a, np.roll(a, 2, axis=1), 2 * a]), R, S)
    assert np.array_equal(dist[0], np.ones(4, F)) and not shift[0].any()           # no column counts: 1, at the lowest shift
    assert dist[1, 0] == F(1.0)
    assert dist[1, 1] == F(0.0) and shift[1, 1] == 0
    assert dist[1, 2] == F(0.0) and shift[1, 2] == 2
    assert dist[1, 3] == F(0.0)                                                     # a cosine distance: scale does not matter


# ---- the host entries of the C ABI -----------------------------------------------------------------------------------------------------
def test_symbols_keys_and_structs():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes and re.search(r"\bint " + name + r"\(", hdr)
    assert _capi.SCAN_CONTEXT_BUILD_MS == 24 and re.search(r"LSR_SCAN_CONTEXT_BUILD_MS\s*=\s*24\b", hdr)
    assert _capi.SCAN_CONTEXT_MATCH_MS == 25 and re.search(r"LSR_SCAN_CONTEXT_MATCH_MS\s*=\s*25\b", hdr)
    assert re.search(r"#define LSR_SCAN_CONTEXT_MAX_RINGS 40\b", hdr) and re.search(r"#define LSR_SCAN_CONTEXT_MAX_SECTORS 120\b", hdr)
    assert C.sizeof(_capi.ScanContextParams) == 24
    assert C.sizeof(_capi.AppearanceLoopParams) == C.sizeof(_capi.LoopParams) + 24 + 8 + C.sizeof(_capi.PoseSearchParams)


@pytest.mark.parametrize("R,S", SC.SHAPES + ((40, 118), (13, 4)))
@pytest.mark.parametrize("L", [80.0, 37.3, 0.1])
def test_tables_equal_the_restatement(R, S, L):
    from lidarslam_ros2_amd import ScanContextParams, scanContextTables

    edge2, b = scanContextTables(ScanContextParams(R, S, L, 2.0))
    e_ref, b_ref = SC.tables(R, S, L)
    assert edge2.dtype == np.float32 and np.array_equal(edge2, e_ref)
    assert b.shape == (S // 2 - 1, 2) and np.array_equal(b, b_ref)


def test_tables_refuse_bad_parameters_and_touch_nothing():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    fp = C.POINTER(C.c_float)
    e, b = np.full(64, 7.0, F), np.full(128, 7.0, F)
    for R, S, L, zo in [(0, 60, 80.0, 2.0), (41, 60, 80.0, 2.0), (20, 61, 80.0, 2.0), (20, 0, 80.0, 2.0), (20, 122, 80.0, 2.0),
                        (20, 60, 0.0, 2.0), (20, 60, -1.0, 2.0), (20, 60, math.nan, 2.0), (20, 60, math.inf, 2.0), (20, 60, 80.0, math.nan)]:
        p = _capi.ScanContextParams(R, S, L, zo)
        assert lib.lsr_scan_context_tables(C.byref(p), e.ctypes.data_as(fp), b.ctypes.data_as(fp)) == -1, (R, S, L, zo)
    p = _capi.ScanContextParams(20, 60, 80.0, 2.0)
    assert lib.lsr_scan_context_tables(None, e.ctypes.data_as(fp), b.ctypes.data_as(fp)) == -1
    assert lib.lsr_scan_context_tables(C.byref(p), None, b.ctypes.data_as(fp)) == -1
    assert lib.lsr_scan_context_tables(C.byref(p), e.ctypes.data_as(fp), None) == -1
    assert np.all(e == 7.0) and np.all(b == 7.0)


def test_guess_equals_the_float64_evaluation():
    from lidarslam_ros2_amd import SubMap, _capi, scanContextGuess

    rng = np.random.default_rng(3)
    for t in range(200):
        S = int(rng.choice([2, 10, 60, 120]))
        shift = int(rng.integers(0, S))
        subs = []
        for _ in range(2):
            yaw = rng.uniform(-math.pi, math.pi)
            subs.append(dict(position=tuple(rng.uniform(-200, 200, 3)), orientation=(0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw))))
        if t % 5 == 0:   # any unit quaternion
            q = rng.normal(size=4)
            subs[0]["orientation"] = tuple(q / np.linalg.norm(q))
        G = scanContextGuess(SubMap(None, **subs[0]), SubMap(None, **subs[1]), shift, S)
        ref = SC.guess64(subs[0], subs[1], shift, S)
        assert G.dtype == np.float32 and G.shape == (4, 4)
        assert np.max(np.abs(G.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))) <= 1e-6
    # a turn of the latest scene by `shift` sectors about its own origin, then the candidate's pose
    lib = _capi.load()
    g = np.full(16, 7.0, F)
    a = _capi.SubMap()
    for shift, S in [(-1, 60), (60, 60), (0, 61), (0, 0), (0, 122)]:
        assert lib.lsr_scan_context_guess(C.byref(a), C.byref(a), shift, S, g.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lib.lsr_scan_context_guess(None, C.byref(a), 0, 60, g.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert lib.lsr_scan_context_guess(C.byref(a), C.byref(a), 0, 60, None) == -1
    assert np.all(g == 7.0)


# ---- the procedure on the drifted route ------------------------------------------------------------------------------------------------
def test_the_range_gate_loses_the_loop_and_appearance_finds_it():
    """Measured with the exact definition (float32, no angle function): distance of the last submap to submap 0 0.16974501, to
    submap 1 0.23664056, the next travel-gated one (submap 2) 0.5006845; shift 0 for both, 30 to 32 on the return leg."""
    from lidarslam_ros2_amd.posemath import pose_delta
    from oracle import oracle

    route, D = SC.drifted_route(), SC.route_descriptors()
    assert len(route) == 21
    nt = min(32, oracle.max_threads())
    # the reference's gate, defaults, NDT resolution 5.0: the candidate it picks is not the revisit, and it is rejected
    ref = oracle.search_loop(route, ndt_resolution=5.0, trans_eps=0.01, max_iterations=100, num_threads=nt)
    assert not any(e["accepted"] for e in ref) and all(e["pair_id"][0] not in (0, 1) for e in ref)
    true_gap = np.linalg.norm(route[0]["truth"][:3, 3] - route[-1]["truth"][:3, 3])
    stored_gap = np.linalg.norm(np.array(route[0]["position"]) - np.array(route[-1]["position"]))
    assert true_gap < 1.5 and stored_gap > 20.0
    # the ranking
    dist, shift = SC.match(D[-1], D, 20, 60)
    travel_ok = [route[-1]["distance"] - sm["distance"] > 20.0 for sm in route]
    order = SC.rank(dist[0], travel_ok, 1e9)
    print("scan context distances", [(i, float(dist[0, i]), int(shift[0, i])) for i in order])
    assert order[:2] == [0, 1] and shift[0, 0] == 0 and shift[0, 1] == 0
    assert all(dist[0, i] >= dist[0, 1] + F(0.1) for i in order[2:])
    # the gate: candidate and heading from appearance, the translation from a lattice of NDT starts
    edges = SC.appearance_gate(route, D, top_k=16, lattice_n=(7, 7, 1), lattice_step=(1.0, 1.0, 1.0), n_yaw=1, search_top_k=16,
                               ndt_resolution=5.0, trans_eps=0.01, max_iterations=100, num_threads=nt)
    assert [e["pair_id"] for e in edges] == [(0, 20), (1, 20)]
    for e in edges:
        truth = np.linalg.inv(route[e["pair_id"][0]]["truth"]) @ route[-1]["truth"]
        dt, dr = pose_delta(e["relative_pose"], truth)
        print("appearance gate", e["pair_id"], "fitness", e["fitness_score"], "error", dt, dr)
        assert e["accepted"] and dt < 0.03 and dr < 2e-3, (e["pair_id"], dt, dr)


def test_cpp_snippet_compiles_and_links(tmp_path):
    """the block of tests/cpp/scan_context_snippets.cpp, compiled against include/lidarslam_reg/scan_context.hpp and
    linked against the library; the program runs the tables, the guess and the refusals that need no device."""
    import subprocess
    import textwrap

    src = os.path.join(ROOT, "tests", "cpp", "scan_context_snippets.cpp")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "scan_context_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0 and "SCAN_CONTEXT_SNIPPETS ok=2 refused=3" in run.stdout, (run.stdout, run.stderr)
    text, doc = open(src).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("### 3l.")[1]
    block = text.split("// [scan-context-snippet begin: search_loop]\n")[1].split("  // [scan-context-snippet end: search_loop]")[0]
    assert textwrap.dedent(block).strip("\n").rstrip() in textwrap.dedent(section.split("```cpp\n")[1].split("```")[0])

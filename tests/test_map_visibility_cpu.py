"""Visibility votes without a device: the definition's corner cases on the numpy restatement (tests/map_visibility_numpy.py), the host
entry lsr_visibility_pairs against an fp64 evaluation, its refusals, the exports — and the behaviour of the definition on the synthetic
world with a car driving ahead of the vehicle."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_visibility_numpy as MV  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("lsr_visibility_pairs", "lsr_depth_images_build", "lsr_visibility_votes", "lsr_assemble_map_static")
INF, NAN = np.inf, np.nan


def _small(**kw):
    """W = 8, H = 4, T = 1: rs = 2 and Tf = 1 are exact, a face is 8 columns, a row is half a unit of z / d."""
    base = dict(face_width=8, height=4, max_tan_elevation=1.0, min_range=0.5, max_range=80.0)
    base.update(kw)
    return MV.params(**base)


def _pix(p, *pts):
    ok, row, col, r = MV.pixel(np.array(pts, F), p)
    return [(int(rw), int(cl)) if o else None for o, rw, cl in zip(ok, row, col)]


# ---- hand cases: step 1 ------------------------------------------------------------------------------------------------------------------
def test_face_ties_and_the_last_column_of_a_face():
    p = _small()
    # |x| == |y| belongs to the x faces: u = +-1, and u = +1 clamps to the face's last column
    assert _pix(p, (5, 5, 0), (-5, 5, 0), (-5, -5, 0), (5, -5, 0)) == [(2, 7), (2, 16), (2, 23), (2, 0)]
    # the next face begins at the next column; the last column wraps to the first
    up = np.nextafter(F(5), F(INF))
    assert _pix(p, (5, up, 0), (-5, up, 0), (-up, 5, 0), (-5, -up, 0), (up, -5, 0)) == [(2, 8), (2, 15), (2, 16), (2, 24), (2, 0)]
    assert _pix(p, (5, -up, 0)) == [(2, 31)]
    # azimuth ascends with the column across all four faces
    az = np.deg2rad(np.arange(-44.0, 315.0, 7.0))
    _, _, col, _ = MV.pixel(np.stack([10 * np.cos(az), 10 * np.sin(az), 0 * az], axis=1).astype(F), p)
    assert np.all(np.diff(col) >= 0) and col[0] == 0 and col[-1] == 31


def test_signed_zeros_and_the_axis():
    p = _small()
    assert _pix(p, (5, 0.0, 0.0), (5, -0.0, -0.0), (0.0, 5, 0), (-0.0, 5, 0), (-5, 0.0, 0), (0.0, -5, 0), (-0.0, -5, -0.0)) == \
        [(2, 4), (2, 4), (2, 12), (2, 12), (2, 20), (2, 28), (2, 28)]
    assert _pix(p, (0.0, 0.0, 5), (-0.0, 0.0, 1), (0.0, -0.0, -3), (0.0, 0.0, 0.0)) == [None] * 4          # d == 0: no pixel


def test_row_edges_are_judged_in_float():
    p = _small()
    d = F(4.0)
    # v = -T is the first row's lower edge and inside; v = T is outside
    assert _pix(p, (4, 0, -4), (4, 0, 4)) == [(0, 4), None]
    # just inside the lower edge: a = 2^-24; just outside: a = -2^-23
    assert _pix(p, (4, 0, -4 + 2.0 ** -22), (4, 0, -4 - 2.0 ** -21)) == [(0, 4), None]
    # below the upper edge: z = 4 - 2^-21 gives a = 2 - 2^-23, row 3; the float next to 4 gives v = 1 - 2^-24, and v + Tf ROUNDS to 2: no pixel
    assert _pix(p, (4, 0, 4 - 2.0 ** -21), (4, 0, np.nextafter(d, F(0)))) == [(3, 4), None]
    assert _pix(p, (4, 0, -2), (4, 0, -0.0), (4, 0, 2)) == [(1, 4), (2, 4), (3, 4)]
    # a quotient that overflows: the row is not finite
    tiny = F(1e-38)
    assert _pix(_small(min_range=-1.0), (tiny, 0, 70), (tiny, 0, -70)) == [None, None]


def test_range_edges_overflow_and_non_finite_coordinates():
    p = _small()
    assert _pix(p, (0.5, 0, 0), (np.nextafter(F(0.5), F(0)), 0, 0), (80, 0, 0), (np.nextafter(F(80), F(0)), 0, 0)) == [(2, 4), None, None, (2, 4)]
    assert _pix(p, (3, 4, 0), (0, 3, 4)) == [(2, 9), None]                        # r = 5 exactly; z / d = 4 / 3 > T
    assert _pix(p, (3e38, 3e38, 0), (1e30, 0, 0), (0, -2e19, 2e19), (1e-30, 0, 0)) == [None] * 4   # x x overflows: r = +inf; underflows: r = 0
    assert _pix(p, (NAN, 1, 1), (1, NAN, 1), (1, 1, NAN), (INF, 1, 1), (1, -INF, 1), (1, 1, INF), (INF, INF, INF)) == [None] * 7
    # the origin is subtracted before all that: a record at the origin has d == 0, and an overflowing difference no pixel
    q = _small(sensor_origin=(1.0, 2.0, 3.0))
    D = MV.depth_image(np.array([[1, 2, 3], [6, 2, 3], [3e38, 2, 3], [1, 2, 9]], F), q)
    assert np.isfinite(D).sum() == 1 and D[2, 4] == F(5.0)
    D = MV.depth_image(np.array([[-3e38, 0, 0]], F), _small(sensor_origin=(3e38, 0.0, 0.0)))
    assert not np.isfinite(D).any()


def test_depth_image_is_a_minimum_whatever_the_order():
    p = _small()
    pts = np.array([[10, 0, 0], [7, 0, 0.1], [9, 0.2, 0], [NAN, 0, 0], [0, 0, 0]], F)
    D = MV.depth_image(pts, p)
    assert D.shape == (4, 32) and D.dtype == F
    assert D[2, 4] == np.sqrt(F(49.0) + F(0.1) * F(0.1)) and np.isfinite(D).sum() == 1
    assert np.array_equal(MV.depth_image(pts[::-1], p), D)
    assert D.view(np.uint32).max() == MV.INF_BITS and np.all(np.isinf(MV.depth_image(np.zeros((0, 3), F), p)))


# ---- step 3 ------------------------------------------------------------------------------------------------------------------------------
def test_erosion_wraps_columns_and_clamps_rows():
    D = np.full((4, 32), INF, F)
    D[0, 31] = 3.0
    D[3, 5] = 2.0
    E = MV.erode(D)
    want = np.full((4, 32), INF, F)
    for r, c in [(0, 30), (0, 31), (0, 0), (1, 30), (1, 31), (1, 0)]:
        want[r, c] = 3.0
    for r, c in [(2, 4), (2, 5), (2, 6), (3, 4), (3, 5), (3, 6)]:
        want[r, c] = 2.0
    assert np.array_equal(E, want)
    D[0, 0] = 1.0                  # column 0 reaches column 31 the other way round
    assert MV.erode(D)[0, 31] == 1.0 and MV.erode(D)[1, 31] == 1.0 and MV.erode(D)[0, 30] == 3.0


# ---- step 5 ------------------------------------------------------------------------------------------------------------------------------
def test_a_vote_needs_a_finite_pixel_and_strictly_more_depth():
    p = _small(margin=0.5)
    eye = np.eye(4, dtype=F)[None, :3]
    clouds = [np.array([[10, 0, 0], [0, 0, 5], [200, 0, 0]], F), np.zeros((0, 3), F)]
    first, other = np.array([0, 1, 1], np.int32), np.array([1], np.int32)

    def run(depth):
        E = np.full((2, 4, 32), INF, F)
        E[1, 2, 4] = depth
        return list(MV.votes(clouds, first, other, eye, E, p))

    assert run(INF) == [0, 0, 0]                                        # the neighbour saw nothing there: no vote
    assert run(F(10.5)) == [0, 0, 0]                                    # r + margin == E is not a vote
    assert run(np.nextafter(F(10.5), F(INF))) == [1, 0, 0]              # records without a pixel never get one
    assert run(F(3.0)) == [0, 0, 0]                                     # a surface in front of the record
    # the transform is lsr_assemble_map's expression, then the origin is subtracted
    shift = eye.copy()
    shift[0, 0, 3] = 2.0
    E = np.full((2, 4, 32), INF, F)
    E[1, 2, 4] = 20.0
    q = _small(margin=0.5, sensor_origin=(2.0, 0.0, 0.0))
    assert list(MV.votes(clouds, first, other, shift, E, q)) == [1, 0, 0]      # (10 + 2) - 2 = 10
    assert list(MV.votes(clouds, first, other, shift, E, p)) == [1, 0, 0]      # 12 + 0.5 < 20
    E[1, 2, 4] = 12.5
    assert list(MV.votes(clouds, first, other, shift, E, p)) == [0, 0, 0]


# ---- the host entry ------------------------------------------------------------------------------------------------------------------------
def _random_submaps(rng, n, spread):
    from lidarslam_ros2_amd import SubMap

    subs = []
    for _ in range(n):
        q = rng.normal(size=4)
        subs.append(SubMap(None, position=tuple(rng.uniform(-spread, spread, 3)), orientation=tuple(q / np.linalg.norm(q))))
    return subs


def _stored(subs):
    from lidarslam_ros2_amd.posemath import matrix_from_pose

    return np.stack([matrix_from_pose(s.position, s.orientation) for s in subs])


def _assert_pairs(got, ref):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert got[2].dtype == np.float32 and got[2].shape == ref[2].shape
    if ref[2].size:
        assert np.max(np.abs(got[2].astype(np.float64) - ref[2]) / np.maximum(1.0, np.abs(ref[2]))) <= 1e-6


@pytest.mark.parametrize("max_neighbours,keyframe_range", [(32, 30.0), (3, 30.0), (1, 1e9), (64, 5.0)])
def test_pairs_equal_the_float64_evaluation(max_neighbours, keyframe_range):
    from lidarslam_ros2_amd import visibilityPairs

    rng = np.random.default_rng(11)
    p = MV.params(max_neighbours=max_neighbours, keyframe_range=keyframe_range)
    for n in (1, 2, 13):
        subs = _random_submaps(rng, n, 20.0)
        _assert_pairs(visibilityPairs(subs, None, p), MV.pairs64(_stored(subs), p))
        poses = _stored(_random_submaps(rng, n, 20.0))                  # the optimiser's poses instead of the stored ones
        _assert_pairs(visibilityPairs(subs, poses, p), MV.pairs64(poses, p))
    first, other, _ = visibilityPairs(_random_submaps(rng, 13, 20.0), None, p)
    assert np.all(np.diff(first) <= max_neighbours)
    assert all(np.all(np.diff(other[a:b]) > 0) for a, b in zip(first[:-1], first[1:]))      # ascending k inside a keyframe's list


def test_pairs_rank_ties_to_the_lower_index_and_the_cap_binds():
    from lidarslam_ros2_amd import SubMap, visibilityPairs

    # on a line, 3 m apart (exact): keyframe 2 has 1 and 3 at 3 m, 0 and 4 at 6 m
    subs = [SubMap(None, position=(3.0 * i, 0.0, 0.0), orientation=(0.0, 0.0, 0.0, 1.0)) for i in range(5)]
    first, other, rel = visibilityPairs(subs, None, MV.params(max_neighbours=1))
    assert list(first) == [0, 1, 2, 3, 4, 5] and list(other) == [1, 0, 1, 2, 3]
    first, other, rel = visibilityPairs(subs, None, MV.params(max_neighbours=3))
    assert list(first) == [0, 3, 6, 9, 12, 15] and list(other[6:9]) == [0, 1, 3]      # 1 and 3, then 0 before 4
    assert np.array_equal(rel[6], np.array([[1, 0, 0, 6], [0, 1, 0, 0], [0, 0, 1, 0]], F))
    first, other, _ = visibilityPairs(subs, None, MV.params(keyframe_range=3.0))      # <= : exactly in range counts
    assert list(np.diff(first)) == [1, 2, 2, 2, 1]
    first, other, _ = visibilityPairs(subs, None, MV.params(keyframe_range=2.999))
    assert list(first) == [0] * 6 and other.size == 0


BAD = [dict(face_width=6), dict(face_width=1026), dict(face_width=9), dict(height=3), dict(height=513), dict(max_tan_elevation=0.0),
       dict(max_tan_elevation=NAN), dict(max_tan_elevation=INF), dict(min_range=80.0), dict(min_range=NAN), dict(max_range=INF),
       dict(max_range=0.0, min_range=-1.0), dict(margin=-0.1), dict(margin=NAN), dict(keyframe_range=0.0), dict(keyframe_range=NAN),
       dict(max_neighbours=0), dict(max_neighbours=65), dict(min_votes=0), dict(sensor_origin=(0.0, NAN, 0.0)),
       dict(sensor_origin=(INF, 0.0, 0.0))]


def test_pairs_refuse_and_touch_nothing():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    subs = (_capi.SubMap * 3)()
    for i in range(3):
        subs[i].orientation[3] = 1.0
        subs[i].position[0] = float(i)
    first, other, rel = np.full(4, 7, np.int32), np.full(6, 7, np.int32), np.full(72, 7.0, F)
    m = C.c_size_t(99)

    def call(p, s=subs, n=3, f=first, o=other, r=rel, cap=6, out=m):
        return lib.lsr_visibility_pairs(s, n, None, C.byref(p) if p is not None else None, f.ctypes.data_as(ip) if f is not None else None,
                                        o.ctypes.data_as(ip) if o is not None else None, r.ctypes.data_as(fp) if r is not None else None,
                                        cap, C.byref(out) if out is not None else None)

    for kw in BAD:
        assert call(MV.params(**kw).struct()) == -1, kw
    good = MV.params().struct()
    assert call(None) == -1 and call(good, s=None) == -1 and call(good, n=0) == -1
    assert call(good, f=None) == -1 and call(good, o=None) == -1 and call(good, r=None) == -1 and call(good, out=None) == -1
    assert m.value == 99
    assert call(good, cap=5) == -1 and m.value == 6                      # too small: the count, and nothing else
    assert np.all(first == 7) and np.all(other == 7) and np.all(rel == 7.0)
    assert call(good) == 0 and m.value == 6 and list(first) == [0, 2, 4, 6]
    assert call(MV.params(min_range=-5.0, max_range=1e-3, margin=0.0, min_votes=1000).struct()) == 0    # the ranges' edges are fine


def test_device_entries_refuse_a_null_handle_before_anything_else():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    n = C.c_size_t(5)
    assert lib.lsr_depth_images_build(None, None, 0, None, 0, None, 1, None, 0) == -1
    assert lib.lsr_visibility_votes(None, None, 0, None, 0, None, None, 0, None, None, 0, None, C.byref(n)) == -1
    assert lib.lsr_assemble_map_static(None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, None, C.byref(n), C.byref(n)) == -1
    assert n.value == 5


def test_symbols_keys_and_structs():
    from lidarslam_ros2_amd import VisibilityParams, _capi

    lib = _capi.load()
    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes and re.search(r"\bint " + name + r"\(", hdr)
    assert _capi.DEPTH_IMAGES_MS == 26 and re.search(r"LSR_DEPTH_IMAGES_MS\s*=\s*26\b", hdr)
    assert _capi.VISIBILITY_MS == 27 and re.search(r"LSR_VISIBILITY_MS\s*=\s*27\b", hdr)
    assert _capi.VISIBILITY_PIECE_BYTES == 56 and re.search(r"LSR_VISIBILITY_PIECE_BYTES\s*=\s*56\b", hdr)
    for name, value in (("FACE_WIDTH", 1024), ("HEIGHT", 512), ("NEIGHBOURS", 64)):
        assert getattr(_capi, "VISIBILITY_MAX_" + name) == value and re.search(r"#define LSR_VISIBILITY_MAX_%s %d\b" % (name, value), hdr)
    assert C.sizeof(_capi.VisibilityParams) == 80
    d = VisibilityParams()
    assert (d.face_width, d.height, d.min_range, d.max_range, d.margin, d.keyframe_range, d.max_neighbours, d.min_votes) == \
        (128, 32, 0.5, 80.0, 0.5, 30.0, 32, 2)
    assert d.max_tan_elevation == math.tan(math.radians(30.0)) and tuple(d.sensor_origin) == (0.0, 0.0, 0.0)
    s = d.struct()
    assert (s.face_width, s.height, s.max_neighbours, s.min_votes, s.max_tan_elevation) == (128, 32, 32, 2, d.max_tan_elevation)
    # the library exports exactly the names the header declares
    import subprocess

    declared = sorted(set(re.findall(r"\b(lsr_[a-z0-9_]+)\s*\(", hdr)))
    nm = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(set(re.findall(r"\sT\s+([A-Za-z][A-Za-z0-9_]*)$", nm, re.M))) == declared
    assert sorted(_capi.EXPORTED_SYMBOLS) == declared
    mk = open(os.path.join(ROOT, "lidarslam_ros2_amd", "csrc", "Makefile")).read()
    assert re.search(r"^map_visibility\.o: CXXFLAGS \+= -ffp-contract=off$", mk, re.M) and "map_visibility.o" in mk.split("OBJS =")[1].split("\n")[0]


# ---- the behaviour of the definition -------------------------------------------------------------------------------------------------------
def test_the_car_goes_and_the_world_stays():
    """Measured with the exact definition at the defaults: 0 of 208 671 records that stand still removed, 352 of 488 car records (72 %)
    removed; the same drive without the car: 0 of 209 505 removed.  (min_votes = 1: 9 static, 394 car, 8 in the empty scene.)"""
    p = MV.params()
    with_car, without = MV.car_scene(True), MV.car_scene(False)
    v1, _ = MV.static_votes(with_car["clouds"], with_car["ma"].submaps, p)
    v0, _ = MV.static_votes(without["clouds"], without["ma"].submaps, p)
    assert v1.size == with_car["is_car"].size
    MV.assert_behaviour(MV.behaviour(v1, v0, p.min_votes))


def test_the_erosion_is_what_keeps_the_ground():
    """Without step 3 the same settings take the ground at grazing incidence: far above the cap.  Measured on the restatement: 34 238
    of 208 671 records that stand still (16.4 %) removed, 436 of the 488 car records."""
    p = MV.params()
    scene = MV.car_scene(True)
    from lidarslam_ros2_amd import visibilityPairs

    first, other, rel = visibilityPairs(scene["ma"].submaps, None, p)
    D = MV.images(scene["clouds"], p, eroded=False)
    v = MV.votes(scene["clouds"], first, other, rel, D, p)
    car = scene["is_car"]
    assert ((v >= p.min_votes) & ~car).sum() > 0.05 * (~car).sum()


def test_cpp_snippet_compiles_and_links(tmp_path):
    """the block of tests/cpp/map_visibility_snippets.cpp, compiled against include/lidarslam_reg/map_visibility.hpp
    and linked against the library; the program runs the pair table and the refusals that need no device."""
    import subprocess
    import textwrap

    src = os.path.join(ROOT, "tests", "cpp", "map_visibility_snippets.cpp")
    libdir = os.path.join(ROOT, "lidarslam_ros2_amd")
    exe = str(tmp_path / "map_visibility_snippets")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir,
                           "-llidarslam_reg", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert run.returncode == 0 and "MAP_VISIBILITY_SNIPPETS ok=1 refused=3" in run.stdout, (run.stdout, run.stderr)
    text, doc = open(src).read(), open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc.split("### 3m.")[1]
    block = text.split("// [map-visibility-snippet begin: static_map]\n")[1].split("  // [map-visibility-snippet end: static_map]")[0]
    assert textwrap.dedent(block).strip("\n").rstrip() in textwrap.dedent(section.split("```cpp\n")[1].split("```")[0])

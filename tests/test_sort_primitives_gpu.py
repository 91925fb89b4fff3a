"""The primitives of csrc/lsd_sort.hip, each alone on the device against its plain restatement (sort_numpy.py), on every case of
sort_cases.py: the stable LSD radix sort in its four scatter forms, one to three passes and 1- to 11-bit digits; the exclusive scan in
its single-block and three-launch forms, aligned and not; the runs of equal keys (table, float centroid, both run counts).

Every comparison is EXACT: integers for the sort, the scan and the tables, bit patterns for the centroids (a chain of float32 additions
in ascending position and one correctly rounded division: nothing to round differently).  Stability has no assertion of its own: the
values must equal the stable argsort's.  test_sort_primitives_cpu.py holds the restatements and the case list to their definitions."""
import ctypes as C

import numpy as np
import pytest

import sort_cases as K
import sort_numpy as SN

pytestmark = pytest.mark.gpu
UP, IP, FP = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float)
CANARY_U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def handle():
    from lidarslam_ros2_amd import _capi

    lib = _capi.load()
    h = C.c_void_p()
    _capi.check(lib.lsr_create(_capi.METHOD_NDT, 0, None, C.byref(h)), "lsr_create")
    yield lib, h
    lib.lsr_destroy(h)


def _groups(cases, key):
    out = {}
    for c in cases:
        out.setdefault(key(c), []).append(c)
    return out


# ---- the entries on numpy arrays -----------------------------------------------------------------------------------------------
def dev_sort(handle, keys, vals, end_bit, alias):
    from lidarslam_ros2_amd import _capi

    lib, h = handle
    n = len(keys)
    keys = np.ascontiguousarray(keys, np.uint32)
    vals = None if vals is None else np.ascontiguousarray(vals, np.int32)
    k_out, v_out, in_b = np.full(n, 0xABABABAB, np.uint32), np.full(n, -7, np.int32), C.c_int(-1)
    _capi.check(lib.lsr_debug_sort_pairs_u32(h, keys.ctypes.data_as(UP), None if vals is None else vals.ctypes.data_as(IP), n, end_bit,
                                             1 if alias else 0, k_out.ctypes.data_as(UP), v_out.ctypes.data_as(IP), C.byref(in_b)),
                "lsr_debug_sort_pairs_u32")
    return k_out, v_out, in_b.value


def dev_scan(handle, a, in_shift=0, out_shift=0):
    from lidarslam_ros2_amd import _capi

    lib, h = handle
    a = np.ascontiguousarray(a, np.int32)
    out = np.full(len(a), -7, np.int32)
    _capi.check(lib.lsr_debug_exclusive_scan_i32(h, a.ctypes.data_as(IP), len(a), in_shift, out_shift, out.ctypes.data_as(IP)),
                "lsr_debug_exclusive_scan_i32")
    return out


def dev_runs(handle, keys, order, planes, sentinel, sentinel_on_device):
    from lidarslam_ros2_amd import _capi

    lib, h = handle
    n = len(keys)
    keys, order = np.ascontiguousarray(keys, np.uint32), np.ascontiguousarray(order, np.int32)
    planes = [np.ascontiguousarray(p, np.float32) for p in planes]
    run_key, run_off = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.int32)
    cent = [np.zeros(n, np.float32) for _ in planes]
    n_runs, n_runs_dev = C.c_int(-1), C.c_int(-1)
    fp = [p.ctypes.data_as(FP) for p in planes] + [None] * (4 - len(planes))
    cp = [c.ctypes.data_as(FP) for c in cent] + [None] * (4 - len(planes))
    _capi.check(lib.lsr_debug_sorted_runs(h, keys.ctypes.data_as(UP), order.ctypes.data_as(IP), n, fp[0], fp[1], fp[2], fp[3], int(sentinel),
                                          1 if sentinel_on_device else 0, run_key.ctypes.data_as(UP), run_off.ctypes.data_as(IP),
                                          cp[0], cp[1], cp[2], cp[3], C.byref(n_runs), C.byref(n_runs_dev)), "lsr_debug_sorted_runs")
    return run_key, run_off, cent, n_runs.value, n_runs_dev.value


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_sort(handle, key_set, n, end_bit, mode):
    keys, vals = K.sort_keys(key_set, n, end_bit), K.sort_values(mode, n)
    want_k, want_v = SN.sort_pairs(keys, vals, end_bit)
    got_k, got_v, in_b = dev_sort(handle, keys, vals, end_bit, mode == "aliased")
    where = (key_set, n, end_bit, mode)
    bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
    assert len(bad) == 0, (where, f"{len(bad)} positions differ, the first at {bad[0]}: key {got_k[bad[0]]:#x} value {got_v[bad[0]]}, "
                                  f"expected {want_k[bad[0]]:#x} / {want_v[bad[0]]}")
    assert in_b == SN.plan(n, end_bit)["passes"] % 2, where


def check_scan(handle, data, n, in_shift, out_shift):
    a = K.scan_data(data, n)
    got, want = dev_scan(handle, a, in_shift, out_shift), SN.exclusive_scan(a)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, ((data, n, in_shift, out_shift), f"{len(bad)} differ, the first at {bad[0]}: {got[bad[0]]}, expected {want[bad[0]]}")


def check_runs(handle, layout, n, sentinel_run, sentinel_on_device, with_w):
    from lidarslam_ros2_amd import _capi

    where = (layout, n, sentinel_run, sentinel_on_device, with_w)
    keys, order, planes, sentinel = K.run_input(layout, n, sentinel_run, with_w)
    want_key, want_off = SN.run_table(keys)
    nr = len(want_key)
    run_key, run_off, cent, n_runs, n_runs_dev = dev_runs(handle, keys, order, planes, sentinel, sentinel_on_device)
    assert n_runs == nr and n_runs_dev == nr, where                        # the mailbox's count and the one left in device memory
    assert np.array_equal(run_key[:nr], want_key) and np.array_equal(run_off[:nr + 1], want_off), where
    assert run_off[nr] == n, where
    assert np.all(run_key[nr:] == CANARY_U32) and np.all(run_off[nr + 1:].view(np.uint32) == CANARY_U32), where   # nothing past the table
    kept = nr - 1 if sentinel_run else nr                                  # the sentinel's run is the last and gets no centroid
    want_cent = SN.run_centroids(want_off, order, planes)
    assert len(cent) == (4 if with_w else 3)
    for k, (got, want) in enumerate(zip(cent, want_cent)):
        bad = np.flatnonzero(SN.bits_of(got[:kept]) != SN.bits_of(want[:kept]))
        assert len(bad) == 0, (where, k, f"{len(bad)} centroids differ, the first in run {bad[0]}: {got[bad[0]]!r}, expected {want[bad[0]]!r}")
        assert np.all(SN.bits_of(got[kept:]) == _capi.DEBUG_CANARY_F32_BITS), (where, k)


SORT_GROUPS = _groups(K.sort_cases(), lambda c: (c[0], c[1]))
SCAN_GROUPS = _groups(K.scan_cases(), lambda c: c[1])
RUN_GROUPS = _groups(K.run_cases(), lambda c: (c[0], c[1]))


@pytest.mark.parametrize("key_set,n", sorted(SORT_GROUPS), ids=lambda v: str(v))
def test_sort_equals_the_stable_argsort(handle, key_set, n):
    for case in SORT_GROUPS[(key_set, n)]:
        check_sort(handle, *case)


@pytest.mark.parametrize("n", sorted(SCAN_GROUPS))
def test_scan_equals_the_cumulative_sum(handle, n):
    for case in SCAN_GROUPS[n]:
        check_scan(handle, *case)


@pytest.mark.parametrize("layout,n", sorted(RUN_GROUPS), ids=lambda v: str(v))
def test_runs_table_counts_and_centroids(handle, layout, n):
    for case in RUN_GROUPS[(layout, n)]:
        check_runs(handle, *case)


def test_large_then_small_on_one_object(handle):
    """each entry twice on the same object, a large input and then a small one: the second answer stands on nothing the first left"""
    check_sort(handle, "uniform", 1048577, 32, "given")
    check_sort(handle, "uniform", 4097, 22, "given")
    check_sort(handle, "descending", 65, 12, "iota")
    check_scan(handle, "random_0_9", 4096 * 1024 + 1, 0, 0)
    check_scan(handle, "random_0_9", 8193, 0, 0)
    check_scan(handle, "ones", 17, 0, 0)
    check_runs(handle, "random_1_9", 262145, True, True, True)
    check_runs(handle, "random_1_9", 257, True, False, True)
    check_runs(handle, "distinct", 1, False, False, False)


def test_entries_leave_the_object_as_they_found_it():
    """an align() on a small scene before and after a burst of the three entries on the SAME object, and with the burst between
    setInputSource and align: the same bits every time (the entries use the object's device and stream, and nothing else of it)"""
    from lidarslam_ros2_amd import DIRECT7, NormalDistributionsTransform, synth

    case = synth.small_case(n_source=4000, n_keyframes=3)
    ndt = NormalDistributionsTransform(device=0)
    ndt.setResolution(3.0)
    ndt.setTransformationEpsilon(0.01)
    ndt.setNeighborhoodSearchMethod(DIRECT7)
    hd = (ndt._lib, ndt._h)

    def burst():
        check_sort(hd, "uniform", 4097, 23, "given")
        check_sort(hd, "four_blocks_of_64", 524289, 22, "aliased")
        check_scan(hd, "mixed_signs", 8193, 2, 1)
        check_runs(hd, "random_1_9", 257, True, True, True)
        check_runs(hd, "across_seams", 262145, True, False, False)

    def align():
        ndt.align(case.guess)
        return np.array(ndt.getFinalTransformation()), ndt.getFinalNumIteration(), ndt.voxelGridFilter(case.source, 0.5)

    ndt.setInputTarget(synth.as_pointxyzi(case.target))
    ndt.setInputSource(synth.as_pointxyzi(case.source))
    T0, it0, vg0 = align()
    burst()
    T1, it1, vg1 = align()
    ndt.setInputTarget(synth.as_pointxyzi(case.target))
    burst()
    ndt.setInputSource(synth.as_pointxyzi(case.source))
    burst()
    T2, it2, vg2 = align()
    assert ndt.hasConverged() and it0 == it1 == it2
    for T, vg in ((T1, vg1), (T2, vg2)):
        assert T.tobytes() == T0.tobytes() and vg.tobytes() == vg0.tobytes() and len(vg0) > 100


def test_entries_check_their_arguments_with_a_live_object(handle):
    """bad arguments with a live object: LSR_ERR_INVALID_ARGUMENT and nothing written (test_sort_primitives_cpu.py: every argument,
    null handle)"""
    from lidarslam_ros2_amd import _capi

    lib, h = handle
    big = _capi.DEBUG_SORT_MAX + 1
    u, i, f = np.full(16, 7, np.uint32), np.full(16, 7, np.int32), np.full(16, 7, np.float32)
    pu, pi, pf = u.ctypes.data_as(UP), i.ctypes.data_as(IP), f.ctypes.data_as(FP)
    flag, flag2 = C.c_int(-7), C.c_int(-7)
    for n, eb, al, vals in ((0, 12, 0, pi), (big, 12, 0, pi), (8, 0, 0, pi), (8, 33, 0, pi), (8, 12, 1, None)):
        assert lib.lsr_debug_sort_pairs_u32(h, pu, vals, n, eb, al, pu, pi, C.byref(flag)) == -1
    assert lib.lsr_debug_sort_pairs_u32(h, None, pi, 8, 12, 0, pu, pi, C.byref(flag)) == -1
    assert lib.lsr_debug_sort_pairs_u32(h, pu, pi, 8, 12, 0, pu, pi, None) == -1
    for n, a, b in ((0, 0, 0), (big, 0, 0), (8, 4, 0), (8, 0, -1)):
        assert lib.lsr_debug_exclusive_scan_i32(h, pi, n, a, b, pi) == -1
    assert lib.lsr_debug_exclusive_scan_i32(h, None, 8, 0, 0, pi) == -1
    order = np.arange(16, dtype=np.int32)
    po = order.ctypes.data_as(IP)
    good = [pu, po, 8, pf, pf, pf, pf, 99, 0, pu, pi, pf, pf, pf, pf, C.byref(flag), C.byref(flag2)]
    for k, v in ((2, 0), (2, big), (0, None), (6, None), (14, None), (15, None), (16, None)):
        bad = list(good)
        bad[k] = v
        assert lib.lsr_debug_sorted_runs(h, *bad) == -1
    order[3] = 8
    assert lib.lsr_debug_sorted_runs(h, *good) == -1
    assert flag.value == -7 and flag2.value == -7 and np.all(u == 7) and np.all(i == 7) and np.all(f == 7)

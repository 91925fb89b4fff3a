"""The sort / scan / run-table tests' own ground, checked without a GPU: the restatements of sort_numpy.py against brute-force
definitions, lsr_debug_lsd_plan (the library's plan, host only) against the restated plan, a guard that the case list of
sort_cases.py still reaches every launch form csrc/lsd_sort.hip has, and the argument checks of the three device entries with a null
handle.  test_sort_primitives_gpu.py runs the same cases on the device."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import sort_cases as K
import sort_numpy as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP, IP, FP, CIP = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib():
    from lidarslam_ros2_amd import _capi

    L = _capi.load()
    L.lsr_last_error.restype = C.c_char_p
    return L


def _lib_plan(lib, n, end_bit):
    out = (C.c_int * 11)(*([-1] * 11))
    assert lib.lsr_debug_lsd_plan(n, end_bit, out) == 0
    return list(out)


# ---- the restatements against brute-force definitions ----------------------------------------------------------------------------
@pytest.mark.parametrize("key_set", K.KEY_SETS + ("stray",))
def test_sort_restatement_is_a_stable_sort_on_the_covered_bits(key_set):
    for n, eb in ((1, 23), (65, 23), (700, 23)) if key_set == "stray" else ((1, 5), (65, 5), (700, 12), (700, 32)):
        keys, vals = K.sort_keys(key_set, n, eb), K.sort_values("given", n)
        m = (1 << SN.plan(n, eb)["covered_bits"]) - 1
        want = sorted(zip(keys.tolist(), vals.tolist()), key=lambda kv: kv[0] & m)      # Python's sort is stable
        k, v = SN.sort_pairs(keys, vals, eb)
        assert list(zip(k.tolist(), v.tolist())) == want
        k, v = SN.sort_pairs(keys, None, eb)
        assert list(zip(k.tolist(), v.tolist())) == sorted(zip(keys.tolist(), range(n)), key=lambda kv: kv[0] & m)
        assert key_set == "stray" or int(keys.max()) < 1 << eb


def test_stray_keys_are_ordered_by_bit_23_and_keep_their_high_byte():
    keys = K.sort_keys("stray", 4097, 23)
    assert (keys >> 23 & 1).any() and (keys >> 24).any() and SN.plan(4097, 23)["covered_bits"] == 24
    k, _v = SN.sort_pairs(keys, None, 23)
    assert np.all(np.diff((k & 0xFFFFFF).astype(np.int64)) >= 0) and np.any(np.diff(k.astype(np.int64)) < 0)
    assert not np.array_equal(k, keys[np.argsort(keys & SN.mask(23), kind="stable")])     # "bits [0, end_bit)" would be another order


def test_scan_restatement():
    for data in K.SCAN_DATA:
        a = K.scan_data(data, 9000)
        run, want = 0, []
        for x in a.tolist():
            want.append(run)
            run += x
        assert SN.exclusive_scan(a).tolist() == want
    for data, off in (("seam_minus_1", -1), ("seam", 0), ("seam_plus_1", 1)):
        assert np.flatnonzero(K.scan_data(data, 9000)).tolist() == [p for p in (off, 4096 + off, 8192 + off) if p >= 0]


@pytest.mark.parametrize("layout", K.RUN_LAYOUTS)
def test_run_restatements_against_groupby_and_an_explicit_float32_loop(layout):
    for n, sentinel_run in ((1, False), (257, True), (1500, False), (1500, True)):
        keys, order, planes, sentinel = K.run_input(layout, n, sentinel_run, True)
        assert sorted(order.tolist()) == list(range(n)) and (n < 3 or not np.array_equal(order, np.arange(n)))
        assert np.all(np.diff(keys.astype(np.int64)) >= 0) and ((keys[-1] == sentinel) == sentinel_run) and not (keys[:-1] > sentinel).any()
        groups = [(k, len(list(g))) for k, g in itertools.groupby(keys.tolist())]
        run_key, run_off = SN.run_table(keys)
        assert run_key.tolist() == [k for k, _c in groups]
        assert run_off.tolist() == [0] + list(itertools.accumulate(c for _k, c in groups)) and run_off.dtype == np.int32
        for long_run in (64, 4):       # both ways the restatement sums a run
            cent = SN.run_centroids(run_off, order, planes, long_run=long_run)
            for plane, got in zip(planes, cent):
                for r, (_k, c) in enumerate(groups):
                    s = np.float32(0.0)
                    for j in range(run_off[r], run_off[r] + c):
                        s = np.float32(s + plane[order[j]])
                    assert np.float32(s / np.float32(c)).view(np.uint32) == got[r].view(np.uint32), (layout, n, r)
        for plane in planes:
            mag = np.abs(plane)
            assert 1e-3 <= mag.min() and mag.max() <= 1e3 and (n < 257 or mag.max() / mag.min() > 1e4)


def test_layouts_put_runs_where_they_say():
    lens = K.run_lengths("across_seams", 2000, None)
    heads = np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert all(any(h < s <= h + c - 1 for h, c in zip(heads, lens)) for s in range(256, 2000, 256))   # a run lies across every seam
    lens = K.run_lengths("long_700", 2000, None)
    heads = set(np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist())
    assert any(not (heads & set(range(b, b + 256))) for b in range(0, 1792, 256))                     # a whole block without a head


def test_the_order_of_the_float_additions_shows_in_the_bits():
    """what makes the centroid comparison a test of the ORDER: on these points another order of the same additions gives other bits"""
    keys, order, planes, _s = K.run_input("random_1_9", 1500, False, False)
    _rk, run_off = SN.run_table(keys)
    fwd = SN.run_centroids(run_off, order, planes)
    rev_order = order.copy()
    for a, b in zip(run_off[:-1], run_off[1:]):
        rev_order[a:b] = order[a:b][::-1]
    rev = SN.run_centroids(run_off, rev_order, planes)
    assert sum(int((SN.bits_of(f) != SN.bits_of(r)).sum()) for f, r in zip(fwd, rev)) > 100


# ---- the library's plan against the restated one, and what the case list reaches -------------------------------------------------
def test_plan_entry_equals_the_restated_plan(lib):
    pairs = {(n, eb) for _ks, n, eb, _vm in K.sort_cases()}
    pairs |= {(n, 32) for _d, n, _a, _b in K.scan_cases()} | {(n, 32) for _l, n, *_ in K.run_cases()}
    for edge in (64, 512, 2048, 4096, 524288, 600000, 1048576, 4096 * 1024, 4096 * 2048, 262144, 1 << 24):
        pairs |= {(n, eb) for n in (edge - 1, edge, edge + 1) if n <= 1 << 24 for eb in (1, 11, 12, 22, 23, 32)}
    for n, eb in sorted(pairs):
        assert _lib_plan(lib, n, eb) == SN.plan_words(n, eb), (n, eb)
    p = dict(zip(SN.PLAN_FIELDS, _lib_plan(lib, 147443, 23)))
    assert (p["passes"], p["bits"], p["covered_bits"], p["steps"], p["nblk"], p["fused"]) == (3, 8, 24, 8, 72, 1)
    for eb in range(1, 33):
        p = SN.plan(1000, eb)
        assert eb <= p["covered_bits"] <= 33 and 1 <= p["bits"] <= 11 and p["passes"] == -(-eb // 11)


def test_case_list_reaches_every_form():
    """If a threshold of lsd_plan, of the scan or of the run scan moves, the form that lost its case is named here.  The forms are read
    from the LIBRARY's plan, not from the restatement."""
    from lidarslam_ros2_amd import _capi

    L = _capi.load()
    plans = [dict(zip(SN.PLAN_FIELDS, _lib_plan(L, n, eb)), n=n, key_set=ks, values=vm) for ks, n, eb, vm in K.sort_cases()]
    missing = []
    for steps in (8, 16):
        for fused in (1, 0):
            for ks in K.KEY_SETS + ("stray",):
                if not any(p["steps"] == steps and p["fused"] == fused and p["key_set"] == ks for p in plans):
                    missing.append(f"scatter steps {steps} fused {fused} on key set {ks}")
            for vm in K.VALUE_MODES:
                if not any(p["steps"] == steps and p["fused"] == fused and p["values"] == vm for p in plans):
                    missing.append(f"scatter steps {steps} fused {fused} with {vm} values")
    missing += [f"{k} passes" for k in (1, 2, 3) if not any(p["passes"] == k for p in plans)]
    missing += [f"{b}-bit digits" for b in range(1, 12) if not any(p["bits"] == b for p in plans)]
    missing += [f"result_in_b {r}" for r in (0, 1) if not any(p["passes"] % 2 == r for p in plans)]
    missing += [f"more than one workgroup with {k} passes" for k in (1, 2, 3) if not any(p["passes"] == k and p["nblk"] > 1 for p in plans)]
    scans = [dict(zip(SN.PLAN_FIELDS, _lib_plan(L, n, 32)), shifted=bool(a or b)) for _d, n, a, b in K.scan_cases()]
    missing += ["single-block scan"] if not any(s["scan_single_block"] for s in scans) else []
    missing += [f"three-launch scan, {k} sums per thread" for k in (1, 2, 3) if not any(not s["scan_single_block"] and s["scan_per"] == k for s in scans)]
    missing += ["misaligned three-launch scan"] if not any(s["shifted"] and not s["scan_single_block"] for s in scans) else []
    runs = [dict(zip(SN.PLAN_FIELDS, _lib_plan(L, n, 32))) for _l, n, *_ in K.run_cases()]
    missing += [f"run scan, {k} counts per thread" for k in (1, 2) if not any(r["run_per"] == k for r in runs)]
    for lay in K.RUN_LAYOUTS:
        seen = {(s, d, w) for l, _n, s, d, w in K.run_cases() if l == lay}
        missing += [f"runs {lay}: sentinel run {s}, on device {d}, w {w}" for s in (0, 1) for d in (0, 1) for w in (0, 1) if (s, d, w) not in seen]
    assert not missing, missing
    # each size sits on its side of its threshold
    assert {(p["steps"], p["fused"]) for p in plans if p["n"] in (524288, 600001, 1048576)} == {(8, 1), (16, 1)}
    assert {(p["steps"], p["fused"]) for p in plans if p["n"] in (524289, 600000)} == {(8, 0)}
    assert {(p["steps"], p["fused"]) for p in plans if p["n"] == 1048577} == {(16, 0)}


# ---- the entries: declared, bound, and refusing bad arguments before they look at the handle -------------------------------------
def test_entries_are_declared_and_bound(lib):
    from lidarslam_ros2_amd import _capi

    hdr = open(os.path.join(ROOT, "include", "lidarslam_reg.h")).read()
    for name in ("lsr_debug_lsd_plan", "lsr_debug_sort_pairs_u32", "lsr_debug_exclusive_scan_i32", "lsr_debug_sorted_runs"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert hasattr(lib, name) and name in _capi.EXPORTED_SYMBOLS and decl
        assert len(getattr(lib, name).argtypes) == decl.group(1).count(",") + 1 and getattr(lib, name).restype is C.c_int
    assert eval(re.search(r"#define LSR_DEBUG_SORT_MAX \((.*)\)", hdr).group(1)) == _capi.DEBUG_SORT_MAX == 1 << 24
    assert int(re.search(r"#define LSR_DEBUG_LSD_PLAN_WORDS (\d+)", hdr).group(1)) == _capi.DEBUG_LSD_PLAN_WORDS == len(SN.PLAN_FIELDS)
    assert int(re.search(r"#define LSR_DEBUG_CANARY_F32_BITS (\w+)u", hdr).group(1), 16) == _capi.DEBUG_CANARY_F32_BITS
    assert np.isnan(np.uint32(_capi.DEBUG_CANARY_F32_BITS).view(np.float32))


def test_entries_refuse_bad_arguments_before_the_handle(lib):
    from lidarslam_ros2_amd import _capi

    big = _capi.DEBUG_SORT_MAX + 1
    out = (C.c_int * 11)(*([-7] * 11))
    for n, eb in ((0, 8), (big, 8), (5, 0), (5, 33), (5, -1)):
        assert lib.lsr_debug_lsd_plan(n, eb, out) == -1
    assert lib.lsr_debug_lsd_plan(5, 8, None) == -1 and list(out) == [-7] * 11

    def refused(status):
        assert status == -1 and b"null handle" not in lib.lsr_last_error()

    u, i, f = np.full(16, 7, np.uint32), np.full(16, 7, np.int32), np.full(16, 7, np.float32)
    pu, pi, pf = u.ctypes.data_as(UP), i.ctypes.data_as(IP), f.ctypes.data_as(FP)
    flag, flag2 = C.c_int(-7), C.c_int(-7)
    # a null handle with good arguments is refused as a null handle; with every bad argument in turn, as that argument
    assert lib.lsr_debug_sort_pairs_u32(None, pu, pi, 8, 12, 1, pu, pi, C.byref(flag)) == -1 and b"null handle" in lib.lsr_last_error()
    assert lib.lsr_debug_sort_pairs_u32(None, pu, None, 8, 12, 0, pu, pi, C.byref(flag)) == -1 and b"null handle" in lib.lsr_last_error()
    refused(lib.lsr_debug_sort_pairs_u32(None, None, pi, 8, 12, 0, pu, pi, C.byref(flag)))
    refused(lib.lsr_debug_sort_pairs_u32(None, pu, pi, 8, 12, 0, None, pi, C.byref(flag)))
    refused(lib.lsr_debug_sort_pairs_u32(None, pu, pi, 8, 12, 0, pu, None, C.byref(flag)))
    refused(lib.lsr_debug_sort_pairs_u32(None, pu, pi, 8, 12, 0, pu, pi, None))
    refused(lib.lsr_debug_sort_pairs_u32(None, pu, None, 8, 12, 1, pu, pi, C.byref(flag)))      # nothing to alias
    for n, eb in ((0, 12), (big, 12), (8, 0), (8, 33), (8, -3)):
        refused(lib.lsr_debug_sort_pairs_u32(None, pu, pi, n, eb, 0, pu, pi, C.byref(flag)))

    assert lib.lsr_debug_exclusive_scan_i32(None, pi, 8, 0, 3, pi) == -1 and b"null handle" in lib.lsr_last_error()
    refused(lib.lsr_debug_exclusive_scan_i32(None, None, 8, 0, 0, pi))
    refused(lib.lsr_debug_exclusive_scan_i32(None, pi, 8, 0, 0, None))
    for n, a, b in ((0, 0, 0), (big, 0, 0), (8, -1, 0), (8, 4, 0), (8, 0, -1), (8, 0, 4)):
        refused(lib.lsr_debug_exclusive_scan_i32(None, pi, n, a, b, pi))

    order = np.arange(16, dtype=np.int32)
    po = order.ctypes.data_as(IP)
    good = [pu, po, 8, pf, pf, pf, pf, 99, 0, pu, pi, pf, pf, pf, pf, C.byref(flag), C.byref(flag2)]
    assert lib.lsr_debug_sorted_runs(None, *good) == -1 and b"null handle" in lib.lsr_last_error()
    no_w = list(good)
    no_w[6] = no_w[14] = None
    assert lib.lsr_debug_sorted_runs(None, *no_w) == -1 and b"null handle" in lib.lsr_last_error()
    for k in (0, 1, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16):       # every pointer; w without cw and cw without w are among them
        bad = list(good)
        bad[k] = None
        refused(lib.lsr_debug_sorted_runs(None, *bad))
    for n in (0, big):
        bad = list(good)
        bad[2] = n
        refused(lib.lsr_debug_sorted_runs(None, *bad))
    for wrong in (-1, 8):                                              # the centroid kernel would gather outside the planes
        order[5] = wrong
        refused(lib.lsr_debug_sorted_runs(None, *good))
        order[5] = 5
    assert flag.value == -7 and flag2.value == -7 and np.all(u == 7) and np.all(i == 7) and np.all(f == 7) and np.array_equal(order, np.arange(16))

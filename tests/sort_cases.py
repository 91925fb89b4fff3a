"""The cases of the sort / scan / run-table tests, one list for test_sort_primitives_cpu.py (plan, coverage guard) and
test_sort_primitives_gpu.py (the device).  Every case is a small tuple of names and numbers; its data is generated on demand from a
seed derived from the tuple, so both files see the same arrays.

Sizes sit on both sides of every threshold csrc/lsd_sort.hip hard-codes: the wave step (64), a small workgroup's share (512), the
2048- and 4096-key workgroups, the four scatter forms (steps 8 fused up to 524288 keys, steps 8 unfused up to 600000, steps 16 fused
up to 1048576, steps 16 unfused above), the 4096-element scan block, one, two and three block sums per thread of the scan's middle
launch (4096 * 1024 and 4096 * 2048 elements), the 256-key run block and two block counts per thread of the run scan (262144 keys)."""
import zlib

import numpy as np

import sort_numpy as SN

SORT_SMALL_N = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4096, 4097)
SORT_LARGE_N = (524288, 524289, 600000, 600001, 1048576, 1048577)
SORT_LARGE_END_BITS = (1, 11, 12, 22, 23, 32)
SORT_ADVERSARIAL_N = (4097, 524289, 600001, 1048577)   # the smallest sizes that reach each scatter form with more than one workgroup
SORT_ADVERSARIAL_END_BITS = (5, 22, 32)           # one, two and three passes; 5- and 11-bit digits
KEY_SETS = ("uniform", "equal_zero", "equal_max", "alternating", "four_blocks_of_64", "ascending", "descending", "lane_distinct",
            "top_digit_only", "bit0_only")
STRAY_END_BIT = 23                                # three passes of 8 bits cover 24: bit 23 is ordered, bits 24..31 are carried
VALUE_MODES = ("iota", "given", "aliased")

SCAN_N = (1, 15, 16, 17, 4095, 4096, 4097, 8192, 8193, 4096 * 1024, 4096 * 1024 + 1, 4096 * 2048 + 5)
SCAN_DATA = ("zeros", "ones", "random_0_9", "mixed_signs", "seam_minus_1", "seam", "seam_plus_1")
SCAN_SHIFTS = ((0, 0), (1, 0), (0, 3), (2, 1))
SCAN_SHIFT_N = (4097, 8193, 4096 * 1024 + 1)

RUN_SMALL_N = (1, 255, 256, 257)
RUN_LARGE_N = (262144, 262145, 600001)
RUN_LAYOUTS = ("distinct", "equal", "random_1_9", "across_seams", "long_700")


def _rng(*parts):
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


# ---- sort ------------------------------------------------------------------------------------------------------------------
def sort_cases():
    """(key set, n, end_bit, value mode); the value mode rotates so that every key set and size meets all three"""
    out = []
    for n in SORT_SMALL_N:
        for eb in range(1, 33):
            out.append(("uniform", n, eb, VALUE_MODES[(eb + n) % 3]))
    for k, n in enumerate(SORT_LARGE_N):
        for j, eb in enumerate(SORT_LARGE_END_BITS):
            out.append(("uniform", n, eb, VALUE_MODES[(k + j) % 3]))
    for s, ks in enumerate(KEY_SETS[1:]):
        for k, n in enumerate(SORT_ADVERSARIAL_N):
            for j, eb in enumerate(SORT_ADVERSARIAL_END_BITS):
                out.append((ks, n, eb, VALUE_MODES[(s + k + j) % 3]))
    for k, n in enumerate(SORT_ADVERSARIAL_N):
        out.append(("stray", n, STRAY_END_BIT, VALUE_MODES[k % 3]))
    return out


def sort_keys(key_set, n, end_bit):
    """uint32 keys below 2^end_bit (the stray set excepted)"""
    rng = _rng("keys", key_set, n, end_bit)
    top = (1 << end_bit) - 1
    p = SN.plan(n, end_bit)
    i = np.arange(n, dtype=np.uint64)
    if key_set == "uniform":
        k = rng.integers(0, top + 1, n, dtype=np.uint64)
    elif key_set == "equal_zero":
        k = np.zeros(n, np.uint64)
    elif key_set == "equal_max":
        k = np.full(n, top, np.uint64)              # 0xFFFFFFFF at end_bit 32
    elif key_set == "alternating":
        k = np.where(i % 2 == 0, top, top // 3).astype(np.uint64)
    elif key_set == "four_blocks_of_64":
        k = np.array([top, 0, top // 2, top // 3], np.uint64)[(i // 64) % 4]
    elif key_set in ("ascending", "descending"):
        k = i if n <= top + 1 else (i * np.uint64(top + 1)) // np.uint64(n)
        k = k[::-1] if key_set == "descending" else k
    elif key_set == "lane_distinct":                # digit i mod 2^bits in EVERY pass: the 64 lanes of a step hold different digits
        d = i % np.uint64(1 << p["bits"])
        k = np.zeros(n, np.uint64)
        for q in range(p["passes"]):
            k |= d << np.uint64(q * p["bits"])
        k &= np.uint64(top)
    elif key_set == "top_digit_only":               # every pass but the last sees ONE digit; the last must keep what they left
        shift = (p["passes"] - 1) * p["bits"]
        k = (rng.integers(0, 1 << (end_bit - shift), n, dtype=np.uint64) << np.uint64(shift)) | np.uint64(0x2A5A5A5A & ((1 << shift) - 1))
    elif key_set == "bit0_only":
        k = np.uint64(top & ~1) | rng.integers(0, 2, n, dtype=np.uint64)
    elif key_set == "stray":                        # end_bit 23: bit 23 set on half the keys, bits 24..31 anything
        assert end_bit == STRAY_END_BIT and p["covered_bits"] == 24
        k = rng.integers(0, 1 << 23, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(23)) | \
            (rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(24))
    else:
        raise KeyError(key_set)
    k = np.ascontiguousarray(k, np.uint64)
    assert k.max() <= (0xFFFFFFFF if key_set == "stray" else top)
    return k.astype(np.uint32)


def sort_values(mode, n):
    """None for iota; else int32 values with negatives and duplicates"""
    if mode == "iota":
        return None
    return _rng("vals", n).integers(-max(2, n // 3), max(2, n // 3), n).astype(np.int32)


# ---- scan ------------------------------------------------------------------------------------------------------------------
def scan_cases():
    """(data, n, in_shift, out_shift)"""
    out = [(d, n, 0, 0) for n in SCAN_N for d in SCAN_DATA]
    out += [(d, n, a, b) for n in SCAN_SHIFT_N for (a, b) in SCAN_SHIFTS[1:] for d in ("random_0_9", "mixed_signs")]
    return out


def scan_data(data, n):
    rng = _rng("scan", data, n)
    if data == "zeros":
        a = np.zeros(n, np.int32)
    elif data == "ones":
        a = np.ones(n, np.int32)
    elif data == "random_0_9":
        a = rng.integers(0, 10, n).astype(np.int32)
    elif data == "mixed_signs":
        a = rng.integers(-1000, 1001, n).astype(np.int32)
        assert np.abs(np.cumsum(a, dtype=np.int64)).max() < 2 ** 31
    elif data.startswith("seam"):                   # a 1 beside every 4096-element block seam: an exclusive prefix off by one element shows
        off = {"seam_minus_1": -1, "seam": 0, "seam_plus_1": 1}[data]
        a = np.zeros(n, np.int32)
        pos = np.arange(0, n + SN.XS_CHUNK, SN.XS_CHUNK) + off
        a[pos[(pos >= 0) & (pos < n)]] = 1
    else:
        raise KeyError(data)
    return a


# ---- runs ------------------------------------------------------------------------------------------------------------------
def run_cases():
    """(layout, n, sentinel run at the end, sentinel on the device, w plane).  The small sizes take all eight settings; the large ones
    one each, rotating, so that no size is paid for twice with the same layout."""
    out = []
    for n in RUN_SMALL_N:
        for lay in RUN_LAYOUTS:
            for c in range(8):
                out.append((lay, n, bool(c & 1), bool(c & 2), bool(c & 4)))
    for k, n in enumerate(RUN_LARGE_N):
        for j, lay in enumerate(RUN_LAYOUTS):
            c = (3 * k + j) % 8
            out.append((lay, n, bool(c & 1), bool(c & 2), bool(c & 4)))
    return out


def run_lengths(layout, n, rng):
    if layout == "distinct":
        return np.ones(n, np.int64)
    if layout == "equal":
        return np.array([n], np.int64)
    if layout == "random_1_9":
        lens = rng.integers(1, 10, n)
    elif layout == "across_seams":                  # heads at 0, 100, 356, 612, ...: every run but the first lies across a 256-position seam
        lens = np.concatenate([[100], np.full(n // 256 + 1, 256)])
    elif layout == "long_700":                      # 700 positions with one head: two whole 256-position blocks hold none
        lens = np.tile([700, 1, 3], n // 704 + 1)
    else:
        raise KeyError(layout)
    lens = np.asarray(lens, np.int64)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]
    lens[-1] -= lens.sum() - n
    return lens[lens > 0]


def run_input(layout, n, sentinel_run, with_w):
    """A sort's output on n points whose keys are laid out as `layout` says: keys_sorted, order (NOT iota: the points carry their
    keys in random order), the planes x, y, z (and w) with magnitudes from 1e-3 to 1e3, and the sentinel key."""
    rng = _rng("runs", layout, n, sentinel_run)
    lens = run_lengths(layout, n, rng)
    assert lens.sum() == n and lens.min() >= 1
    values = np.cumsum(rng.integers(1, 4, len(lens))).astype(np.uint32)      # ascending, with gaps
    keys_sorted = np.repeat(values, lens)
    sentinel = np.uint32(int(values[-1]) + 1)
    if sentinel_run:
        keys_sorted[n - max(1, n // 50):] = sentinel                          # non-finite points: always the last run, never a centroid
    # sorted position j holds point order[j]: a random permutation.  (A stable sort's own output is ascending inside a run, which for
    # the "equal" layout is iota and would let a kernel that ignores `order` pass; the kernels promise the chain in ascending POSITION.)
    order = rng.permutation(n).astype(np.int32)
    planes = [(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32) for _ in range(4 if with_w else 3)]
    return keys_sorted, order, planes, sentinel

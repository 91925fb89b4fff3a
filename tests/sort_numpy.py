"""Plain restatements of the primitives of csrc/lsd_sort.hip, for test_sort_primitives_cpu.py / _gpu.py: the stable sort of (uint32 key,
int32 value) pairs on the low covered_bits of the key, the exclusive int32 scan, the table of runs of equal keys, the float centroid
of every run, and the launch plan (passes, bits, workgroup form, block counts) as a function of (n, end_bit).

Nothing here is tuned to the kernels' output: the sort is numpy's stable argsort, the scan an int64 cumulative sum, the runs come from
np.diff, and the centroid is the float32 chain pcl::CentroidPoint performs (0 + p0 + p1 + ... in ascending sorted position, then one
float32 division by the count).  np.sum / np.mean are NOT used: they add pairwise."""
import numpy as np

# the constants of csrc/lsd_sort.hip the plan depends on
RS_THREADS, RS_MAX_BITS, RS_FUSED_MAX_BLOCKS, STEPS8_MAX_N = 256, 11, 256, 600000
XS_CHUNK, RUN_CHUNK, SCAN_THREADS = 4096, 256, 1024
PLAN_FIELDS = ("passes", "bits", "steps", "nblk", "fused", "covered_bits", "scan_blocks", "scan_single_block", "scan_per",
               "run_blocks", "run_per")


def mask(bits):
    return np.uint32((1 << min(bits, 32)) - 1)      # three passes of 11 bits cover 33: a key has 32


def plan(n, end_bit):
    """What sort_pairs_u32_lsd(n, end_bit), exclusive_scan_i32_lsd(n) and sorted_runs_begin(n) launch."""
    assert n >= 1 and 1 <= end_bit <= 32
    passes = -(-end_bit // RS_MAX_BITS)
    bits = -(-end_bit // passes)
    steps = 8 if n <= STEPS8_MAX_N else 16
    nblk = -(-n // (RS_THREADS * steps))
    scan_blocks, run_blocks = -(-n // XS_CHUNK), -(-n // RUN_CHUNK)
    return dict(passes=passes, bits=bits, steps=steps, nblk=nblk, fused=int(nblk <= RS_FUSED_MAX_BLOCKS), covered_bits=passes * bits,
                scan_blocks=scan_blocks, scan_single_block=int(scan_blocks == 1), scan_per=-(-scan_blocks // SCAN_THREADS),
                run_blocks=run_blocks, run_per=-(-run_blocks // SCAN_THREADS))


def plan_words(n, end_bit):
    p = plan(n, end_bit)
    return [p[f] for f in PLAN_FIELDS]


def sort_pairs(keys, vals, end_bit):
    """(keys, values) in the order of a stable sort on keys & mask(covered_bits); vals None = 0 .. n - 1.  All 32 key bits are carried."""
    keys = np.asarray(keys, np.uint32)
    vals = np.arange(len(keys), dtype=np.int32) if vals is None else np.asarray(vals, np.int32)
    order = np.argsort(keys & mask(plan(len(keys), end_bit)["covered_bits"]), kind="stable")
    return keys[order], vals[order]


def exclusive_scan(a):
    c = np.cumsum(np.asarray(a, np.int32), dtype=np.int64)
    return np.concatenate([[0], c[:-1]]).astype(np.int32)


def run_table(keys_sorted):
    """run_key[r], run_off[r] (with run_off[number of runs] = n) of the runs of equal keys"""
    keys_sorted = np.asarray(keys_sorted, np.uint32)
    heads = np.concatenate([[0], np.flatnonzero(np.diff(keys_sorted)) + 1]).astype(np.int64)
    return keys_sorted[heads], np.concatenate([heads, [len(keys_sorted)]]).astype(np.int32)


def chain_sum(v):
    """0 + v[0] + v[1] + ... in float32, one addition after the other (np.cumsum accumulates sequentially)"""
    return np.cumsum(np.concatenate([np.zeros(1, np.float32), np.asarray(v, np.float32)]), dtype=np.float32)[-1]


def run_centroids(run_off, order, planes, long_run=64):
    """Per plane, the centroid of every run: the float32 chain over the run's points planes[k][order[j]], j ascending, divided in
    float32 by float32(count).  Runs of up to long_run points advance together, one vector addition per position in the run; longer
    ones are summed one by one with chain_sum: the same chain either way (test_sort_primitives_cpu.py holds both to an explicit loop)."""
    run_off = np.asarray(run_off, np.int64)
    off, lens = run_off[:-1], np.diff(run_off)
    short = np.flatnonzero(lens <= long_run)
    out = []
    for plane in planes:
        g = np.asarray(plane, np.float32)[np.asarray(order, np.int64)]
        acc = np.zeros(len(off), np.float32)
        for k in range(int(lens[short].max()) if len(short) else 0):
            act = short[lens[short] > k]
            acc[act] = acc[act] + g[off[act] + k]
        for r in np.flatnonzero(lens > long_run):
            acc[r] = chain_sum(g[off[r]:off[r] + lens[r]])
        out.append(acc / lens.astype(np.float32))
    return out


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

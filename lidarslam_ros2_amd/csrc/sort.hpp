#pragma once
#include "common.hpp"

namespace lsr {
// ---- hand-written stable LSD radix sort + run finder (lsd_sort.hip) -------------------------------------------------------
// Sorts n pairs in passes = ceil(end_bit / 11) passes of bits = ceil(end_bit / passes) bits each, ping-ponging between (key_a, val_a)
// and (key_b, val_b).  The pairs come out ordered by the LOW passes * bits BITS of the key, which is at least end_bit and may be more
// (end_bit 23: three passes of 8 cover 24; end_bit 32: three of 11 cover all 32), equal ones in input order.  Callers keep their keys
// below 2^end_bit, where the two readings agree; a key bit between end_bit and passes * bits would be ordered by, and every bit above
// is carried unchanged and ignored.
// val_a == nullptr: the values are 0..n-1 (no iota pass), val_a_buf then serves as the "a" side from the second pass on (val_a_buf ==
// val_a is allowed: the first pass has read val_a before the second writes it).
// *result_in_b says where the sorted pairs ended up (the "b" side after an odd number of passes).  temp holds the histogram tables.
struct BuildScratch;
int sort_pairs_u32_lsd(unsigned int* key_a, unsigned int* key_b, int* val_a, int* val_a_buf, int* val_b, size_t n, int end_bit,
                       DevBuf<char>& temp, hipStream_t stream, bool* result_in_b, bool first_hist_done = false);
// The scratch of a sort-based builder, carved out of sc.words for n keys: both sides of the sort's ping-pong and the run heads' block
// tables; with a run table also run_key / run_off (n + 1 entries each) and 16 ints, the first of them for the run count in device
// memory (null otherwise).  The ladder starts 32 words into sc.words; the words in front of it are the caller's.
struct SortScratch {
  unsigned int *key_in, *key_out;
  int *val_in, *val_out;
  int *block_heads, *block_base;
  unsigned int* run_key;
  int *run_off, *nruns;
};
int sort_scratch_carve(BuildScratch& sc, size_t n, bool run_table, SortScratch* out);
// Sorts s.key_in (keys below 2^end_bit, see above) with the values 0..n-1: *keys / *order say where the sorted keys and the order ended up.
int sort_scratch_run(const SortScratch& s, size_t n, int end_bit, DevBuf<char>& temp, hipStream_t stream, const unsigned int** keys,
                     const int** order, bool first_hist_done = false);
// The first pass's histogram table as that call will lay it out in temp: digit-major uint16 rows hist[digit * row_pitch + workgroup],
// workgroup = 2048 consecutive keys (key i of workgroup b: b * 2048 + i), digit = key & mask.  A kernel that produces the keys may fill
// it and pass first_hist_done = true (only when `usable`).
struct LsdFirstHist { unsigned short* hist = nullptr; int row_pitch = 0, C = 0, nblk = 0; unsigned int mask = 0; bool usable = false; };
int lsd_first_hist_plan(size_t n, int end_bit, DevBuf<char>& temp, LsdFirstHist* out);
// Runs of equal keys of a sorted sequence: heads counted per 256-key block (block_heads), scanned into block_base; the number of
// runs travels to the host through sc's mailbox (sorted_runs_count polls it).  sorted_runs_blocks(n) = ints each table needs.
size_t sorted_runs_blocks(size_t n);
int sorted_runs_begin(const unsigned int* keys_sorted, size_t n, int* block_heads, int* block_base, BuildScratch& sc, hipStream_t stream,
                      unsigned int* token_out, const unsigned int* dims_dev = nullptr,   // dims_dev: see leaf_key_dims_kernel (ndt.hip)
                      int* total_dev = nullptr);   // total_dev: the number of runs left in device memory too
int sorted_runs_count(BuildScratch& sc, hipStream_t stream, unsigned int token, int* n_runs);
// The runs as a table (enqueue behind sorted_runs_begin; needs no host wait): run r in key order has key run_key[r] and covers the
// sorted positions [run_off[r], run_off[r + 1]); run_off[number of runs] = n.  run_key / run_off: n + 1 entries.
int sorted_runs_table(const unsigned int* keys_sorted, size_t n, const int* block_base, unsigned int* run_key, int* run_off, hipStream_t stream);
// Exclusive scan of an int array of any length (hand-written, three launches); in != out.
int exclusive_scan_i32_lsd(const int* in, int* out, size_t n, DevBuf<char>& temp, hipStream_t stream);
// pcl::VoxelGrid's centroid of every run (float sums, ascending point index; all fields): out[r] for run r in key order; the run
// of `sentinel` (always last) is skipped
int sorted_runs_centroids(const unsigned int* keys_sorted, const int* order, size_t n, const int* block_base, unsigned int sentinel,
                          const float* x, const float* y, const float* z, const float* w, float* ox, float* oy, float* oz, float* ow,
                          hipStream_t stream, const unsigned int* sentinel_dev = nullptr);   // sentinel_dev: the sentinel lives on the device
}  // namespace lsr

// pcl::VoxelGrid for map-sized clouds (csrc/map_filter.hip): records of an lsr_pc2_layout in HBM -> one centroid record per occupied
// leaf, in ascending leaf index, the leaf index carried in 64 bits.  The definition is voxel_grid_filter's (cloud_codec.hip) with a
// wider index — include/lidarslam_reg.h states it —, and wherever that filter accepts a cloud the two return the same bytes.
#pragma once
#include "common.hpp"

namespace lsr {

constexpr int MF_BBOX_MAX_BLOCKS = 1024;   // workgroups of the bounding-box pass: a record of 8 words each for the host to fold
constexpr int MF_CELL_LIMIT = 1 << 24;     // |min_b|, |max_b| stay below it: floorf(p * inv_leaf) - (float)min_b is exact there
constexpr int MF_DIV_LIMIT = 1 << 21;      // div_b per axis: the leaf index stays below 2^63

// the launches of one call, bracketed by hipEvents under LSR_PROFILE
enum MfLeg : int { MF_LEG_BBOX = 0, MF_LEG_KEY, MF_LEG_SORT, MF_LEG_RUNS, MF_LEG_CENTROID, MF_LEG_WRITE, MF_LEGS };

struct MfFields { int step, ox, oy, oz, oi; };   // bytes; oi < 0: no intensity field

// What a call has worked out between its two host waits: the grid, and where the sorted keys, the order and the run bases lie in the
// scratch.  Valid until the next call on the object.
struct MfPlan {
  size_t n = 0;
  unsigned int n_finite = 0;
  int min_b[3] = {0, 0, 0}, div_b[3] = {0, 0, 0};
  unsigned long long cells = 0;   // div_b0 * div_b1 * div_b2: one past the last leaf index, the key of a non-finite point
  int index_bits = 0;             // bits of the largest leaf index
  int sort_bits = 0;              // bits the sort orders: those of `cells` when a non-finite point carries it, else index_bits
  const unsigned int *lo = nullptr, *hi = nullptr;   // sorted key words (hi: null for a one-word index)
  const int* order = nullptr;                        // sorted position -> input record
  const int* block_base = nullptr;                   // runs in front of every 256-key chunk
  size_t n_leaves = 0;                               // occupied leaves = output records
};

// Scratch of the filter, kept on the object: reserved when first needed, never shrunk.
struct MapFilterState {
  DevBuf<unsigned int> words;      // key_a | key_b | val_a | val_b | lo_keep | hi_keep | block_heads | block_base
  DevBuf<char> temp;               // the sort's tables, then the scan's block sums
  DevBuf<unsigned int> parts;      // bounding-box records of the workgroups
  PinBuf<unsigned int> h_parts;    // ... their pinned copy, and behind them the word the leaf count is copied into
  DevBuf<float> centroids;         // x | y | z | intensity planes of the output
  DevBuf<unsigned char> thin;      // lsr_save_map_pcd_filtered: the filtered XYZI records on their way into the file
  hipEvent_t ev[2 * MF_LEGS] = {};
  bool have_events = false;
  int key_bits = 0;                // LSR_MAP_FILTER_KEY_BITS: index bits of the last filter on this object
  double ms[MF_LEGS] = {};         // hipEvent time of the last call's launches (LSR_PROFILE), else 0
  ~MapFilterState() {
    if (have_events)
      for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  int ensure_events() {
    if (have_events) return LSR_OK;
    for (hipEvent_t& e : ev) LSR_HIP(hipEventCreate(&e));
    have_events = true;
    return LSR_OK;
  }
};

// First half: bounding box (host wait), limits, keys, sort, run heads, and the leaf count (host wait).  d_records: n records of F in
// device memory, read on `stream`.  *P says what was found; P->n_leaves == 0: no finite point.  profile: bracket the launches.
int map_filter_runs(MapFilterState& S, const void* d_records, size_t n, const MfFields& F, float leaf, hipStream_t stream, bool profile,
                    MfPlan* P);
// Second half: the centroids of P's runs and the P->n_leaves records of `out` at d_out (device memory), every other byte zero.
// Enqueued, not waited for.
int map_filter_emit(MapFilterState& S, const void* d_records, const MfFields& F, const MfPlan& P, void* d_out, const MfFields& out,
                    hipStream_t stream, bool profile);
// the brackets of the last call read back (after the stream has been synchronised)
int map_filter_collect_ms(MapFilterState& S, bool emitted);

}  // namespace lsr

// The map window (csrc/map_window.hip): the records of a resident map whose absolute voxel cell lies in a box, cut out in input
// order on the device — lsr_crop_map and lsr_set_input_target_window of the C ABI (include/lidarslam_reg.h states the definition;
// the predicate itself is voxel_device.hpp: in_window).
#pragma once
#include "common.hpp"

namespace lsr {

constexpr int MW_CHUNK = 256;             // records per workgroup of the count and of the write: one per thread
constexpr int MW_SCAN_WIDTH = 1024;       // threads of the ONE workgroup that scans the counts: each takes ceil(workgroups / 1024) in a row
constexpr int MW_CELL_LIMIT = 1 << 24;    // |lo[k]|, |hi[k]| stay below it: an int cell is exact as a float there (map_filter.hpp: MF_CELL_LIMIT)

// Scratch of the cut, kept on the object: reserved when first needed, never shrunk.
struct MapWindowState {
  DevBuf<int> counts;              // kept records per workgroup | their exclusive prefix (one more entry: the total)
  DevBuf<unsigned char> records;   // lsr_set_input_target_window: the cut, pcl::PointXYZI records, on its way into the target
  hipEvent_t ev[4] = {};             // brackets of {count, scan} and of {write}: the host learns the count between them
  bool have_events = false;
  double ms = 0.0;                 // LSR_MAP_WINDOW_MS: hipEvent time of the last call's three launches (LSR_PROFILE), else 0
  ~MapWindowState() {
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

// The scan of the cut, for whoever compacts records by a flag (map_visibility.hip does): base[b] = counts[0] + .. + counts[b - 1] for
// b = 0 .. nb by ONE workgroup, enqueued on `stream`; the total also travels to sc's host mailbox under *token — sorted_runs_count
// (sort.hpp) waits for it.  counts != base.
int mw_scan_counts(BuildScratch& sc, hipStream_t stream, const int* counts, int nb, int* base, unsigned int* token);

}  // namespace lsr

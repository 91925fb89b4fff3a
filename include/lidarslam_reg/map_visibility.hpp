// lidarslam_reg/map_visibility.hpp — header-only helpers over lsr_depth_images_build and lsr_assemble_map_static (lidarslam_reg.h):
// the map without what moved.  A backend keeps one eroded depth image per keyframe beside its MapArray, extends the table by the new
// keyframes only, and assembles the map it publishes or saves from the records no neighbouring keyframe saw through.
//
// Needs neither PCL nor Eigen.  INTEGRATION.md §3m shows the map half of doPoseAdjustment written with it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lidarslam_reg.h"

namespace lidarslam_reg {

// 128 columns per 90 degrees x 32 rows out to +-30 degrees, 0.5 .. 80 m; a vote needs 0.5 m of free space behind the record; the 32
// nearest keyframes within 30 m look, two votes remove; the lidar at the keyframe's origin
inline lsr_visibility_params visibilityDefaults() {
  return lsr_visibility_params{128, 32, 0.57735026918962573, 0.5, 80.0, 0.5, 30.0, 32, 2, {0.0, 0.0, 0.0}};
}

// The resident table of eroded depth images of a MapArray (host memory): update() computes the images of the submaps added since the
// last call — an image depends on its own cloud alone, not on any pose — and appends them.
struct DepthImageTable {
  lsr_visibility_params params = visibilityDefaults();
  std::vector<float> images;   // count x height x 4 face_width
  int count = 0;

  size_t pixels() const { return (size_t)params.height * 4 * (size_t)params.face_width; }

  // submaps: the whole MapArray so far (clouds of `layout`, host memory or HIP device pointers with clouds_on_device)
  bool update(lsr_handle h, const std::vector<lsr_submap>& submaps, const lsr_pc2_layout& layout = lsr_pc2_layout{32u, 0u, 4u, 8u, 16},
              bool clouds_on_device = false) {
    const int n = (int)submaps.size();
    if (n <= count) return true;
    images.resize((size_t)n * pixels());
    const int st = lsr_depth_images_build(h, submaps.data() + count, n - count, &layout, clouds_on_device ? 1 : 0, &params, 1,
                                          images.data() + (size_t)count * pixels(), 0);
    if (st != LSR_OK) {
      std::fprintf(stderr, "[lidarslam_reg::DepthImageTable] %s: %s\n", lsr_status_string(st), lsr_last_error());
      images.resize((size_t)count * pixels());
      return false;
    }
    count = n;
    return true;
  }
};

// The static map into `records` (pcl::PointXYZI records in host memory, resized to what is kept): every submap moved by its stored
// pose, or by poses16 (column-major fp64 4x4 each: the optimiser's estimates) when given; first_record (optional) indexes the kept
// records of every submap; *n_removed (optional) = the records left out.  false: refused or failed (reported on stderr), records empty.
inline bool assembleStaticMap(lsr_handle h, const std::vector<lsr_submap>& submaps, const DepthImageTable& table,
                              std::vector<unsigned char>& records, const double* poses16 = nullptr,
                              std::vector<size_t>* first_record = nullptr, size_t* n_removed = nullptr,
                              const lsr_pc2_layout& layout = lsr_pc2_layout{32u, 0u, 4u, 8u, 16}, bool clouds_on_device = false) {
  const int n = (int)submaps.size();
  std::vector<size_t> first((size_t)(n > 0 ? n : 0) + 1, 0);
  size_t total = 0, kept = 0, removed = 0;
  for (const lsr_submap& s : submaps) total += s.n_points;
  int st = LSR_ERR_INVALID_ARGUMENT;
  if (table.count != n) {
    std::fprintf(stderr, "[lidarslam_reg::assembleStaticMap] the image table holds %d of %d submaps\n", table.count, n);
  } else {
    records.resize((total > 0 ? total : 1) * layout.point_step);   // room for the raw map: one call, no counting pass
    st = lsr_assemble_map_static(h, submaps.data(), n, &layout, clouds_on_device ? 1 : 0, poses16, table.images.data(), 0, &table.params,
                                 records.data(), total, &layout, 0, first.data(), &kept, &removed);
    if (st != LSR_OK) std::fprintf(stderr, "[lidarslam_reg::assembleStaticMap] %s: %s\n", lsr_status_string(st), lsr_last_error());
  }
  if (st != LSR_OK) {
    records.clear();
    return false;
  }
  records.resize(kept * layout.point_step);
  if (first_record) *first_record = first;
  if (n_removed) *n_removed = removed;
  return true;
}

}  // namespace lidarslam_reg

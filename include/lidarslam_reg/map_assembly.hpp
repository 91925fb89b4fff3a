// lidarslam_reg/map_assembly.hpp — header-only helper over lsr_assemble_map (lidarslam_reg.h): the whole map from the submaps of a
// lidarslam_msgs/MapArray, on the device.
//
//   scanmatcher/src/scanmatcher_component.cpp:529-552        ScanMatcherComponent::publishMap
//   graph_based_slam/src/graph_based_slam_component.cpp:321-368   the map half of doPoseAdjustment
//
// Needs neither PCL nor Eigen: a pose is anything whose .matrix().data() yields 16 column-major doubles (Eigen::Isometry3d,
// Eigen::Affine3d — g2o's vertex->estimate()).  INTEGRATION.md §3e shows the two call sites replaced.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lidarslam_reg.h"

namespace lidarslam_reg {

// pcl::PointXYZI as pcl::toROSMsg lays it out: what SubMap.cloud holds and what the map is published in
inline lsr_pc2_layout pointXYZILayout() { return lsr_pc2_layout{32u, 0u, 4u, 8u, 16}; }

inline size_t mapRecordCount(const std::vector<lsr_submap>& submaps) {
  size_t n = 0;
  for (const lsr_submap& s : submaps) n += s.n_points;
  return n;
}

// poses16_or_null: submaps.size() column-major fp64 4x4 matrices, or nullptr = every submap's own position / orientation.
// payload receives the PointCloud2 data of the whole map (host); first_record (nullable) submaps.size() + 1 record indices:
// payload[first_record[i] * point_step .. first_record[i + 1] * point_step) is the moved cloud of submap i.
// Reports like the registration adapter does (stderr, false) and leaves payload empty on failure.
inline bool assembleMap(lsr_handle h, const std::vector<lsr_submap>& submaps, const double* poses16_or_null, std::vector<uint8_t>& payload,
                        std::vector<size_t>* first_record = nullptr, const lsr_pc2_layout& in_layout = pointXYZILayout(),
                        const lsr_pc2_layout& out_layout = pointXYZILayout(), bool submaps_on_device = false) {
  const size_t total = mapRecordCount(submaps);
  payload.assign(total * out_layout.point_step, 0);
  std::vector<size_t> first(submaps.size() + 1, 0);
  size_t n_out = 0;
  const int st = lsr_assemble_map(h, submaps.data(), (int)submaps.size(), &in_layout, submaps_on_device ? 1 : 0, poses16_or_null,
                                  payload.data(), total, &out_layout, /*out_on_device=*/0, first.data(), &n_out);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::assembleMap] %s: %s\n", lsr_status_string(st), lsr_last_error());
    payload.clear();
    return false;
  }
  if (first_record) first_record->swap(first);
  return true;
}

// The same with the optimiser's poses as objects: Pose::matrix().data() = 16 column-major doubles.  poses_or_null: submaps.size()
// entries, or nullptr = the submaps' own poses.
template <typename Pose>
inline bool assembleMap(lsr_handle h, const std::vector<lsr_submap>& submaps, const Pose* poses_or_null, std::vector<uint8_t>& payload,
                        std::vector<size_t>* first_record = nullptr) {
  if (!poses_or_null) return assembleMap(h, submaps, static_cast<const double*>(nullptr), payload, first_record);
  std::vector<double> poses16(16 * submaps.size());
  for (size_t i = 0; i < submaps.size(); i++) {
    const auto M = poses_or_null[i].matrix();
    std::memcpy(poses16.data() + 16 * i, M.data(), 16 * sizeof(double));
  }
  return assembleMap(h, submaps, poses16.data(), payload, first_record);
}

// Device output: the map stays in HBM (d_out: capacity_points records of out_layout).  *n_out receives the record count.  Appending
// to a resident map: pass the new submaps only and d_out advanced by the records it already holds.
inline bool assembleMapDevice(lsr_handle h, const std::vector<lsr_submap>& submaps, const double* poses16_or_null, void* d_out,
                              size_t capacity_points, size_t* n_out, std::vector<size_t>* first_record = nullptr,
                              bool submaps_on_device = true, const lsr_pc2_layout& in_layout = pointXYZILayout(),
                              const lsr_pc2_layout& out_layout = pointXYZILayout()) {
  std::vector<size_t> first(submaps.size() + 1, 0);
  size_t n = 0;
  const int st = lsr_assemble_map(h, submaps.data(), (int)submaps.size(), &in_layout, submaps_on_device ? 1 : 0, poses16_or_null, d_out,
                                  capacity_points, &out_layout, /*out_on_device=*/1, first.data(), &n);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::assembleMapDevice] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_out) *n_out = n;
  if (first_record) first_record->swap(first);
  return true;
}

// ---- the map thinned with a leaf size before it leaves the device (lsr_voxel_grid_filter_map, lsr_assemble_map_filtered) ----------
// The forms with a leaf carry their own names: next to the bool and defaulted arguments above, an overload told apart by one float
// argument would be chosen or refused by the literal's type (0.1 against 0.1f).

// pcl::VoxelGrid(leaf).filter of n records of in_layout (host memory, or a HIP device pointer with records_on_device) into `payload`
// (host): one record of out_layout per occupied leaf, in ascending leaf index, the leaf index carried in 64 bits — a map of
// kilometres at a 0.1 m leaf.  Leaves payload empty on failure.
inline bool voxelGridFilterMap(lsr_handle h, const void* records, size_t n, float leaf, std::vector<uint8_t>& payload,
                               const lsr_pc2_layout& in_layout = pointXYZILayout(), const lsr_pc2_layout& out_layout = pointXYZILayout(),
                               bool records_on_device = false) {
  size_t m = 0;
  int st = lsr_voxel_grid_filter_map(h, records, n, &in_layout, records_on_device ? 1 : 0, leaf, nullptr, 0, &out_layout, 0, &m);
  if (st == LSR_OK) {
    payload.assign(m * out_layout.point_step, 0);
    if (m) st = lsr_voxel_grid_filter_map(h, records, n, &in_layout, records_on_device ? 1 : 0, leaf, payload.data(), m, &out_layout, 0, &m);
  }
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::voxelGridFilterMap] %s: %s\n", lsr_status_string(st), lsr_last_error());
    payload.clear();
    return false;
  }
  return true;
}

// assembleMap followed by that filter, the raw map never leaving HBM: payload receives the thinned map (host).  There is no
// first_record: a leaf mixes submaps.  Two calls, like voxelGridFilterMap above: the count, which sizes the payload, then the records (a caller
// that can spare the raw map's size on the device uses assembleMapFilteredDevice below: one call).
inline bool assembleMapFiltered(lsr_handle h, const std::vector<lsr_submap>& submaps, const double* poses16_or_null, float leaf,
                                std::vector<uint8_t>& payload, const lsr_pc2_layout& in_layout = pointXYZILayout(),
                                const lsr_pc2_layout& out_layout = pointXYZILayout(), bool submaps_on_device = false) {
  size_t m = 0;
  int st = lsr_assemble_map_filtered(h, submaps.data(), (int)submaps.size(), &in_layout, submaps_on_device ? 1 : 0, poses16_or_null, leaf,
                                     nullptr, 0, &out_layout, 0, &m);
  if (st == LSR_OK) {
    payload.assign(m * out_layout.point_step, 0);
    if (m)
      st = lsr_assemble_map_filtered(h, submaps.data(), (int)submaps.size(), &in_layout, submaps_on_device ? 1 : 0, poses16_or_null, leaf,
                                     payload.data(), m, &out_layout, 0, &m);
  }
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::assembleMapFiltered] %s: %s\n", lsr_status_string(st), lsr_last_error());
    payload.clear();
    return false;
  }
  return true;
}

// The same with the optimiser's poses as objects (Pose::matrix().data() = 16 column-major doubles), or nullptr = the submaps' own.
template <typename Pose>
inline bool assembleMapFiltered(lsr_handle h, const std::vector<lsr_submap>& submaps, const Pose* poses_or_null, float leaf,
                                std::vector<uint8_t>& payload) {
  if (!poses_or_null) return assembleMapFiltered(h, submaps, static_cast<const double*>(nullptr), leaf, payload);
  std::vector<double> poses16(16 * submaps.size());
  for (size_t i = 0; i < submaps.size(); i++) {
    const auto M = poses_or_null[i].matrix();
    std::memcpy(poses16.data() + 16 * i, M.data(), 16 * sizeof(double));
  }
  return assembleMapFiltered(h, submaps, poses16.data(), leaf, payload);
}

// Device output: the thinned map stays in HBM (d_out: capacity_points records of out_layout; the raw map's record count always
// suffices).  *n_out receives the record count.
inline bool assembleMapFilteredDevice(lsr_handle h, const std::vector<lsr_submap>& submaps, const double* poses16_or_null, float leaf,
                                      void* d_out, size_t capacity_points, size_t* n_out, bool submaps_on_device = true,
                                      const lsr_pc2_layout& in_layout = pointXYZILayout(),
                                      const lsr_pc2_layout& out_layout = pointXYZILayout()) {
  size_t n = 0;
  const int st = lsr_assemble_map_filtered(h, submaps.data(), (int)submaps.size(), &in_layout, submaps_on_device ? 1 : 0, poses16_or_null,
                                           leaf, d_out, capacity_points, &out_layout, /*out_on_device=*/1, &n);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::assembleMapFilteredDevice] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_out) *n_out = n;
  return true;
}

}  // namespace lidarslam_reg

// lidarslam_reg/pcd_io.hpp — header-only helpers over lsr_save_pcd_ascii / lsr_save_map_pcd_ascii (lidarslam_reg.h): map.pcd written
// from the device, the bytes pcl::io::savePCDFileASCII writes — and over lsr_load_pcd / lsr_set_input_target_pcd: such a file (or any
// PCD v0.7 file, DATA ascii or binary — binary_compressed after pcdReadCompressed(h, true) —, with float x y z [intensity]) read back on
// the device.
//
//   graph_based_slam/src/graph_based_slam_component.cpp:369   if (do_save_map) {pcl::io::savePCDFileASCII("map.pcd", *map_ptr);} // too heavy
//
// Needs neither PCL nor Eigen nor HIP: a pose is anything whose .matrix().data() yields 16 column-major doubles (Eigen::Isometry3d,
// Eigen::Affine3d — g2o's vertex->estimate()).  INTEGRATION.md §3g shows the call site replaced.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../lidarslam_reg.h"

namespace lidarslam_reg {

// pcl::PointXYZI as pcl::toROSMsg lays it out: what SubMap.cloud holds
inline lsr_pc2_layout pcdPointXYZILayout() { return lsr_pc2_layout{32u, 0u, 4u, 8u, 16}; }

// pcl::io::savePCDFileASCII(path, cloud) for n records of `layout` in `payload` (a PointCloud2's data; host memory, or a HIP device
// pointer with payload_on_device).  Reports like the registration adapter does (stderr, false); a file that could not be completed is
// removed.  n_bytes (nullable) receives the file's size.
inline bool savePCDFileASCII(lsr_handle h, const std::string& path, const void* payload, size_t n,
                             const lsr_pc2_layout& layout = pcdPointXYZILayout(), bool payload_on_device = false, size_t* n_bytes = nullptr) {
  size_t bytes = 0;
  const int st = lsr_save_pcd_ascii(h, path.c_str(), payload, n, &layout, payload_on_device ? 1 : 0, &bytes);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::savePCDFileASCII] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_bytes) *n_bytes = bytes;
  return true;
}

// pcl::io::savePCDFileBinary(path, cloud) for the fields x y z [intensity]: a DATA binary file of PACKED records of 12 or 16 bytes, the
// fields bit for bit (PCL writes the 32-byte PointXYZI struct with its padding; every PCD reader loads both into the same points).
inline bool savePCDFileBinary(lsr_handle h, const std::string& path, const void* payload, size_t n,
                              const lsr_pc2_layout& layout = pcdPointXYZILayout(), bool payload_on_device = false, size_t* n_bytes = nullptr) {
  size_t bytes = 0;
  const int st = lsr_save_pcd(h, path.c_str(), payload, n, &layout, payload_on_device ? 1 : 0, LSR_PCD_BINARY, &bytes);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::savePCDFileBinary] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_bytes) *n_bytes = bytes;
  return true;
}

// pcl::io::savePCDFileBinaryCompressed(path, cloud) for the same fields: the field-major image as one LZF stream, compressed on the
// device (the stream is the project's own parse, a valid LZF stream every PCD reader inflates to the same image).
inline bool savePCDFileBinaryCompressed(lsr_handle h, const std::string& path, const void* payload, size_t n,
                                        const lsr_pc2_layout& layout = pcdPointXYZILayout(), bool payload_on_device = false,
                                        size_t* n_bytes = nullptr) {
  size_t bytes = 0;
  const int st = lsr_save_pcd(h, path.c_str(), payload, n, &layout, payload_on_device ? 1 : 0, LSR_PCD_BINARY_COMPRESSED, &bytes);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::savePCDFileBinaryCompressed] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_bytes) *n_bytes = bytes;
  return true;
}

// The whole map of a MapArray as map.pcd in one call: every submap moved by its pose on the device — poses16_or_null: submaps.size()
// column-major fp64 4x4 matrices, or nullptr = every submap's own position / orientation —, the map kept in HBM, its text formatted
// there and written piece by piece.  The records are those lsr_assemble_map gives the same arguments.
// data_kind: LSR_PCD_ASCII (the default: savePCDFileASCII's bytes), LSR_PCD_BINARY or LSR_PCD_BINARY_COMPRESSED.
inline bool saveMapPCD(lsr_handle h, const std::string& path, const std::vector<lsr_submap>& submaps, const double* poses16_or_null,
                       bool submaps_on_device = false, const lsr_pc2_layout& in_layout = pcdPointXYZILayout(), size_t* n_bytes = nullptr,
                       int data_kind = LSR_PCD_ASCII) {
  size_t bytes = 0;
  const int st = lsr_save_map_pcd(h, path.c_str(), submaps.data(), (int)submaps.size(), &in_layout, submaps_on_device ? 1 : 0,
                                  poses16_or_null, data_kind, &bytes);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::saveMapPCD] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_bytes) *n_bytes = bytes;
  return true;
}

// The same with the optimiser's poses as objects: Pose::matrix().data() = 16 column-major doubles.  poses_or_null: submaps.size()
// entries, or nullptr = the submaps' own poses.
template <typename Pose>
inline bool saveMapPCD(lsr_handle h, const std::string& path, const std::vector<lsr_submap>& submaps, const Pose* poses_or_null,
                       bool submaps_on_device = false, int data_kind = LSR_PCD_ASCII) {
  if (!poses_or_null)
    return saveMapPCD(h, path, submaps, static_cast<const double*>(nullptr), submaps_on_device, pcdPointXYZILayout(), nullptr, data_kind);
  std::vector<double> poses16(16 * submaps.size());
  for (size_t i = 0; i < submaps.size(); i++) {
    const auto M = poses_or_null[i].matrix();
    std::memcpy(poses16.data() + 16 * i, M.data(), 16 * sizeof(double));
  }
  return saveMapPCD(h, path, submaps, poses16.data(), submaps_on_device, pcdPointXYZILayout(), nullptr, data_kind);
}

// saveMapPCD with the map thinned first: pcl::VoxelGrid(leaf) over the whole map on the device, the leaf index carried in 64 bits
// (lsr_save_map_pcd_filtered: assemble, filter, write; neither map visits the host as records).  n_points (nullable) receives the
// number of records in the file.  (A name of its own: next to saveMapPCD's bool and defaulted arguments an overload told apart by one
// float would be chosen or refused by the literal's type.)
inline bool saveMapPCDFiltered(lsr_handle h, const std::string& path, const std::vector<lsr_submap>& submaps, const double* poses16_or_null,
                               float leaf, int data_kind = LSR_PCD_ASCII, bool submaps_on_device = false,
                               const lsr_pc2_layout& in_layout = pcdPointXYZILayout(), size_t* n_points = nullptr, size_t* n_bytes = nullptr) {
  size_t bytes = 0, points = 0;
  const int st = lsr_save_map_pcd_filtered(h, path.c_str(), submaps.data(), (int)submaps.size(), &in_layout, submaps_on_device ? 1 : 0,
                                           poses16_or_null, leaf, data_kind, &points, &bytes);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::saveMapPCDFiltered] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_points) *n_points = points;
  if (n_bytes) *n_bytes = bytes;
  return true;
}

// The same with the optimiser's poses as objects (Pose::matrix().data() = 16 column-major doubles), or nullptr = the submaps' own.
template <typename Pose>
inline bool saveMapPCDFiltered(lsr_handle h, const std::string& path, const std::vector<lsr_submap>& submaps, const Pose* poses_or_null,
                               float leaf, int data_kind = LSR_PCD_ASCII, bool submaps_on_device = false) {
  if (!poses_or_null) return saveMapPCDFiltered(h, path, submaps, static_cast<const double*>(nullptr), leaf, data_kind, submaps_on_device);
  std::vector<double> poses16(16 * submaps.size());
  for (size_t i = 0; i < submaps.size(); i++) {
    const auto M = poses_or_null[i].matrix();
    std::memcpy(poses16.data() + 16 * i, M.data(), 16 * sizeof(double));
  }
  return saveMapPCDFiltered(h, path, submaps, poses16.data(), leaf, data_kind, submaps_on_device);
}

// Whether lsr_load_pcd / lsr_set_input_target_pcd / lsr_decode_pcd of this object read DATA binary_compressed files (what
// pcl::io::savePCDFileBinaryCompressed writes), the LZF stream inflated on the device (LSR_PCD_READ_COMPRESSED; off by default: such a
// file is then refused as not implemented).
inline bool pcdReadCompressed(lsr_handle h, bool on) {
  const int st = lsr_set_i32(h, LSR_PCD_READ_COMPRESSED, on ? 1 : 0);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::pcdReadCompressed] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  return true;
}

// pcl::io::loadPCDFile(path, cloud) for the fields x y z [intensity]: the file's records, in `layout`, into `payload` (resized to
// n * point_step bytes; a PointCloud2's data).  The text is parsed on the device while this thread reads the file.  Reports like the
// save helpers (stderr, false); on failure `payload` is left as it was.  n_points (nullable) receives the count.
inline bool loadPCDFile(lsr_handle h, const std::string& path, std::vector<uint8_t>& payload, const lsr_pc2_layout& layout = pcdPointXYZILayout(),
                        size_t* n_points = nullptr) {
  size_t n = 0;
  int st = lsr_load_pcd(h, path.c_str(), nullptr, 0, nullptr, 0, &n);
  std::vector<uint8_t> records;
  if (st == LSR_OK) {
    records.resize(n * layout.point_step);
    st = lsr_load_pcd(h, path.c_str(), records.data(), n, &layout, 0, &n);
  }
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::loadPCDFile] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  payload.swap(records);
  if (n_points) *n_points = n;
  return true;
}

// registration->setInputTarget(map) with the map in a .pcd file: the records never visit the host.  n_points (nullable) receives the count.
inline bool setInputTargetPCD(lsr_handle h, const std::string& path, size_t* n_points = nullptr) {
  size_t n = 0;
  const int st = lsr_set_input_target_pcd(h, path.c_str(), &n);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::setInputTargetPCD] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_points) *n_points = n;
  return true;
}

}  // namespace lidarslam_reg

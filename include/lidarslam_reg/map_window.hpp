// lidarslam_reg/map_window.hpp — header-only helpers over lsr_map_window_around, lsr_crop_map and lsr_set_input_target_window
// (lidarslam_reg.h): localising in a saved map.  The target of a registration is not the whole map but the window of it around the
// pose — the records whose voxel cell lies in a box of whole cells, cut out of the resident map in input order on the device.  With
// leaf = the NDT resolution the window's leaves are, bit for bit, the whole map's.
//
// Needs neither PCL nor Eigen.  INTEGRATION.md §3g shows a localiser's callback written with it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lidarslam_reg.h"

namespace lidarslam_reg {

// The window of whole cells of size `leaf` that covers center +- half_extent (metres).  false: refused (reported on stderr), *w untouched.
inline bool mapWindowAround(const double center[3], const double half_extent[3], float leaf, lsr_map_window* w) {
  const int st = lsr_map_window_around(center, half_extent, leaf, w);
  if (st != LSR_OK) std::fprintf(stderr, "[lidarslam_reg::mapWindowAround] %s: %s\n", lsr_status_string(st), lsr_last_error());
  return st == LSR_OK;
}

// The records of the window into `payload` (host): n records of in_layout (host memory, or a HIP device pointer with
// records_on_device) -> the kept ones, in input order, as records of out_layout.  Two calls: the count, which sizes the payload, then
// the records.  Leaves payload empty on failure.
inline bool cropMap(lsr_handle h, const void* records, size_t n, const lsr_map_window& w, std::vector<uint8_t>& payload,
                    const lsr_pc2_layout& in_layout = lsr_pc2_layout{32u, 0u, 4u, 8u, 16},
                    const lsr_pc2_layout& out_layout = lsr_pc2_layout{32u, 0u, 4u, 8u, 16}, bool records_on_device = false) {
  size_t m = 0;
  int st = lsr_crop_map(h, records, n, &in_layout, records_on_device ? 1 : 0, &w, nullptr, 0, &out_layout, 0, &m);
  if (st == LSR_OK) {
    payload.assign(m * out_layout.point_step, 0);
    if (m) st = lsr_crop_map(h, records, n, &in_layout, records_on_device ? 1 : 0, &w, payload.data(), m, &out_layout, 0, &m);
  }
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::cropMap] %s: %s\n", lsr_status_string(st), lsr_last_error());
    payload.clear();
    return false;
  }
  return true;
}

// Device output: the cut stays in HBM (d_out: capacity_points records of out_layout).  *n_out receives the record count.
inline bool cropMapDevice(lsr_handle h, const void* d_records, size_t n, const lsr_map_window& w, void* d_out, size_t capacity_points,
                          size_t* n_out, const lsr_pc2_layout& in_layout = lsr_pc2_layout{32u, 0u, 4u, 8u, 16},
                          const lsr_pc2_layout& out_layout = lsr_pc2_layout{32u, 0u, 4u, 8u, 16}) {
  size_t m = 0;
  const int st = lsr_crop_map(h, d_records, n, &in_layout, 1, &w, d_out, capacity_points, &out_layout, 1, &m);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::cropMapDevice] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  if (n_out) *n_out = m;
  return true;
}

// The re-cut rule of a localiser.  Two per-axis parameters in metres: `reach`, how far scan points lie from the pose, and `slack`.  A
// cut is the window around the pose's translation t with the half extent reach + slack; the map is cut again once t has left the
// centre of the current cut by more than slack / 2 on any axis.  A pose outside the current window altogether is reported as lost (and
// asks for a cut around it): it is never hidden.
struct MapWindowTracker {
  double reach[3] = {100.0, 100.0, 30.0};
  double slack[3] = {20.0, 20.0, 10.0};
  float leaf = 1.0f;           // the NDT resolution; for GICP a leaf of the caller's choice
  lsr_map_window window = {0.f, {0, 0, 0}, {0, 0, 0}};
  double center[3] = {0, 0, 0};
  bool has_window = false, lost = false;
  int n_recuts = 0;            // cuts after the first

  bool contains(const double t[3]) const {
    if (!has_window) return false;
    const float inv_leaf = 1.0f / window.leaf;
    for (int k = 0; k < 3; k++) {
      const float f = std::floor((float)t[k] * inv_leaf);
      if (!((float)window.lo[k] <= f && f <= (float)window.hi[k])) return false;
    }
    return true;
  }
  // Does the target have to be cut again for a pose at t?  (Sets `lost` when t is outside the current window.)
  bool needsCut(const double t[3]) {
    if (!has_window) return true;
    if (!contains(t)) { lost = true; return true; }
    for (int k = 0; k < 3; k++)
      if (std::fabs(t[k] - center[k]) > slack[k] / 2) return true;
    return false;
  }
  // The window around t; the caller hands it to setInputTargetWindow.  false: refused, the current window stays.
  bool cutAround(const double t[3]) {
    const double half[3] = {reach[0] + slack[0], reach[1] + slack[1], reach[2] + slack[2]};
    lsr_map_window w;
    if (!mapWindowAround(t, half, leaf, &w)) return false;
    if (has_window) n_recuts++;
    window = w;
    for (int k = 0; k < 3; k++) center[k] = t[k];
    has_window = true;
    return true;
  }
};

}  // namespace lidarslam_reg

// lidarslam_reg/scan_context.hpp — header-only helpers over lsr_scan_context_build, lsr_scan_context_match and
// lsr_search_loop_appearance (lidarslam_reg.h): loop closure by appearance.  A backend keeps one Scan Context descriptor per keyframe
// beside its MapArray, extends the table by the new keyframes only, and asks the appearance gate where searchLoop asks its range
// gate; the edges come back as lsr_loop_edge, what loop_edges_ is filled from.
//
// Needs neither PCL nor Eigen.  INTEGRATION.md §3l shows searchLoop written with it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../lidarslam_reg.h"

namespace lidarslam_reg {

inline lsr_scan_context_params scanContextDefaults() { return lsr_scan_context_params{20, 60, 80.0, 2.0}; }

// The gate's parameters with the library's defaults: the node's searchLoop parameters, 20 x 60 cells out to 80 m, candidates below a
// Scan Context distance of 0.4, a lattice of 7 x 7 starts 1 m apart around the appearance guess, up to 16 of them refined.
inline lsr_appearance_loop_params appearanceLoopDefaults(const lsr_loop_params& loop) {
  lsr_appearance_loop_params p;
  p.loop = loop;
  p.sc = scanContextDefaults();
  p.sc_distance_threshold = 0.4;
  p.search.lattice = lsr_pose_lattice{{7, 7, 1}, {1.0, 1.0, 1.0}, 1, 0.0};
  p.search.top_k = 16;
  p.search.min_sep_m = 0.9;
  p.search.min_sep_rad = 0.1308996938995747;
  return p;
}

// The resident descriptor table of a MapArray (host memory): update() computes the descriptors of the submaps added since the last
// call — a descriptor depends on its own cloud alone — in one launch and appends them.
struct ScanContextTable {
  lsr_scan_context_params params = scanContextDefaults();
  std::vector<float> descriptors;   // count x num_rings x num_sectors
  int count = 0;

  size_t cells() const { return (size_t)params.num_rings * (size_t)params.num_sectors; }

  // submaps: the whole MapArray so far (clouds of `layout`, host memory or HIP device pointers with clouds_on_device)
  bool update(lsr_handle h, const std::vector<lsr_submap>& submaps, const lsr_pc2_layout& layout = lsr_pc2_layout{32u, 0u, 4u, 8u, 16},
              bool clouds_on_device = false) {
    const int n = (int)submaps.size();
    if (n <= count) return true;
    descriptors.resize((size_t)n * cells());
    const int st = lsr_scan_context_build(h, submaps.data() + count, n - count, &layout, clouds_on_device ? 1 : 0, &params,
                                          descriptors.data() + (size_t)count * cells(), 0);
    if (st != LSR_OK) {
      std::fprintf(stderr, "[lidarslam_reg::ScanContextTable] %s: %s\n", lsr_status_string(st), lsr_last_error());
      descriptors.resize((size_t)count * cells());
      return false;
    }
    count = n;
    return true;
  }
};

// searchLoop by appearance: the evaluated candidates, most alike first, into `edges` (shifts / sc_dist beside them when given).
// false: refused or failed (reported on stderr), edges empty.
inline bool searchLoopAppearance(lsr_handle h, const std::vector<lsr_submap>& submaps, size_t stride_bytes, const ScanContextTable& table,
                                 const lsr_appearance_loop_params& params, std::vector<lsr_loop_edge>& edges,
                                 std::vector<int32_t>* shifts = nullptr, std::vector<float>* sc_dist = nullptr,
                                 bool clouds_on_device = false) {
  const int cap = params.loop.top_k > 1 ? params.loop.top_k : 1;
  edges.assign((size_t)cap, lsr_loop_edge{});
  std::vector<int32_t> sh((size_t)cap, 0);
  std::vector<float> sd((size_t)cap, 0.f);
  int n_eval = 0;
  const int st = lsr_search_loop_appearance(h, submaps.data(), (int)submaps.size(), stride_bytes, clouds_on_device ? 1 : 0,
                                            table.descriptors.data(), table.count, 0, &params, edges.data(), sh.data(), sd.data(), cap,
                                            &n_eval);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::searchLoopAppearance] %s: %s\n", lsr_status_string(st), lsr_last_error());
    edges.clear();
    return false;
  }
  edges.resize((size_t)n_eval);
  sh.resize((size_t)n_eval);
  sd.resize((size_t)n_eval);
  if (shifts) *shifts = sh;
  if (sc_dist) *sc_dist = sd;
  return true;
}

}  // namespace lidarslam_reg

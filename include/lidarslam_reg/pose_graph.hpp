// lidarslam_reg/pose_graph.hpp — header-only helper over lsr_pose_graph_edges / lsr_optimize_pose_graph_long (lidarslam_reg.h): the
// optimiser half of doPoseAdjustment on the device, without g2o.
//
//   graph_based_slam/src/graph_based_slam_component.cpp:267-319   g2o::SparseOptimizer, VertexSE3 / EdgeSE3, optimize(10)
//
// Needs neither g2o nor Eigen: a pose is anything whose .matrix().data() yields 16 column-major doubles, readable on a const object
// and writable on a mutable one (Eigen::Isometry3d, Eigen::Affine3d).  INTEGRATION.md §3f shows the call site with g2o removed.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../lidarslam_reg.h"

namespace lidarslam_reg {

namespace detail {
template <typename Pose>
inline std::vector<double> poses16(const std::vector<Pose>& poses) {
  std::vector<double> out(16 * poses.size());
  for (size_t i = 0; i < poses.size(); i++) {
    const auto& M = poses[i].matrix();
    std::memcpy(out.data() + 16 * i, M.data(), 16 * sizeof(double));
  }
  return out;
}
}  // namespace detail

// one EdgeSE3: vertices()[0] = from, vertices()[1] = to, setMeasurement(relative) with relative = from^-1 * to — a LoopEdge's
// pair_id.first, pair_id.second and relative_pose (:308-315)
template <typename Pose>
inline lsr_pose_edge poseEdge(int from, int to, const Pose& relative) {
  lsr_pose_edge e;
  e.from = from;
  e.to = to;
  const auto& M = relative.matrix();
  std::memcpy(e.measurement, M.data(), 16 * sizeof(double));
  return e;
}

// Appends the odometry edges doPoseAdjustment adds (:289-303): for every i > num_adjacent (strictly) and j = 0 .. num_adjacent - 1
// the edge (i - num_adjacent + j -> i) measured from `poses`.  Host only.
template <typename Pose>
inline bool adjacentPoseEdges(const std::vector<Pose>& poses, int num_adjacent, std::vector<lsr_pose_edge>& edges) {
  const std::vector<double> P = detail::poses16(poses);
  const size_t n = poses.size();
  const size_t want = (num_adjacent > 0 && n > (size_t)num_adjacent + 1) ? (n - (size_t)num_adjacent - 1) * (size_t)num_adjacent : 0;
  const size_t at = edges.size();
  edges.resize(at + want);
  size_t n_out = 0;
  const int st = lsr_pose_graph_edges(P.data(), (int)n, num_adjacent, edges.data() + at, want, &n_out);
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::adjacentPoseEdges] %s: %s\n", lsr_status_string(st), lsr_last_error());
    edges.resize(at);
    return false;
  }
  edges.resize(at + n_out);
  return true;
}

// optimizer.initializeOptimization(); optimizer.optimize(max_iterations) (:317-318): `poses` are the vertices' estimates (vertex 0
// fixed), `edges` the odometry edges followed by the loop edges; `optimized` receives vertex->estimate() of every vertex — what
// lidarslam_reg::assembleMap (map_assembly.hpp) takes as poses.  Reports like the registration adapter does (stderr, false) and leaves
// `optimized` as it was on failure.  Through lsr_optimize_pose_graph_long: up to LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES loop edges, so
// loop_edges_ may keep growing over a drive (:247); within LSR_POSE_GRAPH_MAX_OFFBAND_EDGES the bits are lsr_optimize_pose_graph's.
template <typename Pose>
inline bool optimizePoseGraph(lsr_handle h, const std::vector<Pose>& poses, const std::vector<lsr_pose_edge>& edges,
                              std::vector<Pose>& optimized, lsr_pose_graph_result* result = nullptr, int max_iterations = 10, int band = 5,
                              std::vector<lsr_pose_graph_trace>* trace = nullptr) {
  const std::vector<double> P = detail::poses16(poses);
  std::vector<double> out(P.size());
  std::vector<lsr_pose_graph_trace> tr((size_t)(max_iterations > 0 ? max_iterations : 0));
  lsr_pose_graph_params params = {max_iterations, band};
  lsr_pose_graph_result res;
  const int st = lsr_optimize_pose_graph_long(h, P.data(), (int)poses.size(), edges.data(), (int)edges.size(), &params, out.data(),
                                              &res, tr.empty() ? nullptr : tr.data());
  if (st != LSR_OK) {
    std::fprintf(stderr, "[lidarslam_reg::optimizePoseGraph] %s: %s\n", lsr_status_string(st), lsr_last_error());
    return false;
  }
  optimized = poses;
  for (size_t i = 0; i < optimized.size(); i++) {
    auto& M = optimized[i].matrix();
    std::memcpy(M.data(), out.data() + 16 * i, 16 * sizeof(double));
  }
  if (result) *result = res;
  if (trace) {
    tr.resize((size_t)res.iterations);
    trace->swap(tr);
  }
  return true;
}

}  // namespace lidarslam_reg

// NDT pose search (csrc/pose_search.hip): the score of the source at many candidate poses in one launch, the choice of the distinct
// best, and their refinement as one candidate set — lsr_ndt_score_poses, lsr_pose_lattice_poses, lsr_select_poses and
// lsr_ndt_search_pose of the C ABI (include/lidarslam_reg.h states the definitions).
#pragma once
#include "common.hpp"

namespace lsr {

constexpr int PS_THREADS = 512;          // lanes of a scoring workgroup: eight waves, one canonical chunk of 64 points per wave and trip
constexpr int PS_TILE = 16;              // candidate poses a workgroup owns, over ALL chunks of the source
constexpr int PS_BATCH = 8;              // candidates whose per-point terms go through a wave's staging tile together (2 rows each)
constexpr size_t PS_MAX_POSES = (size_t)LSR_POSE_SEARCH_MAX_POSES;

// Buffers of the scoring launch, kept on the object: reserved when first needed, never shrunk.
struct PoseSearchState {
  DevBuf<float> poses;     // the candidates' column-major 4x4 transforms
  DevBuf<double> out;      // score[count] | pairs[count]
  double ms = 0.0;         // LSR_POSE_SEARCH_MS: hipEvent time of the last call's scoring launches (LSR_PROFILE), else 0
};

}  // namespace lsr

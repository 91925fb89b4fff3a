// Moving objects out of the map (csrc/map_visibility.hip): a depth image per keyframe, its 3 x 3 erosion, one visibility vote per
// (record, neighbouring keyframe) and the map of the records with too few votes against them — lsr_visibility_pairs,
// lsr_depth_images_build, lsr_visibility_votes and lsr_assemble_map_static of the C ABI.  No reference site exists: the definition is
// this project's (unpinned), stated in include/lidarslam_reg.h and DESIGN.md §4.  It uses integer and single-rounded fp32 operations
// only; map_visibility.o is compiled with -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace lsr {

constexpr int VIS_THREADS = 256;
constexpr int VIS_BUILD_SLICE = 4096;   // records of one submap that one workgroup of the image build folds into the image
constexpr int VIS_PIECE_MIN = 256, VIS_PIECE_MAX = 1 << 30, VIS_PIECE_DEFAULT = 1 << 26;   // LSR_VISIBILITY_PIECE_BYTES
constexpr int VIS_CHUNK = 256;          // records per workgroup of the votes, the count and the write: one per thread

// One table entry per run of records of one submap (a submap, or the part of one that fits a staging piece).  The image build cuts
// it into slices of VIS_BUILD_SLICE records, the votes into slices of VIS_CHUNK: first_slice counts in the launch's own slices.
struct VisSlot {
  const unsigned char* records;   // device pointer
  long long first_out;            // the run's first record in assembly order (votes)
  int count;
  int first_slice;
  int submap;                     // index of the image (build) / of the pair list (votes) in the call's tables
  int pad;
};

// the constants of one parameter set as the kernels take them: made on the host in double, each rounded to float once
struct VisConsts {
  int W, H;                    // face_width, height
  float hw, Tf, rs;            // (float)(W / 2), (float)T, (float)(H / (2 T))
  float min_range, max_range, margin;
  float ox, oy, oz;            // sensor_origin
};
struct VisRecordLayout { int step, x, y, z; };   // byte offsets

struct VisibilityState {
  DevBuf<VisSlot> d_slots;
  PinBuf<VisSlot> h_slots;
  DevBuf<float> raw;          // D of an eroded build, on its way into the erosion
  DevBuf<float> images;       // images on their way to a host buffer (build), or staged host images (votes)
  DevBuf<int> first_pair, other;
  DevBuf<float> rel12;
  DevBuf<int> votes;          // votes on their way to a host buffer, or between the votes and the compaction
  DevBuf<int> counts;         // kept records per VIS_CHUNK | their exclusive prefix (one more entry: the total)
  DevBuf<long long> bounds;   // first raw record of every submap | kept records in front of it
  int piece_bytes = VIS_PIECE_DEFAULT;   // LSR_VISIBILITY_PIECE_BYTES: host clouds are staged that many bytes at a time
  double images_ms = 0.0, votes_ms = 0.0;   // LSR_DEPTH_IMAGES_MS / LSR_VISIBILITY_MS: hipEvent time of the last call's launches (LSR_PROFILE)
};

// params -> constants; LSR_ERR_INVALID_ARGUMENT with the reason in set_last_error
int visibility_consts(const lsr_visibility_params* p, VisConsts* C);

}  // namespace lsr

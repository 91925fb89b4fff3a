// The opaque handle behind the C ABI (one registration object = one pcl::Registration instance).
#pragma once
#include "common.hpp"
#include "deskew.hpp"
#include "gicp.hpp"
#include "map_filter.hpp"
#include "map_visibility.hpp"
#include "map_window.hpp"
#include "ndt.hpp"
#include "nn.hpp"
#include "pcd_deflate.hpp"
#include "pcd_read.hpp"
#include "pcd_text.hpp"
#include "pose_graph.hpp"
#include "pose_search.hpp"
#include "scan_context.hpp"

namespace lsr {
// A deferred stream dependency (round 6): the group launches of a candidate set run on the FIRST member's stream; instead of making
// every other member's own stream wait for them right away (one hipStreamWaitEvent per member and call, and one query + record + wait
// per member at the next group call: ~110 us of host time per share of eight), the members only remember the event.  A member's own
// stream waits for it when the member is next used on its own (LSR_CHECK_HANDLE); a group call on the SAME lead stream needs nothing.
struct StreamDep {
  hipEvent_t ev = nullptr;
  ~StreamDep() { if (ev) (void)hipEventDestroy(ev); }
};
}  // namespace lsr

struct lsr_handle_s {
  using NdtParamsHost = lsr::NdtParamsHost; using GicpParamsHost = lsr::GicpParamsHost; using TargetData = lsr::TargetData;
  using DeviceCloud = lsr::DeviceCloud; using HashGridDev = lsr::HashGridDev; using BuildScratch = lsr::BuildScratch;
  using NdtState = lsr::NdtState; using NdtProblem = lsr::NdtProblem; using GicpWorkspace = lsr::GicpWorkspace;
  template <typename T> using DevBuf = lsr::DevBuf<T>;
  template <typename T> using PinBuf = lsr::PinBuf<T>;
  int method = LSR_METHOD_NDT;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // profiling brackets (LSR_PROFILE)
  std::shared_ptr<lsr::StreamDep> dep;        // pending: `stream` must wait for dep->ev before this object's next launch of its own
  hipStream_t dep_stream = nullptr;           // ... the (lead) stream that event was recorded on
  std::shared_ptr<lsr::StreamDep> lead_dep;   // as the lead of a set: the event its members are handed
  // side stream of a batch lead: the neighbour grids of a candidate set are refined there while the shared NDT launch chain
  // runs on `stream` (align_ndt_batch); created on first use
  hipStream_t side_stream = nullptr;
  hipEvent_t side_ev = nullptr, side_fork_ev = nullptr;
  // extra launch-chain streams of a batch lead: a small candidate set runs as several independent chains (run_ndt_feeder)
  hipStream_t chain_stream[3] = {nullptr, nullptr, nullptr};
  hipEvent_t chain_ev[3] = {nullptr, nullptr, nullptr};
  hipEvent_t chain_fork_ev = nullptr;
  bool chain_probed = false;   // the streams above were looked for (each is verified to run concurrently with `stream`)
  int n_chain_streams = 0;

  NdtParamsHost ndt;
  GicpParamsHost gicp;
  double euclidean_fitness_eps = -1.7976931348623157e308;
  int num_threads = 0, ransac_iterations = 0;
  int profile = 0;
  int ndt_threads = 0;       // LSR_NDT_WORKGROUP: 0 = automatic; quad kernel: 64 / 128 points, lane kernel: 512 / 1024 threads
  int ndt_table_mode = -1;   // LSR_NDT_TABLE_MODE: -1 = automatic, else lsr::NdtTableMode
  int ndt_quad = -1;         // LSR_NDT_QUAD: -1 = automatic (single registrations: four lanes per point), 0 = lane kernel, 1 = four
  int ndt_split = -1;        // LSR_NDT_SPLIT: -1 = automatic, 0 / 1 = one / two waves per chunk in the 512-thread lane kernel (single registrations)

  std::shared_ptr<TargetData> target;
  std::shared_ptr<TargetData> spare_target;  // recycled by the next setInputTarget when no other handle shares it
  DeviceCloud source;
  DeviceCloud raw, filtered;  // N1: unfiltered upload / stand-alone filter result
  bool has_source = false;
  bool source_cov_valid = false;
  DevBuf<double> source_cov;  // GICP
  HashGridDev source_hash;    // GICP (20-NN over the source itself)

  BuildScratch scratch;
  DevBuf<unsigned char> staging;
  PinBuf<float> out_xyz;      // align(output): packed transformed xyz on their way into the caller's records

  // NDT run-time buffers (batch-capable: the leader of a batch owns arrays for all members)
  DevBuf<NdtState> d_state;
  DevBuf<long long> d_bins;   // NDT_NBANKS banks of int64 accumulators per registration (exact chunk sums, ndt.hip: canon)
  DevBuf<NdtProblem> d_prob;
  PinBuf<NdtState> h_state;
  PinBuf<NdtProblem> h_prob;
  const NdtState* h_state_dev = nullptr;   // device views of the two pinned arrays (the chain's init launch reads them, ndt_init_batch)
  const NdtProblem* h_prob_dev = nullptr;
  PinBuf<lsr::NdtMailbox> mailbox;        // host-coherent, mapped: progress + result of a single registration
  lsr::NdtMailbox* d_mailbox = nullptr;   // device view of mailbox.p
  unsigned int align_token = 0;
  DevBuf<float> d_T16;
  DevBuf<float> d_poses;  // N2: keyframe poses
  DevBuf<lsr::FrameSlot> d_frames;   // N2, one-launch assembly: the window's frame table ...
  PinBuf<lsr::FrameSlot> h_frames;   // ... and the pinned copy it is uploaded from
  DevBuf<lsr::MapSlot> d_map_slots;  // N5, lsr_assemble_map: the submap table of one launch ...
  PinBuf<lsr::MapSlot> h_map_slots;  // ... and the pinned copy it is uploaded from
  DevBuf<unsigned char> map_out;     // N5: a piece of the map on its way to a host buffer
  int map_form = 0;                  // LSR_MAP_ASSEMBLY_FORM: 0 = none yet, 1 = wide, 2 = general
  double map_ms = 0.0;               // LSR_MAP_ASSEMBLY_MS: hipEvent time of the last call's launches (LSR_PROFILE), else 0

  GicpWorkspace gicp_ws;

  lsr::DeskewState deskew;   // IMU queue and de-skew scratch (use_imu frontend path, csrc/deskew.hip)

  lsr::PgWorkspace pose_graph;   // lsr_optimize_pose_graph (csrc/pose_graph.hip): device buffers, kept between calls

  lsr::PcdState pcd;   // lsr_format_pcd_ascii / lsr_save_pcd_ascii / lsr_save_map_pcd_ascii (csrc/pcd_text.hip): buffers, kept between calls

  lsr::PcdDeflateState pcd_deflate;   // lsr_format_pcd / lsr_save_pcd / lsr_save_map_pcd (csrc/pcd_deflate.hip): image, slots, stream; kept between calls

  lsr::PcdReadState pcd_read;  // lsr_decode_pcd / lsr_load_pcd / lsr_set_input_target_pcd (csrc/pcd_read.hip): buffers, kept between calls

  lsr::MapFilterState map_filter;   // lsr_voxel_grid_filter_map / lsr_assemble_map_filtered / lsr_save_map_pcd_filtered (csrc/map_filter.hip): scratch, kept between calls

  lsr::MapWindowState map_window;   // lsr_crop_map / lsr_set_input_target_window (csrc/map_window.hip): scratch, kept between calls

  lsr::PoseSearchState pose_search;   // lsr_ndt_score_poses / lsr_ndt_search_pose (csrc/pose_search.hip): pose and score buffers, kept between calls

  lsr::ScanContextState scan_context;   // lsr_scan_context_build / _match / lsr_search_loop_appearance (csrc/scan_context.hip): tables and staged descriptors, kept between calls

  lsr::VisibilityState visibility;   // lsr_depth_images_build / lsr_visibility_votes / lsr_assemble_map_static (csrc/map_visibility.hip): tables, staged images, votes; kept between calls

  // worker objects of lsr_search_loop(top_k > 1) and lsr_ndt_search_pose: one per candidate registered in the same launch chain
  std::vector<std::unique_ptr<lsr_handle_s>> aux;

  float final_T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  int converged = 0;
  lsr_profile prof = {0, 0, 0, 0};
};


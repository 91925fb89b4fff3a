// IMU de-skew of a raw PointCloud2 payload on the device (csrc/deskew.hip): what a handle keeps for it.
#pragma once
#include "common.hpp"
#include "deskew_point.hpp"
#include "imu_queue.hpp"

namespace lsr {

// Control block of one de-skew call.  It travels to the device in front of the IMU table (one copy from pinned memory), so every
// call starts from these initial values without a memset of its own.
struct DeskewCtl {
  unsigned int half_index;   // K1: min{i : flag_i} by atomicMin; starts as 0xFFFFFFFF (none)
  unsigned int n_skipped;    // K4: points left untouched because no IMU sample is within scan_period
  int cursor;                // K4: table entry the pointer ends on (c_{n-1})
  int m;                     // table entries (without entry -1)
  float start, end, diff;    // K1: start_ori, end_ori, ori_diff
  int start_missing;         // K2: point 0 is skipped -> no point is moved
  DeskewPose start_pose;     // K2: rpy / shift / velo of point 0 ...
  float Rs[9];               // ... and its rotation (row-major; applied transposed)
  int pad[2];
};
struct DeskewUpload {
  DeskewCtl ctl;
  ImuEntry table[IMU_TABLE_MAX];   // table[0] = entry -1, table[1 + k] = entry k
};
static_assert(sizeof(DeskewCtl) % 8 == 0, "the table behind the control block holds doubles");

// what a call hands back to the host: written straight into host-coherent memory by the last launch, token last
struct DeskewMailbox {
  int cursor, n_skipped, start_missing, half_index;
  unsigned int token;
};

struct DeskewState {
  ImuQueue imu;
  PinBuf<DeskewUpload> h_up;
  DevBuf<DeskewUpload> d_up;
  PinBuf<DeskewMailbox> mb;
  DeskewMailbox* d_mb = nullptr;
  unsigned int token = 0;
  // per point, kept until the next call (lsr_deskew_trace): rel_time, table entry the pointer stood on, skipped
  DevBuf<float> rel;
  DevBuf<int> code, entry;
  DevBuf<unsigned char> skipped;
  DevBuf<int> block_max;
  size_t trace_n = 0;        // points of the last call that reached the device (0: it returned early)
  int trace_base = 0;        // ring slot of table entry 0 in that call
};

constexpr int DESKEW_WG = 256;   // points per workgroup, one per thread

// Enqueues the de-skew of n records on `stream` and waits for its mailbox (no device-to-host copy, no stream synchronisation).
// d_in / d_out: device pointers, equal (in place) or disjoint.  The table and the control block come from S.h_up (filled by the caller).
int deskew_run(DeskewState& S, const void* d_in, void* d_out, size_t n, int step, int ox, int oy, int oz, double scan_time,
               int wait_mode, hipStream_t stream);

}  // namespace lsr

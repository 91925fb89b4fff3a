// Scan Context: a place descriptor per keyframe and its comparison at every yaw shift, on the device (csrc/scan_context.hip), for the
// appearance loop gate lsr_search_loop_appearance (csrc/loop_search.hip).  No reference site exists — the reference picks loop
// candidates by their drifted position alone —: the definitions are this project's (unpinned), stated in include/lidarslam_reg.h and
// DESIGN.md §4.  They use integer and single-rounded fp32 operations only; scan_context.o is compiled with -ffp-contract=off.
#pragma once
#include "common.hpp"

namespace lsr {

constexpr int SC_MAX_RINGS = LSR_SCAN_CONTEXT_MAX_RINGS;
constexpr int SC_MAX_SECTORS = LSR_SCAN_CONTEXT_MAX_SECTORS;
constexpr int SC_BUILD_THREADS = 256;
constexpr int SC_SLICE = 4096;          // records of one submap that one workgroup folds into its LDS maxima
constexpr int SC_MATCH_THREADS = 128;   // >= SC_MAX_SECTORS: one lane per shift

// One table entry per run of records with one descriptor (a submap, or the part of one that fits a staging piece): the workgroups
// first_slice .. first_slice + ceil(count / SC_SLICE) - 1 of the launch fold it.
struct ScSlot {
  const unsigned char* records;   // device pointer
  int count;
  int first_slice;
  int desc;                       // index of the descriptor in the launch's output
  int pad;
};

// the tables of one parameter set as the kernels take them: edge2[0 .. R-2] the squared ring edges k = 1 .. R-1, edge2[R-1] = L2;
// boundary[2 (k-1)], [2 (k-1) + 1] = cos, sin of 2 pi k / S for k = 1 .. S/2-1
struct ScTables {
  int R, S;
  float z_offset;
  float edge2[SC_MAX_RINGS];
  float boundary[SC_MAX_SECTORS];   // 2 (S/2 - 1) <= SC_MAX_SECTORS - 2 entries
};
struct ScRecordLayout { int step, x, y, z; };   // byte offsets

struct ScanContextState {
  DevBuf<ScSlot> d_slots;
  PinBuf<ScSlot> h_slots;
  DevBuf<float> desc;        // descriptors on their way to a host buffer (build), or staged host descriptors (match: queries)
  DevBuf<float> cand;        // staged host descriptors (match: candidates)
  DevBuf<float> dist;        // match results on their way to the host
  DevBuf<int> shift;
  double build_ms = 0.0, match_ms = 0.0;   // LSR_SCAN_CONTEXT_BUILD_MS / _MATCH_MS: hipEvent time of the last call's launches (LSR_PROFILE)
};

// params -> tables (host, double, each entry rounded to float once); LSR_ERR_INVALID_ARGUMENT with the reason in set_last_error
int scan_context_tables(const lsr_scan_context_params* p, ScTables* T);
// one launch over a table of n_slots entries with n_slices workgroups; d_desc (n_desc x R x S floats) has been zeroed by the caller —
// the launch only raises cells (unsigned maxima on the float bits), so several launches may share one output
int scan_context_build(const ScSlot* d_slots, int n_slots, int n_slices, const ScTables& T, const ScRecordLayout& L, float* d_desc,
                       hipStream_t stream);
// nq x nc pairs in one launch: d_dist / d_shift [q * nc + c]
int scan_context_match(const float* d_q, int nq, const float* d_c, int nc, int R, int S, float* d_dist, int* d_shift, hipStream_t stream);

}  // namespace lsr

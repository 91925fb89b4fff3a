// What the host units behind the C ABI share (capi.hip, handle_ops.hip, ndt_align.hip, inputs.hip, loop_search.hip, map_output.hip):
// the handle check every entry starts with, the argument checks several entries repeat, and the functions that cross a unit boundary.
// Host only — no kernel unit includes this header.
#pragma once
#include "handle.hpp"

#define LSR_CHECK_HANDLE(h)                      \
  if (!(h)) {                                    \
    ::lsr::set_last_error("null handle");        \
    return LSR_ERR_INVALID_ARGUMENT;             \
  }                                              \
  ::lsr::DeviceGuard _guard((h)->device);        \
  if (!_guard.ok) {                              \
    ::lsr::set_last_error("hipSetDevice failed"); \
    return LSR_ERR_HIP;                          \
  }                                              \
  if ((h)->dep && ::lsr::settle_dep(h)) return LSR_ERR_HIP;

namespace lsr {

// ---- handle_ops.hip: deferred stream dependencies (handle.hpp: StreamDep) and the life of a target object
int settle_dep(lsr_handle h);
int defer_members_behind(lsr_handle lead, lsr_handle* members, int count);
int order_lead_after(hipStream_t lead, lsr_handle h);
std::shared_ptr<TargetData> fresh_target(lsr_handle h);
bool target_is_shared(lsr_handle h);
int ensure_ndt_grid(lsr_handle h);
bool hash_from_grid_possible(lsr_handle h);
int ensure_target_hash(lsr_handle h);

// ---- ndt_align.hip: the NDT host driver (what gicp_align / gicp_align_batch are for GICP, gicp.hpp)
int align_ndt_batch(lsr_handle_s** hs, int B, const float* guesses, float* finals, lsr_result* results, double* fitness_out = nullptr,
                    double max_range = 1.7976931348623157e308);

// ---- inputs.hip
int assemble_frames(lsr_handle h, int n_frames, const void* const* frames, const size_t* counts, size_t stride_bytes, const float* poses16,
                    bool on_device, DeviceCloud& out);
int check_layout(const lsr_pc2_layout* L);

// ---- loop_search.hip
void submap_pose_matrix(const lsr_submap& s, double M[16]);

// whatever was enqueued on the stream has finished before the scope is left: the object's staging buffers and the caller's buffers are free again
struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } };

// the record stride of a strided xyz cloud
inline int check_stride(size_t stride) {
  if (stride < 12 || (stride % 4) != 0) {
    set_last_error("stride_bytes must be a multiple of 4 and >= 12");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  return LSR_OK;
}

// Member b of a batch call against the members before it: not null, on the first member's device (same_method: of its method too) and,
// with `unique`, not listed before (an object has ONE workspace, mailbox and result).
inline int check_batch_member(lsr_handle_s* const* hs, int b, bool same_method, bool unique) {
  if (!hs[b]) { set_last_error("null handle"); return LSR_ERR_INVALID_ARGUMENT; }
  if (hs[b]->device != hs[0]->device) { set_last_error("batched objects must live on one device"); return LSR_ERR_INVALID_ARGUMENT; }
  if (same_method && hs[b]->method != hs[0]->method) { set_last_error("batched handles must share device and method"); return LSR_ERR_INVALID_ARGUMENT; }
  for (int a = 0; unique && a < b; a++)
    if (hs[a] == hs[b]) { set_last_error("the same object appears twice in the batch"); return LSR_ERR_INVALID_ARGUMENT; }
  return LSR_OK;
}
inline int check_batch_members(lsr_handle_s* const* hs, int count, bool same_method, bool unique) {
  for (int b = 0; b < count; b++)
    if (int st = check_batch_member(hs, b, same_method, unique)) return st;
  return LSR_OK;
}

}  // namespace lsr

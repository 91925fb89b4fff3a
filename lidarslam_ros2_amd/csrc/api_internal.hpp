// What the host units behind the C ABI share (capi.hip, handle_ops.hip, ndt_align.hip, inputs.hip, sensor_frame.hip, loop_search.hip,
// map_output.hip, pcd_input.hip and the C ABI at the bottom of deskew.hip, map_filter.hip and scan_context.hip): the handle check every entry
// starts with, the argument
// checks of record_args.hpp reported through set_last_error, the staging of host records on their way in and out, and the functions
// that cross a unit boundary.
// Host code only, and none of it does floating-point arithmetic: a unit that holds kernels may include this header (deskew.hip does)
// whatever its -ffp-contract rule (Makefile), and what is inline here is the same code in every unit.  It must stay that way — a
// function with floating-point arithmetic belongs in ONE unit, under that unit's rule.
#pragma once
#include "handle.hpp"
#include "record_args.hpp"

// the first part alone: for the entries that touch no device (the IMU ring: lsr_imu_push at IMU rate on the callback thread)
#define LSR_CHECK_HANDLE_NOT_NULL(h)             \
  if (!(h)) {                                    \
    ::lsr::set_last_error("null handle");        \
    return LSR_ERR_INVALID_ARGUMENT;             \
  }
#define LSR_CHECK_HANDLE(h)                      \
  LSR_CHECK_HANDLE_NOT_NULL(h)                   \
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

// the problem record and table mode (lsr::NdtTableMode; tab_bytes: the LDS image's size in that mode, else 0) of a pose-scoring launch
int ndt_score_problem(lsr_handle_s* h, int other_lds, NdtProblem* P, int* tab, int* tab_bytes);

// ---- inputs.hip
int assemble_frames(lsr_handle h, int n_frames, const void* const* frames, const size_t* counts, size_t stride_bytes, const float* poses16,
                    bool on_device, DeviceCloud& out);

// ---- loop_search.hip
void submap_pose_matrix(const lsr_submap& s, double M[16]);

// whatever was enqueued on the stream has finished before the scope is left: the object's staging buffers and the caller's buffers are free again
struct StreamDrain { hipStream_t s; ~StreamDrain() { (void)hipStreamSynchronize(s); } };

// ---- record_args.hpp through set_last_error: "<argument>: <what is wrong with it>"
inline int arg_error(const ArgStatus& a) {
  if (a) set_last_error(std::string(a.what) + ": " + a.why);
  return a.status;
}
inline int check_stride(size_t stride) { return arg_error(check_stride_arg(stride)); }
inline int check_layout(const lsr_pc2_layout* L, const char* what = "layout") { return arg_error(check_layout_arg(L, what)); }
inline int check_out_layout(const lsr_pc2_layout* L) { return arg_error(check_out_layout_arg(L)); }

// ---- staging: host records on their way to a kernel and back (h->staging; the copies are enqueued, nothing here waits but stage_out)
// Records the next launch on `stream` reads -> *d_records.  Device records are read where they are.  Host records are copied to byte
// `at` of h->staging, which the caller has reserved for everything it stages side by side (reserving again would move the pieces
// already there), and the staged copy is read.
inline int stage_in_at(lsr_handle h, const void* records, size_t bytes, bool on_device, hipStream_t stream, size_t at, const void** d_records) {
  *d_records = records;
  if (on_device) return LSR_OK;
  if (at + bytes > h->staging.cap) { set_last_error("staging: a piece outside the reserved buffer"); return LSR_ERR_INVALID_ARGUMENT; }
  *d_records = h->staging.p + at;
  if (bytes > 0) LSR_HIP(hipMemcpyAsync(h->staging.p + at, records, bytes, hipMemcpyHostToDevice, stream));
  return LSR_OK;
}
// the same for an entry that stages one piece: reserves the buffer itself
inline int stage_in(lsr_handle h, const void* records, size_t bytes, bool on_device, hipStream_t stream, const void** d_records) {
  if (!on_device)
    if (int st = h->staging.reserve(bytes)) return st;
  return stage_in_at(h, records, bytes, on_device, stream, 0, d_records);
}
// A result of `bytes` bytes on its way to host memory: write(d) enqueues on the object's stream whatever fills d = h->staging.p (clear:
// zeroed first — the writer leaves the bytes between its fields alone); then the copy to host_dst, and the stream is synchronised.
template <class Writer>
int stage_out(lsr_handle h, void* host_dst, size_t bytes, bool clear, Writer&& write) {
  int st = h->staging.reserve(bytes);
  if (st) return st;
  if (clear) LSR_HIP(hipMemsetAsync(h->staging.p, 0, bytes, h->stream));
  if ((st = write(h->staging.p))) return st;
  LSR_HIP(hipMemcpyAsync(host_dst, h->staging.p, bytes, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  return LSR_OK;
}
// The bracket of a records -> records entry (lsr_transform_pc2, lsr_deskew_pc2) behind check_records_in_out: run(d_in, d_out) enqueues
// the entry's launches.  Device records: run alone, on the caller's buffers — the entry decides how it returns.  Host records: staged in,
// run in place on the staged copy, copied to out_data, synchronised.
template <class Run>
int records_in_records_out(lsr_handle h, const void* data, void* out_data, size_t bytes, bool on_device, Run&& run) {
  if (on_device) return run(data, out_data);
  const void* d_in = nullptr;
  if (int st = stage_in(h, data, bytes, false, h->stream, &d_in)) return st;
  return stage_out(h, out_data, bytes, false, [&](unsigned char* d) { return run(d, d); });
}

// a bracket of two events, the second of which has completed: its time added to *ms (LSR_PROFILE)
inline int add_ms(hipEvent_t a, hipEvent_t b, double* ms) {
  float t = 0.f;
  LSR_HIP(hipEventElapsedTime(&t, a, b));
  *ms += t;
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

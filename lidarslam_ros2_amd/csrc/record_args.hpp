// The pure argument checks of the C ABI entries that take a buffer of records — strided xyz clouds or PointCloud2 payloads, on the host
// or on the device (include/lidarslam_reg.h).  No HIP, no handle, no state: this header needs the public header and the standard library
// only, so the checks are compiled and run by a plain host test (tests/cpp/record_args_harness.cpp).  A check returns the status and
// what to say; the entries report it through arg_error (api_internal.hpp).
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/lidarslam_reg.h"

namespace lsr {

// status == LSR_OK: the argument is fine; else `what` names the offending argument and `why` says what is wrong with it
struct ArgStatus {
  int status;
  const char* what;
  const char* why;
  explicit operator bool() const { return status != LSR_OK; }
};
inline ArgStatus arg_ok() { return {LSR_OK, nullptr, nullptr}; }
inline ArgStatus arg_invalid(const char* what, const char* why) { return {LSR_ERR_INVALID_ARGUMENT, what, why}; }

// The most records one call takes.  Two limits, and they answer differently:
//   the ingest, transform and de-skew entries index their records (and four fields of each) with int32: INVALID_ARGUMENT above half of it;
//   the map and PCD entries count records in int32 and address bytes in 64 bits: INDEX_OVERFLOW above all of it.
struct RecordLimit {
  size_t max_records;
  int status;
  const char* why;
};
constexpr RecordLimit INGEST_RECORD_LIMIT{(size_t)INT32_MAX / 2, LSR_ERR_INVALID_ARGUMENT, "cloud too large (more than INT32_MAX / 2 records)"};
constexpr RecordLimit MAP_RECORD_LIMIT{(size_t)INT32_MAX, LSR_ERR_INDEX_OVERFLOW, "more than INT32_MAX records"};

// the record stride of a strided xyz cloud
inline ArgStatus check_stride_arg(size_t stride, const char* what = "stride_bytes") {
  if (stride < 12 || (stride % 4) != 0) return arg_invalid(what, "must be a multiple of 4 and >= 12");
  return arg_ok();
}

// ---- PointCloud2 layouts ---------------------------------------------------------------------------------------------------------
// point_step and the x / y / z offsets: all an entry needs that copies every other byte of a record as it is (lsr_deskew_pc2)
inline ArgStatus check_layout_xyz(const lsr_pc2_layout* L, const char* what = "layout") {
  if (!L) return arg_invalid(what, "null PointCloud2 layout");
  if (L->point_step < 12 || (L->point_step % 4) != 0) return arg_invalid(what, "point_step must be a multiple of 4 and >= 12");
  const uint32_t offs[3] = {L->offset_x, L->offset_y, L->offset_z};
  for (uint32_t o : offs)
    if ((o % 4) != 0 || (uint64_t)o + 4 > L->point_step) return arg_invalid(what, "x/y/z offsets must be 4-byte aligned and inside point_step");
  return arg_ok();
}
// ... and the intensity field, for the entries that read or write it
inline ArgStatus check_layout_arg(const lsr_pc2_layout* L, const char* what = "layout") {
  if (ArgStatus a = check_layout_xyz(L, what)) return a;
  if (L->offset_intensity >= 0 && ((L->offset_intensity % 4) != 0 || (uint64_t)L->offset_intensity + 4 > L->point_step))
    return arg_invalid(what, "intensity offset must be 4-byte aligned and inside point_step (or < 0 for none)");
  return arg_ok();
}
// ... and, for a layout that is WRITTEN field by field, no two fields at one offset
inline ArgStatus check_out_layout_arg(const lsr_pc2_layout* L, const char* what = "out_layout") {
  if (ArgStatus a = check_layout_arg(L, what)) return a;
  const int64_t f[4] = {(int64_t)L->offset_x, (int64_t)L->offset_y, (int64_t)L->offset_z,
                        L->offset_intensity >= 0 ? (int64_t)L->offset_intensity : (int64_t)-1};
  for (int a = 0; a < 4; a++)
    for (int b = a + 1; b < 4; b++)
      if (f[a] >= 0 && f[a] == f[b]) return arg_invalid(what, "output fields overlap");
  return arg_ok();
}

// ---- record buffers --------------------------------------------------------------------------------------------------------------
inline ArgStatus check_record_count(size_t n, const RecordLimit& limit, const char* what) {
  if (n > limit.max_records) return {limit.status, what, limit.why};
  return arg_ok();
}
// A buffer of n records: a pointer where there are records, on a 4-byte boundary where the entry demands one (align4: the records ->
// records, map and PCD entries do, of host and device buffers alike and whatever n is; the ingest entries never have), no more records
// than the entry's limit.
inline ArgStatus check_records(const void* p, size_t n, const RecordLimit& limit, bool align4, const char* what) {
  if (n > 0 && !p) return arg_invalid(what, "null pointer with records to read or write");
  if (align4 && (reinterpret_cast<uintptr_t>(p) & 3) != 0) return arg_invalid(what, "must be 4-byte aligned");
  return check_record_count(n, limit, what);
}

inline bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a_bytes > 0 && b_bytes > 0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
// a records -> records entry writes where it reads (in place) or somewhere else entirely: its kernel copies records workgroup by workgroup
inline ArgStatus check_in_place_or_disjoint(const void* in, const void* out, size_t bytes, const char* what = "data and out_data") {
  if (in != out && ranges_overlap(in, bytes, out, bytes)) return arg_invalid(what, "overlap: they must be equal (in place) or disjoint");
  return arg_ok();
}
// both buffers of such an entry: n records of `step` bytes read at `data`, written at `out_data`
inline ArgStatus check_records_in_out(const void* data, const void* out_data, size_t n, size_t step) {
  if (ArgStatus a = check_records(data, n, INGEST_RECORD_LIMIT, true, "data")) return a;
  if (ArgStatus a = check_records(out_data, n, INGEST_RECORD_LIMIT, true, "out_data")) return a;
  return check_in_place_or_disjoint(data, out_data, n * step);
}

// ---- map windows -----------------------------------------------------------------------------------------------------------------
// a leaf size > 0 (NaN refused) and, per axis, lo <= hi with both cells below 2^24 in magnitude ((float) of a cell is exact there)
constexpr int64_t WINDOW_CELL_LIMIT = (int64_t)1 << 24;
inline ArgStatus check_window_arg(const lsr_map_window* w, const char* what = "window") {
  if (!w) return arg_invalid(what, "null map window");
  if (!(w->leaf > 0)) return arg_invalid(what, "the leaf size must be > 0");
  for (int k = 0; k < 3; k++) {
    if (w->lo[k] > w->hi[k]) return arg_invalid(what, "lo[k] > hi[k]");
    const int64_t lo = w->lo[k], hi = w->hi[k];
    if (lo <= -WINDOW_CELL_LIMIT || lo >= WINDOW_CELL_LIMIT || hi <= -WINDOW_CELL_LIMIT || hi >= WINDOW_CELL_LIMIT)
      return arg_invalid(what, "a cell of 2^24 or beyond (a float coordinate carries no leaf resolution there)");
  }
  return arg_ok();
}

// ---- frame lists -----------------------------------------------------------------------------------------------------------------
// n_frames clouds of one stride with a pose each (lsr_set_input_target_frames and what shares its assembly); -> the records in all and
// in the biggest frame
inline ArgStatus check_frame_list(int n_frames, const void* const* frames, const size_t* counts, size_t stride_bytes, const void* poses16,
                                  size_t* total_out = nullptr, size_t* biggest_out = nullptr) {
  if (n_frames <= 0) return arg_invalid("n_frames", "bad frame list: no frames");
  if (!frames || !counts || !poses16) return arg_invalid("frames / counts / poses16", "bad frame list: null array");
  if (ArgStatus a = check_stride_arg(stride_bytes)) return a;
  size_t total = 0, biggest = 0;
  for (int f = 0; f < n_frames; f++) {
    if (ArgStatus a = check_records(frames[f], counts[f], INGEST_RECORD_LIMIT, false, "frames[]")) return a;
    total += counts[f];   // (cannot wrap: every count is below 2^30 and there are fewer than 2^31 of them)
    if (counts[f] > biggest) biggest = counts[f];
  }
  if (ArgStatus a = check_record_count(total, INGEST_RECORD_LIMIT, "frames[]")) return a;
  if (total_out) *total_out = total;
  if (biggest_out) *biggest_out = biggest;
  return arg_ok();
}

}  // namespace lsr

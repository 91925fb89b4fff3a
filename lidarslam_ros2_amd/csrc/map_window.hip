// Localising in a saved map: the records inside a box of voxel cells cut out of the resident map, in input order —
// lsr_map_window_around, lsr_crop_map and lsr_set_input_target_window of the C ABI (include/lidarslam_reg.h states the definition).
// setInputTarget lays one int32 cell table over the bounding box of what it is given (grid_build.hip: ndt_grid_geometry); a map is
// kilometres, a scan reaches a hundred metres.  The cut touches no registration kernel: the voxel lattice is anchored at the origin
// (voxel_device.hpp: leaf_axis subtracts an INTEGER min_b behind the floor), so a window of whole cells holds, cell by cell, the
// points the whole-map grid holds there, in the same order.
//
// The chain of one call, on the object's stream — three launches, and no workgroup waits for another:
//   the kept records of every 256 counted (in_window, voxel_device.hpp) ->
//   the counts scanned by ONE workgroup of MW_SCAN_WIDTH threads, each over ceil(workgroups / 1024) counts in a row; the total goes to
//   the builders' host mailbox (common.hpp: BuildMailbox value / value_token): the ONE host wait, it sizes the output ->
//   every record judged again by the same helper and, if kept, ranked among its workgroup's kept ones (ballot and popcount within a
//   wave, the waves' totals through LDS: run_rank_in_block) and written at that rank.
// Two forms of the count and of the write with the same bytes, as in cloud_codec.hip's assemble_map: wide — {32; 0,4,8,16} records on
// 16-byte boundaries, 16-byte loads and stores — and general, field by field.
// Arithmetic: one float multiply and a floor per coordinate, nothing a contraction could fuse (built with -ffp-contract=off all the
// same: lsr_map_window_around below does the same multiply and floor on the host).
#include "map_window.hpp"

#include <algorithm>
#include <cmath>

#include "api_internal.hpp"
#include "sort.hpp"
#include "voxel_device.hpp"

namespace lsr {
namespace {

// x, y, z of record i; WIDE: one 16-byte load
template <bool WIDE>
__device__ __forceinline__ void mw_xyz(const unsigned char* __restrict__ data, const MfFields& F, size_t i, float& x, float& y, float& z) {
  if (WIDE) {
    const uint4 a = *reinterpret_cast<const uint4*>(data + i * 32);
    x = __uint_as_float(a.x); y = __uint_as_float(a.y); z = __uint_as_float(a.z);
  } else {
    const unsigned char* rec = data + i * (size_t)F.step;
    x = record_field(rec, F.ox); y = record_field(rec, F.oy); z = record_field(rec, F.oz);
  }
}

// counts[workgroup] = the records among its MW_CHUNK that the window keeps
template <bool WIDE>
__global__ __launch_bounds__(256) void mw_count_kernel(const unsigned char* __restrict__ data, MfFields F, size_t n, float inv_leaf,
                                                       WindowCells W, int* __restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * MW_CHUNK + threadIdx.x;
  bool keep = false;
  if (i < n) {
    float x, y, z;
    mw_xyz<WIDE>(data, F, i, x, y, z);
    keep = in_window(x, y, z, inv_leaf, W);
  }
  const int c = flags_in_block(keep);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// one workgroup: base[b] = counts[0] + .. + counts[b - 1] for b = 0 .. nb (base[nb]: the total, which also goes to the host mailbox)
__global__ __launch_bounds__(MW_SCAN_WIDTH) void mw_scan_kernel(const int* __restrict__ counts, int nb, int* __restrict__ base,
                                                                BuildMailbox* __restrict__ mb, unsigned int token) {
  __shared__ int s_w[MW_SCAN_WIDTH / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (nb + MW_SCAN_WIDTH - 1) / MW_SCAN_WIDTH;
  const int b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
  int cnt = 0;
  for (int b = b0; b < b1; b++) cnt += counts[b];
  int inc = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int run = inc - cnt;
  for (int w = 0; w < wave; w++) run += s_w[w];
  for (int b = b0; b < b1; b++) { const int t = counts[b]; base[b] = run; run += t; }
  if (tid == MW_SCAN_WIDTH - 1) {   // owns the last (possibly empty) slice: run == the total
    base[nb] = run;
    mb->value = run;
    __threadfence_system();
    __hip_atomic_store(&mb->value_token, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// the kept records written in input order: record i goes to rank base[workgroup] + (kept ones in front of it in the workgroup)
template <bool WIDE>
__global__ __launch_bounds__(256) void mw_write_kernel(const unsigned char* __restrict__ data, MfFields F, size_t n, float inv_leaf,
                                                       WindowCells W, const int* __restrict__ base, unsigned char* __restrict__ out,
                                                       MfFields O) {
  const size_t i = (size_t)blockIdx.x * MW_CHUNK + threadIdx.x;
  bool keep = false;
  float x = 0.f, y = 0.f, z = 0.f;
  if (i < n) {
    mw_xyz<WIDE>(data, F, i, x, y, z);
    keep = in_window(x, y, z, inv_leaf, W);
  }
  const int r = run_rank_in_block(keep, base);
  if (!keep) return;
  if (WIDE) {
    const uint4 b = *reinterpret_cast<const uint4*>(data + i * 32 + 16);
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)r * 32);
    o[0] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
    o[1] = make_uint4(b.x, 0u, 0u, 0u);
  } else {
    const unsigned int vi = F.oi >= 0 ? *reinterpret_cast<const unsigned int*>(data + i * (size_t)F.step + F.oi) : 0u;
    unsigned int* o = reinterpret_cast<unsigned int*>(out + (size_t)r * (size_t)O.step);
    const int wx = O.ox / 4, wy = O.oy / 4, wz = O.oz / 4, wi = O.oi >= 0 ? O.oi / 4 : -1;
    for (int w = 0; w < O.step / 4; w++) {
      unsigned int v = 0u;
      if (w == wx) v = __float_as_uint(x);
      else if (w == wy) v = __float_as_uint(y);
      else if (w == wz) v = __float_as_uint(z);
      else if (w == wi) v = vi;
      o[w] = v;
    }
  }
}

}  // namespace

int mw_scan_counts(BuildScratch& sc, hipStream_t stream, const int* counts, int nb, int* base, unsigned int* token) {
  if (int st = sc.ensure_mailbox()) return st;
  unsigned int t = ++sc.token;
  if (t == 0) t = ++sc.token;
  hipLaunchKernelGGL(mw_scan_kernel, dim3(1), dim3(MW_SCAN_WIDTH), 0, stream, counts, nb, base, sc.d_mb, t);
  LSR_HIP(hipGetLastError());
  *token = t;
  return LSR_OK;
}

namespace {

MfFields mw_fields(const lsr_pc2_layout* L) {
  return MfFields{(int)L->point_step, (int)L->offset_x, (int)L->offset_y, (int)L->offset_z, L->offset_intensity >= 0 ? (int)L->offset_intensity : -1};
}
bool mw_is_xyzi(const MfFields& F) { return F.step == 32 && F.ox == 0 && F.oy == 4 && F.oz == 8 && F.oi == 16; }
bool mw_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct MwCut {
  const unsigned char* d_in;
  size_t n;
  MfFields F;
  bool wide_in;   // the input alone allows 16-byte loads
  float inv_leaf;
  WindowCells W;
  int nb;         // workgroups of the count and of the write
};

// First half: count and scan enqueued, the count awaited (the ONE host wait).  d_in: n > 0 records of F in device memory.
int mw_count(lsr_handle h, const void* d_in, size_t n, const MfFields& F, const lsr_map_window* w, MwCut* C, size_t* kept) {
  MapWindowState& S = h->map_window;
  BuildScratch& sc = h->scratch;
  C->d_in = static_cast<const unsigned char*>(d_in);
  C->n = n;
  C->F = F;
  C->wide_in = mw_is_xyzi(F) && mw_aligned16(d_in);
  C->inv_leaf = 1.0f / w->leaf;
  for (int k = 0; k < 3; k++) { C->W.lo[k] = (float)w->lo[k]; C->W.hi[k] = (float)w->hi[k]; }
  C->nb = (int)((n + MW_CHUNK - 1) / MW_CHUNK);
  int st;
  if ((st = S.counts.reserve(2 * (size_t)C->nb + 1))) return st;
  if (h->profile && (st = S.ensure_events())) return st;
  unsigned int token = 0;
  int* counts = S.counts.p;
  int* base = counts + C->nb;
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[0], h->stream));
  if (C->wide_in)
    hipLaunchKernelGGL(mw_count_kernel<true>, dim3(C->nb), dim3(256), 0, h->stream, C->d_in, F, n, C->inv_leaf, C->W, counts);
  else
    hipLaunchKernelGGL(mw_count_kernel<false>, dim3(C->nb), dim3(256), 0, h->stream, C->d_in, F, n, C->inv_leaf, C->W, counts);
  LSR_HIP(hipGetLastError());
  if ((st = mw_scan_counts(sc, h->stream, counts, C->nb, base, &token))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[1], h->stream));
  int total = 0;
  if ((st = sorted_runs_count(sc, h->stream, token, &total))) return st;
  if (total < 0 || (size_t)total > n) { set_last_error("map window: the count is outside its bounds"); return LSR_ERR_HIP; }
  *kept = (size_t)total;
  return LSR_OK;
}

// Second half: the `kept` records of layout O written at d_out (device memory with room for them).  Enqueued, not waited for.
int mw_write(lsr_handle h, const MwCut& C, void* d_out, const MfFields& O) {
  MapWindowState& S = h->map_window;
  const int* base = S.counts.p + C.nb;
  unsigned char* out = static_cast<unsigned char*>(d_out);
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[2], h->stream));
  if (C.wide_in && mw_is_xyzi(O) && mw_aligned16(d_out))
    hipLaunchKernelGGL(mw_write_kernel<true>, dim3(C.nb), dim3(256), 0, h->stream, C.d_in, C.F, C.n, C.inv_leaf, C.W, base, out, O);
  else
    hipLaunchKernelGGL(mw_write_kernel<false>, dim3(C.nb), dim3(256), 0, h->stream, C.d_in, C.F, C.n, C.inv_leaf, C.W, base, out, O);
  LSR_HIP(hipGetLastError());
  if (h->profile) LSR_HIP(hipEventRecord(S.ev[3], h->stream));
  return LSR_OK;
}

// the brackets read back: the stream is synchronised first
int mw_collect_ms(lsr_handle h, bool written) {
  MapWindowState& S = h->map_window;
  S.ms = 0.0;
  if (!h->profile) return LSR_OK;
  LSR_HIP(hipStreamSynchronize(h->stream));
  int st = add_ms(S.ev[0], S.ev[1], &S.ms);
  if (!st && written) st = add_ms(S.ev[2], S.ev[3], &S.ms);
  return st;
}

// what lsr_crop_map and lsr_set_input_target_window check alike
int mw_check_in(const void* data, size_t n_points, const lsr_pc2_layout* in_layout, const lsr_map_window* w) {
  int st = check_layout(in_layout, "in_layout");
  if (st || (st = arg_error(check_window_arg(w, "w")))) return st;
  return arg_error(check_records(data, n_points, MAP_RECORD_LIMIT, true, "data"));
}

const lsr_pc2_layout MW_XYZI = {32, 0, 4, 8, 16};   // pcl::PointXYZI, what map_ptr holds

}  // namespace
}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_map_window_around(const double center[3], const double half_extent[3], float leaf, lsr_map_window* w) {
  if (!center || !half_extent || !w) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if (!(leaf > 0)) { set_last_error("leaf: the leaf size must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
  const float inv_leaf = 1.0f / leaf;
  lsr_map_window out;
  out.leaf = leaf;
  for (int k = 0; k < 3; k++) {
    if (!std::isfinite(center[k]) || !std::isfinite(half_extent[k]) || half_extent[k] < 0) {
      set_last_error("center / half_extent: not finite, or a negative half extent");
      return LSR_ERR_INVALID_ARGUMENT;
    }
    const float a = (float)(center[k] - half_extent[k]), b = (float)(center[k] + half_extent[k]);
    const float lo = std::floor(a * inv_leaf), hi = std::floor(b * inv_leaf);
    if (!(std::fabs(lo) < (float)MW_CELL_LIMIT) || !(std::fabs(hi) < (float)MW_CELL_LIMIT)) {
      set_last_error("map window: a cell of 2^24 or beyond (a float coordinate carries no leaf resolution there)");
      return LSR_ERR_INDEX_OVERFLOW;
    }
    out.lo[k] = (int32_t)lo;
    out.hi[k] = (int32_t)hi;
  }
  *w = out;
  return LSR_OK;
}

int lsr_crop_map(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout, int on_device, const lsr_map_window* w,
                 void* out_data, size_t capacity_points, const lsr_pc2_layout* out_layout, int out_on_device, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!n_out) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = mw_check_in(data, n_points, in_layout, w);
  if (st || (st = check_out_layout(out_layout)) || (st = arg_error(check_records(out_data, 0, MAP_RECORD_LIMIT, true, "out_data")))) return st;
  const bool in_host = on_device == 0, out_host = out_on_device == 0;
  // (the output never holds more records than the input: the part of the buffer that can be written)
  if (out_data && in_host == out_host &&
      ranges_overlap(out_data, std::min(capacity_points, n_points) * out_layout->point_step, data, n_points * in_layout->point_step)) {
    set_last_error("the output range overlaps the input records");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  h->map_window.ms = 0.0;
  if (n_points == 0) { *n_out = 0; return LSR_OK; }
  // whatever was enqueued has finished before the call returns: the staging buffer and the caller's buffers are free again
  StreamDrain drain{h->stream};
  const void* d = nullptr;
  if ((st = stage_in(h, data, n_points * in_layout->point_step, !in_host, h->stream, &d))) return st;
  MwCut C;
  size_t kept = 0;
  if ((st = mw_count(h, d, n_points, mw_fields(in_layout), w, &C, &kept))) return st;
  if (!out_data || kept == 0) {
    if ((st = mw_collect_ms(h, false))) return st;
    *n_out = kept;
    return LSR_OK;
  }
  if (capacity_points < kept) {
    *n_out = kept;
    set_last_error("output buffer too small");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  const size_t out_bytes = kept * (size_t)out_layout->point_step;
  void* d_out = out_data;
  if (out_host) {
    if ((st = h->map_out.reserve(out_bytes))) return st;
    d_out = h->map_out.p;
  }
  if ((st = mw_write(h, C, d_out, mw_fields(out_layout)))) return st;
  if (out_host) LSR_HIP(hipMemcpyAsync(out_data, d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if ((st = mw_collect_ms(h, true))) return st;
  *n_out = kept;
  return LSR_OK;
}

int lsr_set_input_target_window(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout, int on_device,
                                const lsr_map_window* w, size_t* n_kept) {
  LSR_CHECK_HANDLE(h);
  if (!n_kept) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = mw_check_in(data, n_points, in_layout, w);
  if (st) return st;
  h->map_window.ms = 0.0;
  // whatever was enqueued has finished before the call returns; in front of the target build the count is the only host wait (the
  // build reads the cut in stream order, and stages nothing: its input is on the device)
  StreamDrain drain{h->stream};
  size_t kept = 0;
  MwCut C;
  const void* d = nullptr;
  if (n_points > 0) {
    if ((st = stage_in(h, data, n_points * in_layout->point_step, on_device != 0, h->stream, &d)) ||
        (st = mw_count(h, d, n_points, mw_fields(in_layout), w, &C, &kept)))
      return st;
  }
  if (kept == 0) {
    if (n_points > 0 && (st = mw_collect_ms(h, false))) return st;
    *n_kept = 0;
    set_last_error("w: the window keeps no record of the map (the previous target stays)");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if ((st = h->map_window.records.reserve(kept * MW_XYZI.point_step)) || (st = mw_write(h, C, h->map_window.records.p, mw_fields(&MW_XYZI))) ||
      (st = mw_collect_ms(h, true)))
    return st;
  if ((st = lsr_set_input_target_device(h, h->map_window.records.p, MW_XYZI.point_step, kept))) return st;
  *n_kept = kept;
  return LSR_OK;
}

}  // extern "C"

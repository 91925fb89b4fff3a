// pcl::VoxelGrid over a whole map, records in and records out, the leaf index in 64 bits: lsr_voxel_grid_filter_map,
// lsr_assemble_map_filtered and lsr_save_map_pcd_filtered of the C ABI (include/lidarslam_reg.h states the definition).
// ScanMatcherComponent::publishMap (scanmatcher_component.cpp:529-552) and the map half of doPoseAdjustment
// (graph_based_slam_component.cpp:321-369) hand on the raw concatenation of the submaps; this thins it with a leaf size before it
// is published or saved.
//
// The chain of one call, on the object's stream:
//   bounding box of the finite points over the records (one launch; the workgroups' records are copied to the host: WAIT 1) -> the
//   host folds them, refuses what is beyond the limits and decides the key width ->
//   key words (low into the sort's buffer; for an index of more than 32 bits low and high kept aside) ->
//   sort_pairs_u32_lsd on the low word with implicit iota values; for a wide index the high words gathered through that order and
//   sorted stably on their bits_for(cells) - 32 bits with the order as the value, then the low words gathered through the final order ->
//   run heads per 256-key chunk over (high, low) pairs, exclusive scan (exclusive_scan_i32_lsd), the leaf count copied to the host:
//   WAIT 2 (it sizes the output) ->
//   centroids (one thread per head, float sums in ascending input index, four gathers in flight) -> the output records, word by word.
// Arithmetic: one float multiply per coordinate, a floor, a float subtraction (exact below MF_CELL_LIMIT), float additions in index
// order and one float division per field: nothing a contraction could fuse (the unit is built with -ffp-contract=off all the same).
// That arithmetic, the box fold and the run walk are the int32 filter's own text (voxel_device.hpp), instantiated here over records,
// (high, low) key words and int64 products.
#include "map_filter.hpp"

#include <algorithm>
#include <cmath>

#include "api_internal.hpp"
#include "sort.hpp"
#include "voxel_device.hpp"

namespace lsr {

namespace {

constexpr int MF_CHUNK = 256;   // sorted keys per workgroup of the run finder and of the centroids: one per thread

// per workgroup {min xyz, max xyz, finite points, -} of the finite points it walked (float bits): parts[8 * workgroup + k]
__global__ __launch_bounds__(256) void mf_bbox_kernel(const unsigned char* __restrict__ data, int step, int ox, int oy, int oz, size_t n,
                                                      unsigned int* __restrict__ parts) {
  BoxAcc box;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += 4 * stride) {   // four records per trip in flight
    float p[4][3];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const size_t i = i0 + u * stride;
      if (i < n) {
        const unsigned char* rec = data + i * (size_t)step;
        p[u][0] = record_field(rec, ox); p[u][1] = record_field(rec, oy); p[u][2] = record_field(rec, oz);
      } else {
        p[u][0] = p[u][1] = p[u][2] = NAN;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) box.add(p[u][0], p[u][1], p[u][2]);
  }
  box_publish(box_fold_block(box), nullptr, 0u, nullptr, parts + (size_t)blockIdx.x * 8);
}

// The leaf index of every record, as voxel_grid_filter forms it (voxel_device.hpp: leaf_key) with the products in int64; a record
// with a non-finite coordinate gets `cells`, one past the last index.  lo_sort: the low word where the sort reads it; for a wide
// index (hi_keep != null) both words are also kept where the sort does not write.
__global__ __launch_bounds__(256) void mf_key_kernel(const unsigned char* __restrict__ data, int step, int ox, int oy, int oz, size_t n,
                                                     float inv_leaf, int mb0, int mb1, int mb2, long long mul1, long long mul2,
                                                     unsigned long long cells, unsigned int* __restrict__ lo_sort,
                                                     unsigned int* __restrict__ lo_keep, unsigned int* __restrict__ hi_keep) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned char* rec = data + i * (size_t)step;
  const unsigned long long k =
      leaf_key<long long>(record_field(rec, ox), record_field(rec, oy), record_field(rec, oz), inv_leaf, mb0, mb1, mb2, mul1, mul2, cells);
  lo_sort[i] = (unsigned int)k;
  if (hi_keep) { lo_keep[i] = (unsigned int)k; hi_keep[i] = (unsigned int)(k >> 32); }
}

// out[j] = src[order[j]]: the high words through the order of the low-word sort, then the low words through the final order
__global__ __launch_bounds__(256) void mf_gather_kernel(const unsigned int* __restrict__ src, const int* __restrict__ order, size_t n,
                                                        unsigned int* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j < n) out[j] = src[order[j]];
}

// heads of the runs of equal (high, low) pairs per chunk of MF_CHUNK sorted keys; workgroup 0 also zeroes the closing entry
// block_heads[gridDim.x], whose exclusive prefix is the number of runs
__global__ __launch_bounds__(256) void mf_heads_kernel(const unsigned int* __restrict__ lo, const unsigned int* __restrict__ hi, size_t n,
                                                       int* __restrict__ block_heads) {
  const int c = run_heads_in_block(KeysHiLo{lo, hi}, (size_t)blockIdx.x * MF_CHUNK + threadIdx.x, n);
  if (threadIdx.x == 0) {
    block_heads[blockIdx.x] = c;
    if (blockIdx.x == 0) block_heads[gridDim.x] = 0;
  }
}

// Every head sums its run: the walk, the additions and the division of rs_centroid_kernel (lsd_sort.hip; voxel_device.hpp:
// run_centroid), the records read where they lie.  Run r in key order -> cx/cy/cz/cw[r]; the run of the non-finite records
// (key == cells, always last) is dropped.
__global__ __launch_bounds__(256) void mf_centroid_kernel(const unsigned int* __restrict__ lo, const unsigned int* __restrict__ hi,
                                                          const int* __restrict__ order, size_t n, const int* __restrict__ block_base,
                                                          unsigned long long cells, int has_sentinel, const unsigned char* __restrict__ data,
                                                          int step, int ox, int oy, int oz, int oi, float* __restrict__ cx,
                                                          float* __restrict__ cy, float* __restrict__ cz, float* __restrict__ cw) {
  const KeysHiLo K{lo, hi};
  const size_t i = (size_t)blockIdx.x * MF_CHUNK + threadIdx.x;
  const bool head = (i < n) && run_is_head(K, i);
  const int r = run_rank_in_block(head, block_base);
  if (!head) return;
  const unsigned long long key = K.at(i);
  if (has_sentinel && key == cells) return;
  float c[4];
  run_centroid(K, key, RecordPoints{data, step, ox, oy, oz, oi}, order, i, n, c);
  cx[r] = c[0]; cy[r] = c[1]; cz[r] = c[2]; cw[r] = c[3];
}

// the output records, one 4-byte word per thread: a field's word takes its plane's value, every other word is zero
__global__ __launch_bounds__(256) void mf_write_kernel(const float* __restrict__ cx, const float* __restrict__ cy, const float* __restrict__ cz,
                                                       const float* __restrict__ cw, size_t n_out, int words_per_record, int wx, int wy,
                                                       int wz, int wi, unsigned int* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_out * (size_t)words_per_record) return;
  const size_t r = t / (size_t)words_per_record;
  const int w = (int)(t - r * (size_t)words_per_record);
  unsigned int v = 0u;
  if (w == wx) v = __float_as_uint(cx[r]);
  else if (w == wy) v = __float_as_uint(cy[r]);
  else if (w == wz) v = __float_as_uint(cz[r]);
  else if (w == wi) v = __float_as_uint(cw[r]);
  out[t] = v;
}

int mf_limit_error(const char* what) {
  set_last_error(what);
  return LSR_ERR_INDEX_OVERFLOW;
}

unsigned int mf_blocks(size_t n) { return (unsigned int)((n + 255) / 256); }

}  // namespace

int map_filter_runs(MapFilterState& S, const void* d_records, size_t n, const MfFields& F, float leaf, hipStream_t stream, bool profile,
                    MfPlan* P) {
  *P = MfPlan{};
  P->n = n;
  for (double& v : S.ms) v = 0.0;
  if (n == 0) return LSR_OK;
  int st;
  const unsigned char* data = static_cast<const unsigned char*>(d_records);
  const int nb_box = (int)std::max<size_t>(1, std::min<size_t>((n + 1023) / 1024, MF_BBOX_MAX_BLOCKS));
  if ((st = S.parts.reserve((size_t)MF_BBOX_MAX_BLOCKS * 8)) || (st = S.h_parts.reserve((size_t)MF_BBOX_MAX_BLOCKS * 8 + 8))) return st;
  if (profile && (st = S.ensure_events())) return st;

  // ---- bounding box of the finite points: WAIT 1
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_BBOX], stream));
  hipLaunchKernelGGL(mf_bbox_kernel, dim3(nb_box), dim3(256), 0, stream, data, F.step, F.ox, F.oy, F.oz, n, S.parts.p);
  LSR_HIP(hipGetLastError());
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_BBOX + 1], stream));
  LSR_HIP(hipMemcpyAsync(S.h_parts.p, S.parts.p, (size_t)nb_box * 8 * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
  LSR_HIP(hipStreamSynchronize(stream));
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  unsigned long long n_finite = 0;
  for (int b = 0; b < nb_box; b++) {
    const unsigned int* g = S.h_parts.p + (size_t)b * 8;
    if (g[6] == 0u) continue;
    n_finite += g[6];
    for (int k = 0; k < 3; k++) {
      float lo, hi;
      std::memcpy(&lo, &g[k], 4);
      std::memcpy(&hi, &g[3 + k], 4);
      mn[k] = std::fmin(mn[k], lo);
      mx[k] = std::fmax(mx[k], hi);
    }
  }
  P->n_finite = (unsigned int)n_finite;
  if (n_finite == 0) { S.key_bits = 0; return LSR_OK; }

  // ---- the grid, and what is beyond it
  const float inv_leaf = 1.0f / leaf;
  const GridDims G = grid_dims(mn, mx, inv_leaf);
  unsigned long long cells = 1;
  for (int k = 0; k < 3; k++) {
    if (!(std::fabs(G.cell_lo[k]) < (float)MF_CELL_LIMIT) || !(std::fabs(G.cell_hi[k]) < (float)MF_CELL_LIMIT))
      return mf_limit_error("map filter: a cell coordinate reaches 2^24 (a float coordinate carries no leaf resolution there): leaf size too small for where the cloud lies");
    P->min_b[k] = G.min_b[k];
    P->div_b[k] = G.div_b[k];
    if (P->div_b[k] > MF_DIV_LIMIT)
      return mf_limit_error("map filter: more than 2^21 cells along an axis: leaf size too small for the cloud extent");
    cells *= (unsigned long long)P->div_b[k];
  }
  P->cells = cells;
  P->index_bits = bits_for(cells - 1);
  const bool has_sentinel = n_finite < (unsigned long long)n;
  P->sort_bits = has_sentinel ? bits_for(cells) : P->index_bits;
  const bool wide = P->sort_bits > 32;
  S.key_bits = P->index_bits;

  // ---- scratch: key_a | key_b | val_a | val_b | lo_keep | hi_keep | block_heads[nb + 1] | block_base[nb + 1]
  const size_t nb = (n + MF_CHUNK - 1) / MF_CHUNK;
  if ((st = S.words.reserve((wide ? 6 : 4) * n + 2 * (nb + 1)))) return st;
  unsigned int* key_a = S.words.p;
  unsigned int* key_b = key_a + n;
  int* val_a = reinterpret_cast<int*>(key_b + n);
  int* val_b = val_a + n;
  unsigned int* lo_keep = wide ? reinterpret_cast<unsigned int*>(val_b + n) : nullptr;
  unsigned int* hi_keep = wide ? lo_keep + n : nullptr;
  int* block_heads = reinterpret_cast<int*>(S.words.p + (wide ? 6 : 4) * n);
  int* block_base = block_heads + nb + 1;

  // ---- keys
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_KEY], stream));
  hipLaunchKernelGGL(mf_key_kernel, dim3(mf_blocks(n)), dim3(256), 0, stream, data, F.step, F.ox, F.oy, F.oz, n, inv_leaf, P->min_b[0],
                     P->min_b[1], P->min_b[2], (long long)P->div_b[0], (long long)P->div_b[0] * P->div_b[1], cells, key_a, lo_keep, hi_keep);
  LSR_HIP(hipGetLastError());
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_KEY + 1], stream));

  // ---- sort: the low word, then (wide) the high word through the low word's order
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_SORT], stream));
  bool in_b = false;
  if ((st = sort_pairs_u32_lsd(key_a, key_b, nullptr, val_a, val_b, n, std::min(32, P->sort_bits), S.temp, stream, &in_b))) return st;
  const unsigned int* lo_sorted = in_b ? key_b : key_a;
  const unsigned int* hi_sorted = nullptr;
  int* order = in_b ? val_b : val_a;
  if (wide) {
    // the sorted low words are not needed as such (they are gathered again through the final order): both key buffers are free
    unsigned int* h_in = in_b ? key_a : key_b;
    unsigned int* h_other = in_b ? key_b : key_a;
    int* v_other = in_b ? val_a : val_b;
    hipLaunchKernelGGL(mf_gather_kernel, dim3(mf_blocks(n)), dim3(256), 0, stream, hi_keep, order, n, h_in);
    LSR_HIP(hipGetLastError());
    bool hi_in_b = false;
    if ((st = sort_pairs_u32_lsd(h_in, h_other, order, order, v_other, n, P->sort_bits - 32, S.temp, stream, &hi_in_b))) return st;
    unsigned int* hs = hi_in_b ? h_other : h_in;
    unsigned int* lo_out = hi_in_b ? h_in : h_other;   // the side of the ping-pong the last pass did not write
    order = hi_in_b ? v_other : order;
    hipLaunchKernelGGL(mf_gather_kernel, dim3(mf_blocks(n)), dim3(256), 0, stream, lo_keep, order, n, lo_out);
    LSR_HIP(hipGetLastError());
    hi_sorted = hs;
    lo_sorted = lo_out;
  }
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_SORT + 1], stream));

  // ---- runs: heads per chunk, their exclusive prefix, the total to the host: WAIT 2
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_RUNS], stream));
  hipLaunchKernelGGL(mf_heads_kernel, dim3((unsigned int)nb), dim3(256), 0, stream, lo_sorted, hi_sorted, n, block_heads);
  LSR_HIP(hipGetLastError());
  if ((st = exclusive_scan_i32_lsd(block_heads, block_base, nb + 1, S.temp, stream))) return st;
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_RUNS + 1], stream));
  unsigned int* h_total = S.h_parts.p + (size_t)MF_BBOX_MAX_BLOCKS * 8;
  LSR_HIP(hipMemcpyAsync(h_total, block_base + nb, sizeof(int), hipMemcpyDeviceToHost, stream));
  LSR_HIP(hipStreamSynchronize(stream));
  const long long runs = (long long)(int)*h_total - (has_sentinel ? 1 : 0);
  if (runs <= 0 || (unsigned long long)runs > n_finite) { set_last_error("map filter: the run count is outside its bounds"); return LSR_ERR_HIP; }
  P->lo = lo_sorted;
  P->hi = hi_sorted;
  P->order = order;
  P->block_base = block_base;
  P->n_leaves = (size_t)runs;
  return LSR_OK;
}

int map_filter_emit(MapFilterState& S, const void* d_records, const MfFields& F, const MfPlan& P, void* d_out, const MfFields& out,
                    hipStream_t stream, bool profile) {
  if (P.n_leaves == 0) return LSR_OK;
  int st;
  const size_t m = P.n_leaves;
  if ((st = S.centroids.reserve(4 * m))) return st;
  float* cx = S.centroids.p;
  const size_t nb = (P.n + MF_CHUNK - 1) / MF_CHUNK;
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_CENTROID], stream));
  hipLaunchKernelGGL(mf_centroid_kernel, dim3((unsigned int)nb), dim3(256), 0, stream, P.lo, P.hi, P.order, P.n, P.block_base, P.cells,
                     (size_t)P.n_finite < P.n ? 1 : 0, static_cast<const unsigned char*>(d_records), F.step, F.ox, F.oy, F.oz, F.oi, cx, cx + m,
                     cx + 2 * m, cx + 3 * m);
  LSR_HIP(hipGetLastError());
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_CENTROID + 1], stream));
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_WRITE], stream));
  const int wpr = out.step / 4;
  hipLaunchKernelGGL(mf_write_kernel, dim3(mf_blocks(m * (size_t)wpr)), dim3(256), 0, stream, cx, cx + m, cx + 2 * m, cx + 3 * m, m, wpr,
                     out.ox / 4, out.oy / 4, out.oz / 4, out.oi >= 0 ? out.oi / 4 : -1, static_cast<unsigned int*>(d_out));
  LSR_HIP(hipGetLastError());
  if (profile) LSR_HIP(hipEventRecord(S.ev[2 * MF_LEG_WRITE + 1], stream));
  return LSR_OK;
}

int map_filter_collect_ms(MapFilterState& S, bool emitted) {
  if (!S.have_events) return LSR_OK;
  const int legs = emitted ? (int)MF_LEGS : (int)MF_LEG_CENTROID;
  for (int k = 0; k < legs; k++) {
    float t = 0.f;
    LSR_HIP(hipEventElapsedTime(&t, S.ev[2 * k], S.ev[2 * k + 1]));
    S.ms[k] = t;
  }
  return LSR_OK;
}

}  // namespace lsr

using namespace lsr;

namespace {

constexpr size_t MF_SORT_LIMIT = (size_t)INT32_MAX / 2;   // what sort_pairs_u32_lsd orders in one call

MfFields mf_fields(const lsr_pc2_layout* L) {
  return MfFields{(int)L->point_step, (int)L->offset_x, (int)L->offset_y, (int)L->offset_z, L->offset_intensity >= 0 ? (int)L->offset_intensity : -1};
}

int mf_check_leaf(float leaf) {
  if (!(leaf > 0)) { set_last_error("leaf: the leaf size must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
  return LSR_OK;
}

int mf_check_out(const void* out_data, const lsr_pc2_layout* out_layout) {
  if (int st = check_out_layout(out_layout)) return st;
  return arg_error(check_records(out_data, 0, MAP_RECORD_LIMIT, true, "out_data"));   // (null: the count alone)
}

// n records of layout F in DEVICE memory at d_in thinned into device memory: the runs, then (unless count_only, or no leaf) the m records
// of layout O emitted, the stream synchronised and the legs' times collected.  They go to d_out (room for `capacity` records) or,
// d_out null, into `grow`, reserved to fit; h_out non-null: copied on to host memory in front of the synchronisation.  *m_out: the
// leaves, set on success and when the buffer is too small.
int mf_thin(lsr_handle h, const void* d_in, size_t n, const MfFields& F, float leaf, const MfFields& O, bool count_only, void* d_out,
            size_t capacity, DevBuf<unsigned char>* grow, void* h_out, size_t* m_out) {
  MapFilterState& S = h->map_filter;
  if (n > MF_SORT_LIMIT) { set_last_error("map filter: more than INT32_MAX / 2 records (the sort's limit)"); return LSR_ERR_INDEX_OVERFLOW; }
  const bool profile = h->profile != 0;
  MfPlan P;
  int st = map_filter_runs(S, d_in, n, F, leaf, h->stream, profile, &P);
  if (st) return st;
  const size_t m = P.n_leaves;
  if (count_only || m == 0) {
    if (profile && P.n_finite > 0 && (st = map_filter_collect_ms(S, false))) return st;
    *m_out = m;
    return LSR_OK;
  }
  if (capacity < m) {
    *m_out = m;
    set_last_error("output buffer too small");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  const size_t out_bytes = m * (size_t)O.step;
  if (!d_out) {
    if ((st = grow->reserve(out_bytes))) return st;
    d_out = grow->p;
  }
  if ((st = map_filter_emit(S, d_in, F, P, d_out, O, h->stream, profile))) return st;
  if (h_out) LSR_HIP(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (profile && (st = map_filter_collect_ms(S, true))) return st;
  *m_out = m;
  return LSR_OK;
}

// the same for the entries that hand out records: out_data in host or device memory (null: count only).  The arguments have been
// checked.  *n_out as lsr_voxel_grid_filter_map sets it.
int mf_filter_device(lsr_handle h, const void* d_in, size_t n, const lsr_pc2_layout* in_layout, float leaf, void* out_data,
                     size_t capacity_points, const lsr_pc2_layout* out_layout, bool out_on_device, size_t* n_out) {
  return mf_thin(h, d_in, n, mf_fields(in_layout), leaf, mf_fields(out_layout), !out_data, out_on_device ? out_data : nullptr, capacity_points,
                 &h->map_out, out_on_device ? nullptr : out_data, n_out);
}

int mf_count_submaps(const lsr_submap* submaps, int num_submaps, size_t* total_out) {
  size_t total = 0;
  int st;
  for (int i = 0; i < num_submaps; i++)   // (the size of the map buffer; lsr_assemble_map checks the clouds themselves)
    if ((st = arg_error(check_record_count(submaps[i].n_points, MAP_RECORD_LIMIT, "submaps[].n_points"))) ||
        (st = arg_error(check_record_count(total += submaps[i].n_points, MAP_RECORD_LIMIT, "submaps[] (the whole map)"))))
      return st;
  *total_out = total;
  return LSR_OK;
}

const lsr_pc2_layout MF_XYZI = {32, 0, 4, 8, 16};   // pcl::PointXYZI, what map_ptr holds

}  // namespace

extern "C" {

int lsr_voxel_grid_filter_map(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout, int on_device, float leaf,
                              void* out_data, size_t capacity_points, const lsr_pc2_layout* out_layout, int out_on_device, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!n_out) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_layout(in_layout, "in_layout");
  if (st || (st = mf_check_out(out_data, out_layout)) || (st = mf_check_leaf(leaf))) return st;
  if ((st = arg_error(check_records(data, n_points, MAP_RECORD_LIMIT, true, "data")))) return st;
  const bool in_host = on_device == 0, out_host = out_on_device == 0;
  // (the output never holds more records than the input: the part of the buffer that can be written)
  if (out_data && in_host == out_host &&
      ranges_overlap(out_data, std::min(capacity_points, n_points) * out_layout->point_step, data, n_points * in_layout->point_step)) {
    set_last_error("the output range overlaps the input records");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (n_points == 0) { *n_out = 0; return LSR_OK; }
  // whatever was enqueued has finished before the call returns: the staging buffer and the caller's buffers are free again
  StreamDrain drain{h->stream};
  const void* d = nullptr;
  if ((st = stage_in(h, data, n_points * in_layout->point_step, !in_host, h->stream, &d))) return st;
  return mf_filter_device(h, d, n_points, in_layout, leaf, out_data, capacity_points, out_layout, !out_host, n_out);
}

int lsr_assemble_map_filtered(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout, int on_device,
                              const double* poses16, float leaf, void* out_data, size_t capacity_points, const lsr_pc2_layout* out_layout,
                              int out_on_device, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!submaps || num_submaps <= 0 || !n_out) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_layout(in_layout, "in_layout");
  if (st || (st = mf_check_out(out_data, out_layout)) || (st = mf_check_leaf(leaf))) return st;
  size_t total = 0;
  if ((st = mf_count_submaps(submaps, num_submaps, &total))) return st;
  if (out_data && (on_device == 0) == (out_on_device == 0))
    for (int i = 0; i < num_submaps; i++)
      if (ranges_overlap(out_data, std::min(capacity_points, total) * out_layout->point_step, submaps[i].cloud,
                         submaps[i].n_points * in_layout->point_step)) {
        set_last_error("the output range overlaps an input cloud");
        return LSR_ERR_INVALID_ARGUMENT;
      }
  // the raw map, pcl::PointXYZI records kept on the object (the buffer of lsr_save_map_pcd), then the filter from it
  if ((st = h->pcd.map.reserve(std::max<size_t>(total, 1) * MF_XYZI.point_step))) return st;
  size_t n = 0;
  if ((st = lsr_assemble_map(h, submaps, num_submaps, in_layout, on_device, poses16, h->pcd.map.p, total, &MF_XYZI, 1, nullptr, &n))) return st;
  if (n == 0) { *n_out = 0; return LSR_OK; }
  StreamDrain drain{h->stream};
  return mf_filter_device(h, h->pcd.map.p, n, &MF_XYZI, leaf, out_data, capacity_points, out_layout, out_on_device != 0, n_out);
}

int lsr_save_map_pcd_filtered(lsr_handle h, const char* path, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout,
                              int on_device, const double* poses16, float leaf, int data_kind, size_t* n_points, size_t* n_bytes) {
  LSR_CHECK_HANDLE(h);
  if (!path || !n_bytes || !submaps || num_submaps <= 0) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if (data_kind != LSR_PCD_ASCII && data_kind != LSR_PCD_BINARY && data_kind != LSR_PCD_BINARY_COMPRESSED) {
    set_last_error("data_kind: not LSR_PCD_ASCII, LSR_PCD_BINARY or LSR_PCD_BINARY_COMPRESSED");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  int st = check_layout(in_layout, "in_layout");
  if (st || (st = mf_check_leaf(leaf))) return st;
  size_t total = 0;
  if ((st = mf_count_submaps(submaps, num_submaps, &total))) return st;
  if (total == 0) { set_last_error("submaps[]: an empty map has no PCD file"); return LSR_ERR_INVALID_ARGUMENT; }
  if ((st = h->pcd.map.reserve(total * MF_XYZI.point_step))) return st;
  size_t n = 0, m = 0;
  if ((st = lsr_assemble_map(h, submaps, num_submaps, in_layout, on_device, poses16, h->pcd.map.p, total, &MF_XYZI, 1, nullptr, &n))) return st;
  MapFilterState& S = h->map_filter;
  {
    StreamDrain drain{h->stream};
    const MfFields F = mf_fields(&MF_XYZI);
    if ((st = mf_thin(h, h->pcd.map.p, n, F, leaf, F, false, nullptr, SIZE_MAX, &S.thin, nullptr, &m))) return st;
    if (m == 0) { set_last_error("submaps[]: a map without a finite point has no PCD file"); return LSR_ERR_INVALID_ARGUMENT; }
  }
  size_t bytes = 0;
  if ((st = lsr_save_pcd(h, path, S.thin.p, m, &MF_XYZI, 1, data_kind, &bytes))) return st;
  if (n_points) *n_points = m;
  *n_bytes = bytes;
  return LSR_OK;
}

}  // extern "C"

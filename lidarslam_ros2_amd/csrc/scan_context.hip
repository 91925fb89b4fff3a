// Scan Context on the device: the place descriptor of every submap of a table in one launch, and nq x nc descriptor pairs compared
// at every yaw shift in one launch.  The C ABI on top (lsr_scan_context_tables / _build / _match; the appearance gate that uses them
// is in loop_search.hip) is at the bottom.  include/lidarslam_reg.h and DESIGN.md §4 state the definition; what matters here:
//   every fp32 result is ONE rounded operation on rounded inputs (this unit is compiled with -ffp-contract=off, and hipcc's divide and
//   square root are correctly rounded), so a numpy float32 restatement (tests/scan_context_numpy.py) has the same bits;
//   a descriptor cell is a maximum, and a maximum does not depend on the order of its points: cells are raised with unsigned integer
//   maxima on the float bits (the values are >= +0, where the two orders agree), first in LDS, then in the output;
//   the sums of a comparison run in the order the definition fixes (rings ascending inside a column, columns ascending), one lane per
//   shift, sequentially — not a tree.
#include <cmath>

#include "api_internal.hpp"
#include "scan_context.hpp"

using namespace lsr;

namespace lsr {
namespace {

// ---- build ---------------------------------------------------------------------------------------------------------------------------
// Workgroup b folds slice b - first_slice of its slot (found by bisection over the table: first_slice ascends) into R x S maxima in LDS
// and merges the cells it raised into the slot's descriptor.  LDS: R x S words (19.2 KB at 40 x 120) + the two tables.
__global__ __launch_bounds__(SC_BUILD_THREADS) void scan_context_build_kernel(const ScSlot* __restrict__ slots, const int n_slots,
                                                                              const ScTables T, const ScRecordLayout L,
                                                                              unsigned int* __restrict__ desc) {
  extern __shared__ unsigned int s_cell[];   // R x S
  __shared__ float s_edge2[SC_MAX_RINGS];
  __shared__ float s_bx[SC_MAX_SECTORS / 2], s_by[SC_MAX_SECTORS / 2];
  const int tid = threadIdx.x, R = T.R, S = T.S, half = S >> 1, cells = R * S;
  int lo = 0, hi = n_slots - 1;   // the last slot whose first_slice <= blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (slots[mid].first_slice <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const ScSlot slot = slots[lo];
  for (int c = tid; c < cells; c += SC_BUILD_THREADS) s_cell[c] = 0u;
  if (tid < R) s_edge2[tid] = T.edge2[tid];
  if (tid < half - 1) { s_bx[tid] = T.boundary[2 * tid]; s_by[tid] = T.boundary[2 * tid + 1]; }
  __syncthreads();

  const float L2 = s_edge2[R - 1], zoff = T.z_offset;
  const int first = ((int)blockIdx.x - slot.first_slice) * SC_SLICE;
  const int last = min(slot.count, first + SC_SLICE);
  for (int i = first + tid; i < last; i += SC_BUILD_THREADS) {
    const unsigned char* rec = slot.records + (size_t)i * (size_t)L.step;
    const float x = *reinterpret_cast<const float*>(rec + L.x), y = *reinterpret_cast<const float*>(rec + L.y),
                z = *reinterpret_cast<const float*>(rec + L.z);
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) continue;
    const float xx = x * x, yy = y * y;
    const float r2 = xx + yy;
    if (r2 >= L2) continue;   // (an overflowed r2 = +inf is outside too)
    int ring = 0;
    for (int k = 0; k < R - 1; k++) ring += (r2 >= s_edge2[k]) ? 1 : 0;
    const bool upper = (y > 0.0f) || (y == 0.0f && x >= 0.0f);
    const float xp = upper ? x : -x, yp = upper ? y : -y;
    int sector = upper ? 0 : half;
    for (int k = 0; k < half - 1; k++) {
      const float a = s_bx[k] * yp, b = s_by[k] * xp;
      const float cr = a - b;
      sector += (cr >= 0.0f) ? 1 : 0;
    }
    const float t = z + zoff;
    const float v = (t > 0.0f) ? t : 0.0f;   // max(+0, t): never -0, whose bits would beat every positive value
    if (v > 0.0f) atomicMax(&s_cell[ring * S + sector], __float_as_uint(v));
  }
  __syncthreads();
  unsigned int* out = desc + (size_t)slot.desc * (size_t)cells;
  for (int c = tid; c < cells; c += SC_BUILD_THREADS) {
    const unsigned int v = s_cell[c];
    if (v != 0u) atomicMax(&out[c], v);
  }
}

// ---- match ---------------------------------------------------------------------------------------------------------------------------
// One workgroup per (query, candidate) pair.  LDS (dynamic): the query R x S | the candidate with its columns doubled R x 2S (lane n
// reads column j + n: consecutive lanes, consecutive words; the query word is a broadcast) | column norms of the query S | of the
// doubled candidate 2S | the distance of every shift S.  58 KB at 40 x 120, 15 KB at 20 x 60.
__global__ __launch_bounds__(SC_MATCH_THREADS) void scan_context_match_kernel(const float* __restrict__ q_all, const float* __restrict__ c_all,
                                                                              const int nc, const int R, const int S,
                                                                              float* __restrict__ dist, int* __restrict__ shift) {
  extern __shared__ float s_mem[];
  const int tid = threadIdx.x, cells = R * S, S2 = 2 * S;
  float* s_q = s_mem;
  float* s_c = s_q + cells;
  float* s_nq = s_c + 2 * cells;
  float* s_nc = s_nq + S;
  float* s_d = s_nc + S2;
  const int pair = (int)blockIdx.x, iq = pair / nc, ic = pair - iq * nc;
  const float* __restrict__ q = q_all + (size_t)iq * (size_t)cells;
  const float* __restrict__ c = c_all + (size_t)ic * (size_t)cells;
  for (int e = tid; e < cells; e += SC_MATCH_THREADS) {
    const int r = e / S, j = e - r * S;
    const float v = c[e];
    s_q[e] = q[e];
    s_c[r * S2 + j] = v;
    s_c[r * S2 + j + S] = v;
  }
  __syncthreads();
  for (int j = tid; j < S; j += SC_MATCH_THREADS) {   // column norms: rings ascending, product then sum
    float sq = 0.0f, sc = 0.0f;
    for (int r = 0; r < R; r++) {
      const float a = s_q[r * S + j], b = s_c[r * S2 + j];
      const float aa = a * a, bb = b * b;
      sq = sq + aa;
      sc = sc + bb;
    }
    const float nq = sqrtf(sq), ncn = sqrtf(sc);
    s_nq[j] = nq;
    s_nc[j] = ncn;
    s_nc[j + S] = ncn;
  }
  __syncthreads();
  if (tid < S) {   // lane n: the distance at shift n
    const int n = tid;
    float sum = 0.0f;
    int count = 0;
    for (int j = 0; j < S; j++) {
      const float nq = s_nq[j], ncn = s_nc[j + n];
      float dot = 0.0f;
      for (int r = 0; r < R; r++) {
        const float p = s_q[r * S + j] * s_c[r * S2 + j + n];
        dot = dot + p;
      }
      if (nq > 0.0f && ncn > 0.0f) {
        const float den = nq * ncn;
        const float quo = dot / den;
        const float term = 1.0f - quo;
        sum = sum + term;
        count++;
      }
    }
    s_d[n] = count > 0 ? sum / (float)count : 1.0f;
  }
  __syncthreads();
  if (tid == 0) {   // the minimum, ties to the lowest shift
    float best = s_d[0];
    int arg = 0;
    for (int n = 1; n < S; n++)
      if (s_d[n] < best) { best = s_d[n]; arg = n; }
    dist[pair] = best;
    shift[pair] = arg;
  }
}

int check_params(const lsr_scan_context_params* p) {
  if (!p) { set_last_error("params: null Scan Context parameters"); return LSR_ERR_INVALID_ARGUMENT; }
  if (p->num_rings < 1 || p->num_rings > SC_MAX_RINGS) { set_last_error("params: num_rings outside 1 .. 40"); return LSR_ERR_INVALID_ARGUMENT; }
  if (p->num_sectors < 2 || p->num_sectors > SC_MAX_SECTORS || (p->num_sectors & 1)) {
    set_last_error("params: num_sectors must be even and in 2 .. 120");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (!(p->max_radius > 0) || !std::isfinite(p->max_radius)) { set_last_error("params: max_radius must be > 0 and finite"); return LSR_ERR_INVALID_ARGUMENT; }
  if (!std::isfinite(p->z_offset)) { set_last_error("params: z_offset must be finite"); return LSR_ERR_INVALID_ARGUMENT; }
  return LSR_OK;
}

}  // namespace

int scan_context_tables(const lsr_scan_context_params* p, ScTables* T) {
  if (int st = check_params(p)) return st;
  const int R = p->num_rings, S = p->num_sectors;
  const double Lr = p->max_radius;
  std::memset(T, 0, sizeof(*T));
  T->R = R; T->S = S;
  T->z_offset = (float)p->z_offset;
  for (int k = 1; k < R; k++) {
    const double e = (double)k * Lr / (double)R;
    T->edge2[k - 1] = (float)(e * e);
  }
  T->edge2[R - 1] = (float)(Lr * Lr);
  for (int k = 1; k < S / 2; k++) {
    const double a = 2.0 * 3.141592653589793 * (double)k / (double)S;
    T->boundary[2 * (k - 1)] = (float)std::cos(a);
    T->boundary[2 * (k - 1) + 1] = (float)std::sin(a);
  }
  return LSR_OK;
}

int scan_context_build(const ScSlot* d_slots, int n_slots, int n_slices, const ScTables& T, const ScRecordLayout& L, float* d_desc,
                       hipStream_t stream) {
  if (n_slots <= 0 || n_slices <= 0) return LSR_OK;
  const size_t dyn = sizeof(unsigned int) * (size_t)T.R * (size_t)T.S;
  hipLaunchKernelGGL(scan_context_build_kernel, dim3((unsigned int)n_slices), dim3(SC_BUILD_THREADS), dyn, stream, d_slots, n_slots, T, L,
                     reinterpret_cast<unsigned int*>(d_desc));
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int scan_context_match(const float* d_q, int nq, const float* d_c, int nc, int R, int S, float* d_dist, int* d_shift, hipStream_t stream) {
  if (nq <= 0 || nc <= 0) return LSR_OK;
  const size_t dyn = sizeof(float) * ((size_t)3 * R * S + (size_t)4 * S);
  hipLaunchKernelGGL(scan_context_match_kernel, dim3((unsigned int)((size_t)nq * (size_t)nc)), dim3(SC_MATCH_THREADS), dyn, stream, d_q,
                     d_c, nc, R, S, d_dist, d_shift);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

}  // namespace lsr

extern "C" {

int lsr_scan_context_tables(const lsr_scan_context_params* params, float* edge2, float* boundaries) {
  if (!edge2 || !boundaries) { set_last_error("edge2 / boundaries: null table"); return LSR_ERR_INVALID_ARGUMENT; }
  ScTables T;
  if (int st = scan_context_tables(params, &T)) return st;
  std::memcpy(edge2, T.edge2, sizeof(float) * (size_t)T.R);
  std::memcpy(boundaries, T.boundary, sizeof(float) * (size_t)(T.S - 2));
  return LSR_OK;
}

// One launch per piece, in the shape of lsr_assemble_map: with the clouds on the device the whole table is one piece; host clouds are
// staged SC_STAGE_BYTES at a time (a long submap is cut: a table slot is a run of records with a descriptor index, and the pieces of
// one submap meet in its descriptor through the same maxima).
int lsr_scan_context_build(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* layout, int on_device,
                           const lsr_scan_context_params* params, float* out_desc, int out_on_device) {
  constexpr size_t SC_STAGE_BYTES = (size_t)64 << 20;
  LSR_CHECK_HANDLE(h);
  if (!submaps || num_submaps <= 0 || !out_desc) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = arg_error(check_layout_xyz(layout));
  if (st) return st;
  ScTables T;
  if ((st = scan_context_tables(params, &T))) return st;
  if ((uintptr_t)out_desc & 3) { set_last_error("out_desc: must be 4-byte aligned"); return LSR_ERR_INVALID_ARGUMENT; }
  const size_t step = layout->point_step, cells = (size_t)T.R * (size_t)T.S;
  const bool in_host = on_device == 0, out_host = out_on_device == 0;
  size_t total = 0;
  for (int i = 0; i < num_submaps; i++) {
    const lsr_submap& s = submaps[i];
    if (s.n_points == 0) continue;
    if ((st = arg_error(check_records(s.cloud, s.n_points, MAP_RECORD_LIMIT, true, "submaps[].cloud")))) return st;
    if ((st = arg_error(check_record_count(total += s.n_points, MAP_RECORD_LIMIT, "submaps[] (all clouds)")))) return st;
  }
  ScanContextState& W = h->scan_context;
  W.build_ms = 0.0;
  const size_t n_floats = (size_t)num_submaps * cells;
  if (out_host && (st = W.desc.reserve(n_floats))) return st;
  float* d_desc = out_host ? W.desc.p : out_desc;
  const size_t piece_cap = in_host ? std::max<size_t>(1, SC_STAGE_BYTES / step) : std::max<size_t>(total, 1);
  if (in_host && total && (st = h->staging.reserve(std::min(total, piece_cap) * step))) return st;
  StreamDrain drain{h->stream};   // whatever was enqueued has finished before the call returns
  LSR_HIP(hipMemsetAsync(d_desc, 0, sizeof(float) * n_floats, h->stream));   // an empty submap's descriptor is all zeros
  const ScRecordLayout RL{(int)layout->point_step, (int)layout->offset_x, (int)layout->offset_y, (int)layout->offset_z};
  std::vector<ScSlot> slots;
  size_t done = 0, at = 0;
  int i = 0;
  while (done < total) {
    slots.clear();
    size_t piece = 0;
    int n_slices = 0;
    while (i < num_submaps && piece < piece_cap) {
      const size_t left = submaps[i].n_points - at;
      if (left == 0) { i++; at = 0; continue; }
      const size_t take = std::min(left, piece_cap - piece);
      const unsigned char* src = static_cast<const unsigned char*>(submaps[i].cloud) + at * step;
      const void* d_src = nullptr;
      if ((st = stage_in_at(h, src, take * step, !in_host, h->stream, piece * step, &d_src))) return st;
      ScSlot S;
      S.records = static_cast<const unsigned char*>(d_src);
      S.count = (int)take;
      S.first_slice = n_slices;
      S.desc = i;
      S.pad = 0;
      slots.push_back(S);
      n_slices += (int)((take + SC_SLICE - 1) / SC_SLICE);
      piece += take;
      at += take;
    }
    if ((st = W.h_slots.reserve(slots.size())) || (st = W.d_slots.reserve(slots.size()))) return st;
    std::memcpy(W.h_slots.p, slots.data(), sizeof(ScSlot) * slots.size());
    LSR_HIP(hipMemcpyAsync(W.d_slots.p, W.h_slots.p, sizeof(ScSlot) * slots.size(), hipMemcpyHostToDevice, h->stream));
    if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));   // LSR_PROFILE: the launch alone
    if ((st = scan_context_build(W.d_slots.p, (int)slots.size(), n_slices, T, RL, d_desc, h->stream))) return st;
    if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));   // the pinned table and the staging buffer are reused by the next piece
    if (h->profile && (st = add_ms(h->ev0, h->ev1, &W.build_ms))) return st;
    done += piece;
  }
  if (out_host) {
    LSR_HIP(hipMemcpyAsync(out_desc, d_desc, sizeof(float) * n_floats, hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));
  }
  return LSR_OK;
}

int lsr_scan_context_match(lsr_handle h, const float* q, int nq, const float* c, int nc, int on_device, const lsr_scan_context_params* params,
                           float* dist, int32_t* shift) {
  LSR_CHECK_HANDLE(h);
  if (!q || !c || !dist || !shift || nq <= 0 || nc <= 0) { set_last_error("q / c / dist / shift null, or a count below 1"); return LSR_ERR_INVALID_ARGUMENT; }
  ScTables T;
  int st = scan_context_tables(params, &T);
  if (st) return st;
  if ((size_t)nq * (size_t)nc > (size_t)INT32_MAX) { set_last_error("nq x nc: more than INT32_MAX pairs"); return LSR_ERR_INDEX_OVERFLOW; }
  if (((uintptr_t)q | (uintptr_t)c) & 3) { set_last_error("q / c: must be 4-byte aligned"); return LSR_ERR_INVALID_ARGUMENT; }
  const size_t cells = (size_t)T.R * (size_t)T.S, pairs = (size_t)nq * (size_t)nc;
  ScanContextState& W = h->scan_context;
  W.match_ms = 0.0;
  if ((st = W.dist.reserve(pairs)) || (st = W.shift.reserve(pairs))) return st;
  const float *d_q = q, *d_c = c;
  StreamDrain drain{h->stream};
  if (!on_device) {
    if ((st = W.desc.reserve(cells * (size_t)nq)) || (st = W.cand.reserve(cells * (size_t)nc))) return st;
    LSR_HIP(hipMemcpyAsync(W.desc.p, q, sizeof(float) * cells * (size_t)nq, hipMemcpyHostToDevice, h->stream));
    LSR_HIP(hipMemcpyAsync(W.cand.p, c, sizeof(float) * cells * (size_t)nc, hipMemcpyHostToDevice, h->stream));
    d_q = W.desc.p;
    d_c = W.cand.p;
  }
  if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));
  if ((st = scan_context_match(d_q, nq, d_c, nc, T.R, T.S, W.dist.p, W.shift.p, h->stream))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
  LSR_HIP(hipMemcpyAsync(dist, W.dist.p, sizeof(float) * pairs, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipMemcpyAsync(shift, W.shift.p, sizeof(int32_t) * pairs, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (h->profile && (st = add_ms(h->ev0, h->ev1, &W.match_ms))) return st;
  return LSR_OK;
}

}  // extern "C"

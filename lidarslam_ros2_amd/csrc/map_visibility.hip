// Moving objects out of the map: a depth image per keyframe, its erosion, one visibility vote per (record, neighbouring keyframe) and
// the records with too few votes against them written in input order.  The C ABI on top (lsr_visibility_pairs,
// lsr_depth_images_build, lsr_visibility_votes, lsr_assemble_map_static) is at the bottom.  include/lidarslam_reg.h and DESIGN.md §4
// state the definition; what matters here:
//   every fp32 result is ONE rounded operation on rounded inputs (this unit is compiled with -ffp-contract=off, and hipcc's divide and
//   square root are correctly rounded), so a numpy float32 restatement (tests/map_visibility_numpy.py) has the same bits;
//   a pixel is a minimum, and a minimum does not depend on the order of its points: pixels are lowered with unsigned integer minima on
//   the float bits (the values are >= +0 or +inf, where the two orders agree), straight in the image — ONE launch form: an image has
//   16 384 pixels at the defaults and a keyframe a few ten thousand records, so a copy in LDS would cost more to clear and merge per
//   workgroup than the atomics it saves;
//   the votes take one lane per record and a workgroup never straddles a submap: the pair list and the 12 floats of a pair are
//   uniform loads, the pixel of the neighbour's image the one gather per pair;
//   the compaction is flags -> scan -> write with the primitives of the map window (voxel_device.hpp: flags_in_block,
//   run_rank_in_block; map_window.hpp: mw_scan_counts).  No workgroup waits for another.
#include "map_visibility.hpp"

#include <algorithm>
#include <cmath>

#include "api_internal.hpp"
#include "sort.hpp"
#include "voxel_device.hpp"

using namespace lsr;

namespace lsr {
namespace {

constexpr unsigned int VIS_EMPTY = 0x7f800000u;   // +inf: a pixel no record has lowered

// Step 1: the pixel (row * 4 W + col) and the range of a sensor-centred point; false: no pixel
__device__ __forceinline__ bool vis_pixel(const float x, const float y, const float z, const VisConsts& C, int& pix, float& r) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const float ax = fabsf(x), ay = fabsf(y);
  const float d = ax > ay ? ax : ay;
  if (d == 0.0f) return false;
  int face;
  float u;
  if (ax >= ay) { face = x > 0.0f ? 0 : 2; u = y / x; }
  else { face = y > 0.0f ? 1 : 3; const float nx = -x; u = nx / y; }
  const float xx = x * x, yy = y * y, zz = z * z;
  const float s = xx + yy;
  const float s2 = s + zz;
  r = sqrtf(s2);
  if (r < C.min_range || r >= C.max_range) return false;
  const float v = z / d;
  const float a = v + C.Tf;
  const float b = a * C.rs;
  const float rowf = floorf(b);
  if (!(rowf >= 0.0f) || !(rowf < (float)C.H)) return false;   // (a NaN fails both)
  const float c = u + 1.0f;
  const float e = c * C.hw;
  const int ci = min(C.W - 1, (int)floorf(e));
  pix = (int)rowf * 4 * C.W + face * C.W + ci;
  return true;
}

__device__ __forceinline__ int vis_slot_of_slice(const VisSlot* __restrict__ slots, int n_slots, int sl) {
  int lo = 0, hi = n_slots - 1;   // the last slot whose first slice is <= sl (every slot owns at least one slice)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (slots[mid].first_slice <= sl) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- step 2: the images ------------------------------------------------------------------------------------------------------------------
// Workgroup b lowers the pixels of slice b - first_slice of its slot in the slot's image (filled with +inf by the caller).
__global__ __launch_bounds__(VIS_THREADS) void vis_build_kernel(const VisSlot* __restrict__ slots, const int n_slots, const VisConsts C,
                                                                const VisRecordLayout L, unsigned int* __restrict__ images) {
  const VisSlot slot = slots[vis_slot_of_slice(slots, n_slots, (int)blockIdx.x)];
  unsigned int* __restrict__ img = images + (size_t)slot.submap * (size_t)(4 * C.W * C.H);
  const int first = ((int)blockIdx.x - slot.first_slice) * VIS_BUILD_SLICE;
  const int last = min(slot.count, first + VIS_BUILD_SLICE);
  for (int i = first + (int)threadIdx.x; i < last; i += VIS_THREADS) {
    const unsigned char* rec = slot.records + (size_t)i * (size_t)L.step;
    const float x = record_field(rec, L.x) - C.ox, y = record_field(rec, L.y) - C.oy, z = record_field(rec, L.z) - C.oz;
    int pix;
    float r;
    if (vis_pixel(x, y, z, C, pix, r)) atomicMin(&img[pix], __float_as_uint(r));
  }
}

// ---- step 3: the erosion, one launch over all images ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIS_THREADS) void vis_erode_kernel(const unsigned int* __restrict__ D, unsigned int* __restrict__ E, const int H,
                                                                const int W4, const size_t total) {
  const size_t idx = (size_t)blockIdx.x * VIS_THREADS + threadIdx.x;
  if (idx >= total) return;
  const size_t cells = (size_t)H * (size_t)W4;
  const size_t image = idx / cells;
  const int rem = (int)(idx - image * cells);
  const int row = rem / W4, col = rem - row * W4;
  const unsigned int* __restrict__ img = D + image * cells;
  const int r0 = max(row - 1, 0), r1 = min(row + 1, H - 1);
  const int cl = col == 0 ? W4 - 1 : col - 1, cr = col == W4 - 1 ? 0 : col + 1;
  unsigned int m = VIS_EMPTY;
  for (int rr = r0; rr <= r1; rr++) {
    const unsigned int* __restrict__ line = img + (size_t)rr * W4;
    m = min(m, min(line[cl], min(line[col], line[cr])));
  }
  E[idx] = m;
}

// ---- step 5: the votes ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIS_THREADS) void vis_votes_kernel(const VisSlot* __restrict__ slots, const int n_slots, const VisConsts C,
                                                                const VisRecordLayout L, const int* __restrict__ first_pair,
                                                                const int* __restrict__ other, const float* __restrict__ rel12,
                                                                const float* __restrict__ E, int* __restrict__ votes) {
  const VisSlot slot = slots[vis_slot_of_slice(slots, n_slots, (int)blockIdx.x)];
  const int i = ((int)blockIdx.x - slot.first_slice) * VIS_CHUNK + (int)threadIdx.x;
  if (i >= slot.count) return;
  const unsigned char* rec = slot.records + (size_t)i * (size_t)L.step;
  const float x = record_field(rec, L.x), y = record_field(rec, L.y), z = record_field(rec, L.z);
  const size_t cells = (size_t)(4 * C.W * C.H);
  const int p0 = first_pair[slot.submap], p1 = first_pair[slot.submap + 1];
  int v = 0;
  for (int p = p0; p < p1; p++) {
    const float* __restrict__ m = rel12 + 12 * (size_t)p;
    const float* __restrict__ img = E + (size_t)other[p] * cells;
    float q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {   // ((m0 x + m1 y) + m2 z) + m3: lsr_assemble_map's expression
      const float a = m[4 * k] * x, b = m[4 * k + 1] * y, c = m[4 * k + 2] * z;
      const float ab = a + b;
      const float abc = ab + c;
      q[k] = abc + m[4 * k + 3];
    }
    const float sx = q[0] - C.ox, sy = q[1] - C.oy, sz = q[2] - C.oz;
    int pix;
    float r;
    if (!vis_pixel(sx, sy, sz, C, pix, r)) continue;
    const float e = img[pix];
    const float rm = r + C.margin;
    if (e < INFINITY && rm < e) v++;
  }
  votes[(size_t)slot.first_out + (size_t)i] = v;
}

// ---- step 6: flags -> scan -> write ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIS_CHUNK) void vis_count_kernel(const int* __restrict__ votes, const size_t n, const int min_votes,
                                                              int* __restrict__ counts) {
  const size_t i = (size_t)blockIdx.x * VIS_CHUNK + threadIdx.x;
  const int c = flags_in_block(i < n && votes[i] < min_votes);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// kept[t] = the kept records in front of raw record first[t] (a submap's first record, or the total): the prefix of its chunk and the
// flags of the chunk in front of it
__global__ __launch_bounds__(VIS_THREADS) void vis_bounds_kernel(const int* __restrict__ votes, const int min_votes, const int* __restrict__ base,
                                                                 const long long* __restrict__ first, const int n_bounds,
                                                                 long long* __restrict__ kept) {
  const int t = (int)(blockIdx.x * VIS_THREADS + threadIdx.x);
  if (t >= n_bounds) return;
  const long long g = first[t];
  const long long b = g / VIS_CHUNK;
  long long r = base[b];
  for (long long j = b * VIS_CHUNK; j < g; j++) r += votes[j] < min_votes ? 1 : 0;
  kept[t] = r;
}

// the kept records of the raw map (records of `words` 4-byte words) written at their rank; WIDE: 32-byte records on 16-byte boundaries
template <bool WIDE>
__global__ __launch_bounds__(VIS_CHUNK) void vis_write_kernel(const int* __restrict__ votes, const size_t n, const int min_votes,
                                                              const int* __restrict__ base, const unsigned int* __restrict__ raw,
                                                              const int words, unsigned int* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * VIS_CHUNK + threadIdx.x;
  const bool keep = i < n && votes[i] < min_votes;
  const int r = run_rank_in_block(keep, base);
  if (!keep) return;
  if (WIDE) {
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(raw) + 2 * i;
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(out) + 2 * (size_t)r;
    const uint4 a = src[0], b = src[1];
    dst[0] = a;
    dst[1] = b;
  } else {
    const unsigned int* __restrict__ src = raw + i * (size_t)words;
    unsigned int* __restrict__ dst = out + (size_t)r * (size_t)words;
    for (int w = 0; w < words; w++) dst[w] = src[w];
  }
}

bool vis_finite(double v) { return std::isfinite(v); }
int vis_refuse(const char* why) { set_last_error(std::string("params: ") + why); return LSR_ERR_INVALID_ARGUMENT; }

// rows 0 .. 2 of M (column-major 4x4): R[r][c] = M[4 c + r], t[r] = M[12 + r]
void vis_relative(const double* Mk, const double* Mi, float* rel12) {
  double inv[12];   // (R^T, -R^T t) of M_k, row-major 3x4
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) inv[4 * r + c] = Mk[4 * r + c];   // R^T[r][c] = R[c][r] = M[4 r + c]
    inv[4 * r + 3] = -((inv[4 * r] * Mk[12] + inv[4 * r + 1] * Mk[13]) + inv[4 * r + 2] * Mk[14]);
  }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) {
      double v = (inv[4 * r] * Mi[4 * c] + inv[4 * r + 1] * Mi[4 * c + 1]) + inv[4 * r + 2] * Mi[4 * c + 2];
      if (c == 3) v += inv[4 * r + 3];
      rel12[4 * r + c] = (float)v;
    }
}

// Step 4 into vectors
int vis_pairs(const lsr_submap* submaps, int n, const double* poses16, const lsr_visibility_params* p, std::vector<int>& first_pair,
              std::vector<int>& other, std::vector<float>& rel12) {
  std::vector<double> M((size_t)n * 16);
  for (int i = 0; i < n; i++) {
    if (poses16) std::memcpy(&M[16 * (size_t)i], poses16 + 16 * (size_t)i, sizeof(double) * 16);
    else submap_pose_matrix(submaps[i], &M[16 * (size_t)i]);
  }
  first_pair.assign((size_t)n + 1, 0);
  other.clear();
  rel12.clear();
  std::vector<std::pair<double, int>> near;
  for (int i = 0; i < n; i++) {
    near.clear();
    const double* ti = &M[16 * (size_t)i + 12];
    for (int k = 0; k < n; k++) {
      if (k == i) continue;
      const double* tk = &M[16 * (size_t)k + 12];
      const double dx = tk[0] - ti[0], dy = tk[1] - ti[1], dz = tk[2] - ti[2];
      const double dist = std::sqrt((dx * dx + dy * dy) + dz * dz);
      if (dist <= p->keyframe_range) near.emplace_back(dist, k);
    }
    std::sort(near.begin(), near.end());   // by distance, ties to the lower index
    if ((int)near.size() > p->max_neighbours) near.resize((size_t)p->max_neighbours);
    std::sort(near.begin(), near.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.second < b.second; });
    for (const auto& e : near) {
      other.push_back(e.second);
      rel12.resize(rel12.size() + 12);
      vis_relative(&M[16 * (size_t)e.second], &M[16 * (size_t)i], rel12.data() + rel12.size() - 12);
    }
    first_pair[(size_t)i + 1] = (int)other.size();
  }
  return LSR_OK;
}

VisRecordLayout vis_layout(const lsr_pc2_layout* L) { return VisRecordLayout{(int)L->point_step, (int)L->offset_x, (int)L->offset_y, (int)L->offset_z}; }

// what the two entries over a table of submaps check alike -> the records in all
int vis_check_submaps(const lsr_submap* submaps, int num_submaps, size_t* total_out) {
  size_t total = 0;
  for (int i = 0; i < num_submaps; i++) {
    const lsr_submap& s = submaps[i];
    if (s.n_points == 0) continue;
    int st;
    if ((st = arg_error(check_records(s.cloud, s.n_points, MAP_RECORD_LIMIT, true, "submaps[].cloud")))) return st;
    if ((st = arg_error(check_record_count(total += s.n_points, MAP_RECORD_LIMIT, "submaps[] (all clouds)")))) return st;
  }
  *total_out = total;
  return LSR_OK;
}

// The table of submaps walked in pieces (with the clouds on the device the whole table is one piece; host clouds are staged
// LSR_VISIBILITY_PIECE_BYTES at a time, a long submap cut): launch(d_slots, n_slots, n_slices) enqueues the piece's launch; *ms gets its time.
template <class Launch>
int vis_walk(lsr_handle h, const lsr_submap* submaps, int num_submaps, size_t step, bool in_host, size_t total, int slice, double* ms,
             Launch&& launch) {
  VisibilityState& W = h->visibility;
  int st;
  const size_t piece_cap = in_host ? std::max<size_t>(1, (size_t)W.piece_bytes / step) : std::max<size_t>(total, 1);
  if (in_host && total && (st = h->staging.reserve(std::min(total, piece_cap) * step))) return st;
  std::vector<VisSlot> slots;
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
      VisSlot S;
      S.records = static_cast<const unsigned char*>(d_src);
      S.first_out = (long long)(done + piece);
      S.count = (int)take;
      S.first_slice = n_slices;
      S.submap = i;
      S.pad = 0;
      slots.push_back(S);
      n_slices += (int)((take + (size_t)slice - 1) / (size_t)slice);
      piece += take;
      at += take;
    }
    if ((st = W.h_slots.reserve(slots.size())) || (st = W.d_slots.reserve(slots.size()))) return st;
    std::memcpy(W.h_slots.p, slots.data(), sizeof(VisSlot) * slots.size());
    LSR_HIP(hipMemcpyAsync(W.d_slots.p, W.h_slots.p, sizeof(VisSlot) * slots.size(), hipMemcpyHostToDevice, h->stream));
    if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));   // LSR_PROFILE: the launch alone
    launch(W.d_slots.p, (int)slots.size(), n_slices);
    LSR_HIP(hipGetLastError());
    if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));   // the pinned table and the staging buffer are reused by the next piece
    if (h->profile && (st = add_ms(h->ev0, h->ev1, ms))) return st;
    done += piece;
  }
  return LSR_OK;
}

// The votes of every record in assembly order into d_votes (device, `total` ints).  The caller has checked the arguments and drains
// the stream.
int vis_votes_run(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* layout, bool in_host, size_t total,
                  const double* poses16, const float* images, bool images_on_device, const lsr_visibility_params* params, const VisConsts& C,
                  int* d_votes) {
  VisibilityState& W = h->visibility;
  int st;
  std::vector<int> first_pair, other;
  std::vector<float> rel12;
  if ((st = vis_pairs(submaps, num_submaps, poses16, params, first_pair, other, rel12))) return st;
  if (other.empty()) {   // nobody looks at anybody: no votes
    LSR_HIP(hipMemsetAsync(d_votes, 0, sizeof(int) * total, h->stream));
    return LSR_OK;
  }
  const size_t cells = (size_t)4 * C.W * C.H, n_floats = cells * (size_t)num_submaps;
  if ((st = W.first_pair.reserve(first_pair.size())) || (st = W.other.reserve(other.size())) || (st = W.rel12.reserve(rel12.size()))) return st;
  LSR_HIP(hipMemcpyAsync(W.first_pair.p, first_pair.data(), sizeof(int) * first_pair.size(), hipMemcpyHostToDevice, h->stream));
  LSR_HIP(hipMemcpyAsync(W.other.p, other.data(), sizeof(int) * other.size(), hipMemcpyHostToDevice, h->stream));
  LSR_HIP(hipMemcpyAsync(W.rel12.p, rel12.data(), sizeof(float) * rel12.size(), hipMemcpyHostToDevice, h->stream));
  const float* d_images = images;
  if (!images_on_device) {
    if ((st = W.images.reserve(n_floats))) return st;
    LSR_HIP(hipMemcpyAsync(W.images.p, images, sizeof(float) * n_floats, hipMemcpyHostToDevice, h->stream));
    d_images = W.images.p;
  }
  const VisRecordLayout RL = vis_layout(layout);
  st = vis_walk(h, submaps, num_submaps, layout->point_step, in_host, total, VIS_CHUNK, &W.votes_ms,
                [&](const VisSlot* d_slots, int n_slots, int n_slices) {
                  hipLaunchKernelGGL(vis_votes_kernel, dim3((unsigned int)n_slices), dim3(VIS_THREADS), 0, h->stream, d_slots, n_slots, C, RL,
                                     W.first_pair.p, W.other.p, W.rel12.p, d_images, d_votes);
                });
  LSR_HIP(hipStreamSynchronize(h->stream));   // the vectors above have been read
  return st;
}

int vis_check_common(const lsr_submap* submaps, int num_submaps, bool pointers_ok) {
  if (!submaps || num_submaps <= 0 || !pointers_ok) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  return LSR_OK;
}

}  // namespace

int visibility_consts(const lsr_visibility_params* p, VisConsts* C) {
  if (!p) { set_last_error("params: null visibility parameters"); return LSR_ERR_INVALID_ARGUMENT; }
  if (p->face_width < 8 || p->face_width > LSR_VISIBILITY_MAX_FACE_WIDTH || (p->face_width & 1)) return vis_refuse("face_width must be even and in 8 .. 1024");
  if (p->height < 4 || p->height > LSR_VISIBILITY_MAX_HEIGHT) return vis_refuse("height outside 4 .. 512");
  if (!(p->max_tan_elevation > 0) || !vis_finite(p->max_tan_elevation)) return vis_refuse("max_tan_elevation must be > 0 and finite");
  if (!vis_finite(p->min_range) || !vis_finite(p->max_range) || !(p->max_range > 0) || !(p->min_range < p->max_range))
    return vis_refuse("min_range < max_range, both finite, max_range > 0");
  if (!(p->margin >= 0) || !vis_finite(p->margin)) return vis_refuse("margin must be >= 0 and finite");
  if (!(p->keyframe_range > 0)) return vis_refuse("keyframe_range must be > 0");
  if (p->max_neighbours < 1 || p->max_neighbours > LSR_VISIBILITY_MAX_NEIGHBOURS) return vis_refuse("max_neighbours outside 1 .. 64");
  if (p->min_votes < 1) return vis_refuse("min_votes must be >= 1");
  for (int k = 0; k < 3; k++)
    if (!vis_finite(p->sensor_origin[k])) return vis_refuse("sensor_origin must be finite");
  C->W = p->face_width;
  C->H = p->height;
  C->hw = (float)(p->face_width / 2);
  C->Tf = (float)p->max_tan_elevation;
  C->rs = (float)((double)p->height / (2.0 * p->max_tan_elevation));
  C->min_range = (float)p->min_range;
  C->max_range = (float)p->max_range;
  C->margin = (float)p->margin;
  C->ox = (float)p->sensor_origin[0]; C->oy = (float)p->sensor_origin[1]; C->oz = (float)p->sensor_origin[2];
  return LSR_OK;
}

}  // namespace lsr

extern "C" {

int lsr_visibility_pairs(const lsr_submap* submaps, int num_submaps, const double* poses16, const lsr_visibility_params* params,
                         int32_t* first_pair, int32_t* other, float* rel12, size_t capacity_pairs, size_t* n_pairs) {
  if (!submaps || num_submaps <= 0 || !first_pair || !other || !rel12 || !n_pairs) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  VisConsts C;
  int st = visibility_consts(params, &C);
  if (st) return st;
  std::vector<int> fp, ot;
  std::vector<float> rel;
  if ((st = vis_pairs(submaps, num_submaps, poses16, params, fp, ot, rel))) return st;
  *n_pairs = ot.size();
  if (ot.size() > capacity_pairs) { set_last_error("other / rel12: more pairs than capacity_pairs"); return LSR_ERR_INVALID_ARGUMENT; }
  std::memcpy(first_pair, fp.data(), sizeof(int32_t) * fp.size());
  if (!ot.empty()) {
    std::memcpy(other, ot.data(), sizeof(int32_t) * ot.size());
    std::memcpy(rel12, rel.data(), sizeof(float) * rel.size());
  }
  return LSR_OK;
}

int lsr_depth_images_build(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* layout, int on_device,
                           const lsr_visibility_params* params, int eroded, float* out_images, int out_on_device) {
  LSR_CHECK_HANDLE(h);
  int st = vis_check_common(submaps, num_submaps, out_images != nullptr);
  if (st || (st = arg_error(check_layout_xyz(layout)))) return st;
  VisConsts C;
  if ((st = visibility_consts(params, &C))) return st;
  if ((uintptr_t)out_images & 3) { set_last_error("out_images: must be 4-byte aligned"); return LSR_ERR_INVALID_ARGUMENT; }
  size_t total = 0;
  if ((st = vis_check_submaps(submaps, num_submaps, &total))) return st;
  const bool in_host = on_device == 0, out_host = out_on_device == 0;
  VisibilityState& W = h->visibility;
  W.images_ms = 0.0;
  const size_t cells = (size_t)4 * C.W * C.H, n_floats = cells * (size_t)num_submaps;
  if (eroded && (st = W.raw.reserve(n_floats))) return st;
  if (out_host && (st = W.images.reserve(n_floats))) return st;
  float* d_final = out_host ? W.images.p : out_images;
  float* d_D = eroded ? W.raw.p : d_final;
  StreamDrain drain{h->stream};   // whatever was enqueued has finished before the call returns
  LSR_HIP(hipMemsetD32Async((hipDeviceptr_t)d_D, (int)VIS_EMPTY, n_floats, h->stream));   // a pixel no record reaches is +inf
  const VisRecordLayout RL = vis_layout(layout);
  if ((st = vis_walk(h, submaps, num_submaps, layout->point_step, in_host, total, VIS_BUILD_SLICE, &W.images_ms,
                     [&](const VisSlot* d_slots, int n_slots, int n_slices) {
                       hipLaunchKernelGGL(vis_build_kernel, dim3((unsigned int)n_slices), dim3(VIS_THREADS), 0, h->stream, d_slots, n_slots, C,
                                          RL, reinterpret_cast<unsigned int*>(d_D));
                     })))
    return st;
  if (eroded) {
    if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(vis_erode_kernel, dim3((unsigned int)((n_floats + VIS_THREADS - 1) / VIS_THREADS)), dim3(VIS_THREADS), 0, h->stream,
                       reinterpret_cast<const unsigned int*>(d_D), reinterpret_cast<unsigned int*>(d_final), C.H, 4 * C.W, n_floats);
    LSR_HIP(hipGetLastError());
    if (h->profile) {
      LSR_HIP(hipEventRecord(h->ev1, h->stream));
      LSR_HIP(hipStreamSynchronize(h->stream));
      if ((st = add_ms(h->ev0, h->ev1, &W.images_ms))) return st;
    }
  }
  if (out_host) {
    LSR_HIP(hipMemcpyAsync(out_images, d_final, sizeof(float) * n_floats, hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));
  }
  return LSR_OK;
}

int lsr_visibility_votes(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* layout, int on_device,
                         const double* poses16, const float* images, int images_on_device, const lsr_visibility_params* params,
                         int32_t* votes, int votes_on_device, size_t* first_record, size_t* n_records) {
  LSR_CHECK_HANDLE(h);
  int st = vis_check_common(submaps, num_submaps, images && votes);
  if (st) return st;
  if (!n_records) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if ((st = arg_error(check_layout_xyz(layout)))) return st;
  VisConsts C;
  if ((st = visibility_consts(params, &C))) return st;
  if (((uintptr_t)images | (uintptr_t)votes) & 3) { set_last_error("images / votes: must be 4-byte aligned"); return LSR_ERR_INVALID_ARGUMENT; }
  size_t total = 0;
  if ((st = vis_check_submaps(submaps, num_submaps, &total))) return st;
  VisibilityState& W = h->visibility;
  W.votes_ms = 0.0;
  if (total > 0) {
    const bool votes_host = votes_on_device == 0;
    if (votes_host && (st = W.votes.reserve(total))) return st;
    int* d_votes = votes_host ? W.votes.p : votes;
    StreamDrain drain{h->stream};
    if ((st = vis_votes_run(h, submaps, num_submaps, layout, on_device == 0, total, poses16, images, images_on_device != 0, params, C, d_votes)))
      return st;
    if (votes_host) {
      LSR_HIP(hipMemcpyAsync(votes, d_votes, sizeof(int32_t) * total, hipMemcpyDeviceToHost, h->stream));
      LSR_HIP(hipStreamSynchronize(h->stream));
    }
  }
  if (first_record) {
    size_t off = 0;
    for (int i = 0; i < num_submaps; i++) { first_record[i] = off; off += submaps[i].n_points; }
    first_record[num_submaps] = off;
  }
  *n_records = total;
  return LSR_OK;
}

int lsr_assemble_map_static(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout, int on_device,
                            const double* poses16, const float* images, int images_on_device, const lsr_visibility_params* params,
                            void* out_data, size_t capacity_points, const lsr_pc2_layout* out_layout, int out_on_device,
                            size_t* first_record, size_t* n_out, size_t* n_removed) {
  LSR_CHECK_HANDLE(h);
  int st = vis_check_common(submaps, num_submaps, images && n_out);
  if (st) return st;
  if (!n_removed) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if ((st = check_layout(in_layout, "in_layout")) || (st = check_out_layout(out_layout))) return st;
  VisConsts C;
  if ((st = visibility_consts(params, &C))) return st;
  if ((uintptr_t)images & 3) { set_last_error("images: must be 4-byte aligned"); return LSR_ERR_INVALID_ARGUMENT; }
  size_t total = 0;
  if ((st = vis_check_submaps(submaps, num_submaps, &total))) return st;
  if ((st = arg_error(check_records(out_data, 0, MAP_RECORD_LIMIT, true, "out_data")))) return st;
  const size_t in_step = in_layout->point_step, out_step = out_layout->point_step;
  const bool in_host = on_device == 0, out_host = out_on_device == 0;
  if (out_data && in_host == out_host)   // (the output never holds more records than the raw map)
    for (int i = 0; i < num_submaps; i++)
      if (ranges_overlap(out_data, std::min(capacity_points, total) * out_step, submaps[i].cloud, submaps[i].n_points * in_step)) {
        set_last_error("the output range overlaps an input cloud");
        return LSR_ERR_INVALID_ARGUMENT;
      }
  VisibilityState& W = h->visibility;
  W.votes_ms = 0.0;
  std::vector<long long> bounds((size_t)num_submaps + 1, 0);
  for (int i = 0; i < num_submaps; i++) bounds[(size_t)i + 1] = bounds[(size_t)i] + (long long)submaps[i].n_points;
  auto finish = [&](const long long* kept_first, size_t kept) {
    if (first_record)
      for (int i = 0; i <= num_submaps; i++) first_record[i] = (size_t)kept_first[i];
    *n_out = kept;
    *n_removed = total - kept;
    return LSR_OK;
  };
  if (total == 0) return finish(bounds.data(), 0);

  const int nb = (int)((total + VIS_CHUNK - 1) / VIS_CHUNK), min_votes = params->min_votes;
  const size_t nbounds = bounds.size();
  if ((st = W.votes.reserve(total)) || (st = W.counts.reserve(2 * (size_t)nb + 1)) || (st = W.bounds.reserve(2 * nbounds)) ||
      (st = h->pcd.map.reserve(total * out_step)))
    return st;
  StreamDrain drain{h->stream};
  if ((st = vis_votes_run(h, submaps, num_submaps, in_layout, in_host, total, poses16, images, images_on_device != 0, params, C, W.votes.p)))
    return st;
  // the raw map, records of out_layout kept on the object (the buffer of lsr_save_map_pcd): the bytes every kept record has
  size_t n_raw = 0;
  if ((st = lsr_assemble_map(h, submaps, num_submaps, in_layout, on_device, poses16, h->pcd.map.p, total, out_layout, 1, nullptr, &n_raw))) return st;
  if (n_raw != total) { set_last_error("static map: the raw map has another size than the votes"); return LSR_ERR_HIP; }
  int* counts = W.counts.p;
  int* base = counts + nb;
  unsigned int token = 0;
  LSR_HIP(hipMemcpyAsync(W.bounds.p, bounds.data(), sizeof(long long) * nbounds, hipMemcpyHostToDevice, h->stream));
  if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));
  hipLaunchKernelGGL(vis_count_kernel, dim3((unsigned int)nb), dim3(VIS_CHUNK), 0, h->stream, W.votes.p, total, min_votes, counts);
  LSR_HIP(hipGetLastError());
  if ((st = mw_scan_counts(h->scratch, h->stream, counts, nb, base, &token))) return st;
  if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
  hipLaunchKernelGGL(vis_bounds_kernel, dim3((unsigned int)((nbounds + VIS_THREADS - 1) / VIS_THREADS)), dim3(VIS_THREADS), 0, h->stream,
                     W.votes.p, min_votes, base, W.bounds.p, (int)nbounds, W.bounds.p + nbounds);
  LSR_HIP(hipGetLastError());
  int kept_i = 0;
  if ((st = sorted_runs_count(h->scratch, h->stream, token, &kept_i))) return st;   // the ONE host wait in front of the write: it sizes the output
  if (kept_i < 0 || (size_t)kept_i > total) { set_last_error("static map: the count is outside its bounds"); return LSR_ERR_HIP; }
  const size_t kept = (size_t)kept_i;
  std::vector<long long> kept_first(nbounds, 0);
  LSR_HIP(hipMemcpyAsync(kept_first.data(), W.bounds.p + nbounds, sizeof(long long) * nbounds, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (h->profile && (st = add_ms(h->ev0, h->ev1, &W.votes_ms))) return st;
  if (!out_data || kept == 0) return finish(kept_first.data(), kept);
  if (capacity_points < kept) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
  void* d_out = out_data;
  if (out_host) {
    if ((st = h->map_out.reserve(kept * out_step))) return st;
    d_out = h->map_out.p;
  }
  const bool wide = out_step == 32 && (((uintptr_t)d_out | (uintptr_t)h->pcd.map.p) & 15) == 0;
  if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));
  if (wide)
    hipLaunchKernelGGL(vis_write_kernel<true>, dim3((unsigned int)nb), dim3(VIS_CHUNK), 0, h->stream, W.votes.p, total, min_votes, base,
                       reinterpret_cast<const unsigned int*>(h->pcd.map.p), (int)(out_step / 4), static_cast<unsigned int*>(d_out));
  else
    hipLaunchKernelGGL(vis_write_kernel<false>, dim3((unsigned int)nb), dim3(VIS_CHUNK), 0, h->stream, W.votes.p, total, min_votes, base,
                       reinterpret_cast<const unsigned int*>(h->pcd.map.p), (int)(out_step / 4), static_cast<unsigned int*>(d_out));
  LSR_HIP(hipGetLastError());
  if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
  if (out_host) LSR_HIP(hipMemcpyAsync(out_data, d_out, kept * out_step, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (h->profile && (st = add_ms(h->ev0, h->ev1, &W.votes_ms))) return st;
  return finish(kept_first.data(), kept);
}

}  // extern "C"

// The voxel arithmetic that defines the bits of pcl::VoxelGrid / VoxelGridCovariance here, written ONCE: the bounding box of the
// finite points and its workgroup fold, the leaf cell and linear index of a point, the grid dimensions of a box, and the walk over
// runs of equal sorted keys (rank of a run, heads per chunk, float centroid of a run).  Device helpers only, no kernels: every
// translation unit that includes it compiles its own copy (internal linkage).
//
// CONTRACTION RULE.  The units that include this header are built with different -ffp-contract settings (on: ndt.o, grid_build.o,
// cloud_codec.o; off: map_filter.o, nn.o; the compiler's default elsewhere) and promise the same bits from all of them.  So no
// expression in here may hold a product whose result feeds an addition or subtraction directly: a floor sits between the multiply
// and the subtract of leaf_cell, (hi - lo) * inv_leaf is a subtract THEN a multiply, the centroid is additions and one division.
// Keep it that way when changing anything below.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace lsr {
namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// ---- bounding box of the finite points ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool point_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// one thread's share: a point with a non-finite coordinate is not counted and moves no bound
struct BoxAcc {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  unsigned int cnt = 0;
  __device__ __forceinline__ void add(float x, float y, float z) {
    if (!point_finite(x, y, z)) return;
    cnt++;
    mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
    mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
    mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
  }
};

// The box of a workgroup, one row per wave in LDS: any thread may read it once box_fold_block has returned.
struct BoxFolded {
  const float (*mn)[3];
  const float (*mx)[3];
  const unsigned int* cnt;
  __device__ __forceinline__ float lo(int k) const { return fminf(fminf(mn[0][k], mn[1][k]), fminf(mn[2][k], mn[3][k])); }
  __device__ __forceinline__ float hi(int k) const { return fmaxf(fmaxf(mx[0][k], mx[1][k]), fmaxf(mx[2][k], mx[3][k])); }
  __device__ __forceinline__ unsigned int count() const { return cnt[0] + cnt[1] + cnt[2] + cnt[3]; }
  // the record of a workgroup, word k: {min xyz, max xyz (float bits), finite points, 0}
  __device__ __forceinline__ unsigned int word(int k) const {
    if (k < 3) return __float_as_uint(lo(k));
    if (k < 6) return __float_as_uint(hi(k - 3));
    return k == 6 ? count() : 0u;
  }
};

// Folds the threads' boxes of a workgroup of 256 threads (4 waves): a butterfly inside every wave, one row per wave in LDS (112
// bytes, owned here), ONE barrier.  Called by ALL threads of the workgroup.
__device__ __forceinline__ BoxFolded box_fold_block(BoxAcc b) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) { b.mn[k] = fminf(b.mn[k], __shfl_xor(b.mn[k], m, 64)); b.mx[k] = fmaxf(b.mx[k], __shfl_xor(b.mx[k], m, 64)); }
    b.cnt += __shfl_xor(b.cnt, m, 64);
  }
  __shared__ float s_mn[4][3], s_mx[4][3];
  __shared__ unsigned int s_cnt[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    for (int k = 0; k < 3; k++) { s_mn[w][k] = b.mn[k]; s_mx[w][k] = b.mx[k]; }
    s_cnt[w] = b.cnt;
  }
  __syncthreads();
  return BoxFolded{s_mn, s_mx, s_cnt};
}

// Threads 0..6 publish the workgroup's record.  words != null: eight plain words (the eighth zero), nothing else.  Otherwise seven
// self-validating granules token << 32 | bits (common.hpp: BboxPart) into the host mailbox record `mail`, each ONE relaxed
// system-scope store, and (dev != null) the same granules into device memory.
__device__ __forceinline__ void box_publish(const BoxFolded& F, BboxPart* __restrict__ mail, unsigned int token,
                                            unsigned long long* __restrict__ dev, unsigned int* __restrict__ words) {
  const int k = threadIdx.x;
  if (words) {
    if (k < 8) words[k] = F.word(k);
    return;
  }
  if (k < BBOX_GRANULES) {
    const unsigned long long g = ((unsigned long long)token << 32) | F.word(k);
    if (dev) dev[k] = g;
    __hip_atomic_store(&mail->g[k], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- leaf cell and linear leaf index -----------------------------------------------------------------------------------------
// ijk = (int)(floor(p * inv_leaf) - (float)min_b), exactly as VoxelGrid / VoxelGridCovariance compute it: a FLOAT
// subtraction behind the floor.  (The neighbour hash of nn.hip / nn_device.hpp computes (int)floorf(p * inv_cell) - o with an INTEGER
// subtraction: another expression with another rounding, deliberately not this helper.)
struct LeafCell { int i0, i1, i2; };
__device__ __forceinline__ int leaf_axis(float pk, float inv_leaf, int min_b) { return (int)(floorf(pk * inv_leaf) - (float)min_b); }
__device__ __forceinline__ LeafCell leaf_cell(float px, float py, float pz, float inv_leaf, int mb0, int mb1, int mb2) {
  return LeafCell{leaf_axis(px, inv_leaf, mb0), leaf_axis(py, inv_leaf, mb1), leaf_axis(pz, inv_leaf, mb2)};
}
// The map window (include/lidarslam_reg.h: lsr_map_window): a point is inside iff it is finite and its ABSOLUTE cell
// floorf(p * inv_leaf) — the float leaf_axis forms before it subtracts min_b — lies in [lo, hi] on every axis.  The bounds are the
// window's int cells as floats (exact below 2^24); the comparison stays in float: no conversion, and no min_b to subtract.
struct WindowCells { float lo[3], hi[3]; };
__device__ __forceinline__ bool window_axis(float pk, float inv_leaf, float lo, float hi) {
  const float f = floorf(pk * inv_leaf);
  return lo <= f && f <= hi;
}
__device__ __forceinline__ bool in_window(float px, float py, float pz, float inv_leaf, const WindowCells& W) {
  return point_finite(px, py, pz) && window_axis(px, inv_leaf, W.lo[0], W.hi[0]) && window_axis(py, inv_leaf, W.lo[1], W.hi[1]) &&
         window_axis(pz, inv_leaf, W.lo[2], W.hi[2]);
}
// i0 + i1 * div_b[0] + i2 * div_b[0] * div_b[1], the products in T (int: the int32 filters and builders; long long: the map filter)
template <class T>
__device__ __forceinline__ T leaf_index(const LeafCell& c, T mul1, T mul2) { return (T)c.i0 + (T)c.i1 * mul1 + (T)c.i2 * mul2; }
// the sort key of a point: its leaf index, or `sentinel` (one past the last cell: sorts last) for a non-finite point
template <class T>
__device__ __forceinline__ std::make_unsigned_t<T> leaf_key(float px, float py, float pz, float inv_leaf, int mb0, int mb1, int mb2, T mul1,
                                                            T mul2, std::make_unsigned_t<T> sentinel) {
  if (!point_finite(px, py, pz)) return sentinel;
  return (std::make_unsigned_t<T>)leaf_index<T>(leaf_cell(px, py, pz, inv_leaf, mb0, mb1, mb2), mul1, mul2);
}

// ---- grid dimensions of a box ------------------------------------------------------------------------------------------------
// min_b / div_b as PCL forms them, the cell coordinates of the two corners as floats (for a caller whose limits are stated on
// them) and PCL's overflow volume, the product over the axes of (int64)((max - min) * inv_leaf) + 1.  The limits and their error
// texts are the callers'.
struct GridDims { int min_b[3], div_b[3]; float cell_lo[3], cell_hi[3]; long long volume; };
__host__ __device__ inline GridDims grid_dims(const float* mn, const float* mx, float inv_leaf) {
  GridDims G;
  G.volume = 1;
  for (int k = 0; k < 3; k++) {
    G.volume *= (long long)((mx[k] - mn[k]) * inv_leaf) + 1;
    G.cell_lo[k] = floorf(mn[k] * inv_leaf);
    G.cell_hi[k] = floorf(mx[k] * inv_leaf);
    G.min_b[k] = (int)G.cell_lo[k];
    G.div_b[k] = (int)G.cell_hi[k] - G.min_b[k] + 1;
  }
  return G;
}

__host__ __device__ inline int bits_for(unsigned long long max_key) {  // bits needed to write max_key (at least 1): the radix bits of keys in [0, max_key]
  int b = 1;
  while (b < 64 && (max_key >> b) != 0ull) b++;
  return b;
}

// ---- runs of equal keys in a sorted sequence: one position per thread, 256 per workgroup ---------------------------------------
// A key view says whether two sorted positions hold the same key; Index is the type the caller indexes with (int: the int32
// paths; size_t: the map filter).
struct KeysU32 {
  const unsigned int* __restrict__ k;
  typedef unsigned int Value;
  template <class I> __device__ __forceinline__ Value at(I i) const { return k[i]; }
  template <class I> __device__ __forceinline__ bool is(I i, Value v) const { return k[i] == v; }
};
struct KeysHiLo {   // (high, low) words; hi == null: the low word is the whole key
  const unsigned int* __restrict__ lo;
  const unsigned int* __restrict__ hi;
  typedef unsigned long long Value;
  template <class I> __device__ __forceinline__ Value at(I i) const { return ((unsigned long long)(hi ? hi[i] : 0u) << 32) | lo[i]; }
  template <class I> __device__ __forceinline__ bool is(I i, Value v) const { return lo[i] == (unsigned int)v && (!hi || hi[i] == (unsigned int)(v >> 32)); }
};
template <class Keys, class I>
__device__ __forceinline__ bool run_is_head(const Keys& K, I i) { return i == 0 || !K.is(i, K.at(i - 1)); }

// The threads of a workgroup of 256 whose flag is set, counted.  Called by all threads: one barrier inside.
__device__ __forceinline__ int flags_in_block(bool flag) {
  __shared__ int s_w[4];
  int c = flag ? 1 : 0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// The heads among this workgroup's 256 positions.
template <class Keys, class I>
__device__ __forceinline__ int run_heads_in_block(const Keys& K, I i, I n) { return flags_in_block(i < n && run_is_head(K, i)); }

// The number of heads in front of this thread's position: those of the workgroups before (block_base[blockIdx.x]), of the earlier
// waves and of the lanes below.  For a head that is the index of its run.  Called by all threads: one barrier inside.  (The flag need
// not be a run's head: the map window ranks the records it keeps with it.)
__device__ __forceinline__ int run_rank_in_block(bool head, const int* __restrict__ block_base) {
  __shared__ int s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long heads = __ballot(head);
  if (lane == 0) s_w[wave] = __popcll(heads);
  __syncthreads();
  int r = block_base[blockIdx.x] + __popcll(heads & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
  for (int k = 0; k < wave; k++) r += s_w[k];
  return r;
}

// A point source hands out the fields of input point p: SoA planes, or strided records.
struct PlanePoints {
  const float* __restrict__ x; const float* __restrict__ y; const float* __restrict__ z; const float* __restrict__ w;   // w nullable
  __device__ __forceinline__ bool has_w() const { return w != nullptr; }
  __device__ __forceinline__ void xyz(int p, float& a, float& b, float& c) const { a = x[p]; b = y[p]; c = z[p]; }
  __device__ __forceinline__ float wf(int p) const { return w[p]; }
};
__device__ __forceinline__ float record_field(const unsigned char* __restrict__ rec, int off) { return *reinterpret_cast<const float*>(rec + off); }
struct RecordPoints {
  const unsigned char* __restrict__ data; int step, ox, oy, oz, oi;   // oi < 0: no fourth field
  __device__ __forceinline__ bool has_w() const { return oi >= 0; }
  __device__ __forceinline__ const unsigned char* rec(int p) const { return data + (size_t)p * step; }
  __device__ __forceinline__ void xyz(int p, float& a, float& b, float& c) const {
    const unsigned char* r = rec(p);
    a = record_field(r, ox); b = record_field(r, oy); c = record_field(r, oz);
  }
  __device__ __forceinline__ float wf(int p) const { return record_field(rec(p), oi); }
};

// pcl::CentroidPoint over the run that starts at sorted position i with key `key`: FLOAT accumulators, the run's points in ascending
// input index (order[] of a stable sort), one division per field.  The additions are a chain by definition; the gathers that feed
// them are not: four points in flight.  c[3] is 0 for a source without a fourth field.
template <class Keys, class Points, class I>
__device__ __forceinline__ void run_centroid(const Keys& K, typename Keys::Value key, const Points& P, const int* __restrict__ order, I i,
                                             I n, float* c) {
  float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
  const bool has_w = P.has_w();
  I j = i;
  for (; j + 3 < n && K.is(j + 3, key); j += 4) {   // sorted keys: position j + 3 in the run implies the three before it
    const int p0 = order[j], p1 = order[j + 1], p2 = order[j + 2], p3 = order[j + 3];
    float x0, y0, z0, x1, y1, z1, x2, y2, z2, x3, y3, z3;
    P.xyz(p0, x0, y0, z0); P.xyz(p1, x1, y1, z1); P.xyz(p2, x2, y2, z2); P.xyz(p3, x3, y3, z3);
    sx += x0; sy += y0; sz += z0; sx += x1; sy += y1; sz += z1; sx += x2; sy += y2; sz += z2; sx += x3; sy += y3; sz += z3;
    if (has_w) { const float w0 = P.wf(p0), w1 = P.wf(p1), w2 = P.wf(p2), w3 = P.wf(p3); sw += w0; sw += w1; sw += w2; sw += w3; }
  }
  for (; j < n && K.is(j, key); j++) {
    const int p = order[j];
    float x0, y0, z0;
    P.xyz(p, x0, y0, z0);
    sx += x0; sy += y0; sz += z0;
    if (has_w) sw += P.wf(p);
  }
  const float m = (float)(j - i);
  c[0] = sx / m; c[1] = sy / m; c[2] = sz / m;
  c[3] = has_w ? sw / m : 0.f;
}

}  // namespace
}  // namespace lsr

// What every kernel that returns the sums of an NDT pass shares (the derivative kernels of ndt.hip, the pose-scoring kernel of
// pose_search.hip): the neighbourhood offsets, the address-space typedefs of the table reads, and the canonical sum (canon::) —
// the definition that makes a pass's sums a function of its input and not of the launch.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "ndt.hpp"

namespace lsr {

// sum partner inside a quad of lanes via DPP quad_perm (no LDS traffic): CTRL 0xB1 = [1,0,3,2], 0x4E = [2,3,0,1]
template <int CTRL>
__device__ __forceinline__ double dpp_quad_xor(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

template <int NOFF>
struct Offsets;
template <>
struct Offsets<1> {
  static __device__ __forceinline__ void get(int o, int& dx, int& dy, int& dz) { dx = dy = dz = 0; }
};
template <>
struct Offsets<7> {
  static __device__ __forceinline__ void get(int o, int& dx, int& dy, int& dz) {
    dx = (o == 1) - (o == 2);
    dy = (o == 3) - (o == 4);
    dz = (o == 5) - (o == 6);
  }
};
template <>
struct Offsets<27> {
  static __device__ __forceinline__ void get(int o, int& dx, int& dy, int& dz) {
    dx = o / 9 - 1;
    dy = (o / 3) % 3 - 1;
    dz = o % 3 - 1;
  }
};

// pointers read from a problem record are generic to the compiler (flat loads, which also count against the LDS counter): say
// where they point
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const v4f LdsV4;
typedef __attribute__((address_space(1))) const v4f GlbV4;
typedef __attribute__((address_space(1))) const float GlbFloat;
typedef __attribute__((address_space(1))) const int GlbInt;

// Ordering of LDS traffic inside ONE wave: its lanes run in lockstep and the LDS unit executes a wave's operations in
// order, so "lane 0 wrote, every lane reads" needs no workgroup barrier — only that the compiler keeps the order and the
// writes have been issued.
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The canonical sum of a pass (the definition: ndt.hip, "The canonical sum of a pass: one input, one answer").
namespace canon {
constexpr int TILE_PITCH = 68;    // floats per row of a staging tile: rows 16-byte aligned, consecutive rows four banks apart
constexpr int TILE_ROWS = 16;     // values staged at a time (a Hessian pass goes through the tile twice)
constexpr int TILE_FLOATS = TILE_ROWS * TILE_PITCH;

__device__ __forceinline__ double quantum(const int k) { return __hiloint2double((1023 + 62 - 31 * (k + 1)) << 20, 0); }
__device__ __forceinline__ double iquantum(const int k) { return __hiloint2double((1023 - 62 + 31 * (k + 1)) << 20, 0); }

// piece k of the exact split of t: the pieces of one value can be formed independently of each other (five lanes, one piece
// each) because t minus its multiple-of-q_(k-1) part is exact in fp64.  |t| >= 2^62 or NaN: no piece, *poison raised.
__device__ __forceinline__ int piece(const double t, const int k, bool* poison) {
  *poison = !(fabs(t) < 4611686018427387904.0);
  if (*poison) return 0;
  double r = t;
  if (k > 0) r = t - trunc(t * iquantum(k - 1)) * quantum(k - 1);   // |r| < q_(k-1) = 2^31 q_k, exact
  return (int)(r * iquantum(k));                                     // truncation toward zero
}

// The way back: the integer sum m of the pieces k of a value is worth m q_k (an int64 below 2^53 converts exactly), and the five
// bins are folded smallest quantum first, in this fixed order; a raised poison slot (overflow / NaN partial) makes every value of the
// pass poisoned().
__device__ __forceinline__ double bin_value(const long long m, const int k) { return (double)m * quantum(k); }
__device__ __forceinline__ double fold(const double b0, const double b1, const double b2, const double b3, const double b4) {
  return (((b4 + b3) + b2) + b1) + b0;
}
__device__ __forceinline__ double poisoned() { return __longlong_as_double(0x7FF8000000000000ll); }

// 8 consecutive fp32 terms at p (16-byte aligned, LDS), lanes l & 7 = run: the chunk total of a gradient-only pass, in every lane
__device__ __forceinline__ double reduce_grad(const float* p) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 a = *reinterpret_cast<const f4*>(p), b = *reinterpret_cast<const f4*>(p + 4);
  double t = (double)a.x;
  t += (double)a.y; t += (double)a.z; t += (double)a.w;
  t += (double)b.x; t += (double)b.y; t += (double)b.z; t += (double)b.w;
  t += dpp_quad_xor<0xB1>(t);    // runs {0<->1, 2<->3, ...}
  t += dpp_quad_xor<0x4E>(t);    // pairs of runs
  t += dpp_quad_xor<0x141>(t);   // row_half_mirror: lane 7 - l of the 8-lane group = the other quad (whose lanes all hold its sum)
  return t;
}
// 16 consecutive fp32 terms at p, lanes l & 3 = run: the chunk total of a pass with Hessian, in every lane of the quad
__device__ __forceinline__ double reduce_hess(const float* p) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 a = *reinterpret_cast<const f4*>(p), b = *reinterpret_cast<const f4*>(p + 4), c = *reinterpret_cast<const f4*>(p + 8),
           d = *reinterpret_cast<const f4*>(p + 12);
  double t = (double)a.x;
  t += (double)a.y; t += (double)a.z; t += (double)a.w;
  t += (double)b.x; t += (double)b.y; t += (double)b.z; t += (double)b.w;
  t += (double)c.x; t += (double)c.y; t += (double)c.z; t += (double)c.w;
  t += (double)d.x; t += (double)d.y; t += (double)d.z; t += (double)d.w;
  t += dpp_quad_xor<0xB1>(t);
  t += dpp_quad_xor<0x4E>(t);
  return t;
}
// piece k of chunk total t of value v -> a workgroup's LDS bins [NDT_NBINS][32] (poison: slot 31 of bin 0, raised by the k = 0 caller)
__device__ __forceinline__ void add_piece_lds(unsigned long long* ibin, const int v, const int k, const double t) {
  bool poison;
  const int m = piece(t, k, &poison);
  if (m != 0) atomicAdd(&ibin[k * 32 + v], (unsigned long long)(long long)m);
  if (poison && k == 0) atomicAdd(&ibin[31], 1ull);
}
}  // namespace canon

}  // namespace lsr

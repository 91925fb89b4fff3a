// The per-point arithmetic of the IMU de-skew — LidarUndistortion::adjustDistortion (scanmatcher/include/scanmatcher/
// lidar_undistortion.hpp:110-226, called on the raw cloud at scanmatcher_component.cpp:204-208) — shared by the kernels of
// csrc/deskew.hip and, compiled for the host under LSR_HOST_EMU, by tools/deskew_host_emu (tests/test_deskew_cpu.py).
//
// The reference is one loop over the points with two carried states.  Both reduce to order-free quantities:
//   half_passed   true from the first point on whose first-branch angle h_i satisfies h_i - start > pi
//                 -> H = min{i : flag_i}; points i <= H take the first branch, points i > H the second;
//   the IMU pointer walks forward from where the previous point left it; a skipped point does not move it
//                 -> on a table with non-decreasing stamps the pointer after point i is the inclusive prefix maximum of
//                    f'_j = (|t_j - stamp[f_j]| > scan_period) ? 0 : f_j, f_j = first entry with t_j < stamp (or the last one).
// Every comparison is written the way the reference writes it, so a NaN takes the path it takes there.
// Number formats: angles, rel_time, interpolation ratios and poses are f32; an f32 compared or combined with a double constant
// (M_PI, scan_period) is promoted, the result rounded back to f32 when it is stored; t = scan_time + rel_time is f64.
#pragma once
#ifndef LSR_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#include "imu_queue.hpp"

namespace lsr {

constexpr double DESKEW_PI = 3.14159265358979323846;

// pose of the sensor at one instant, as the table holds it
struct DeskewPose { float rpy[3], shift[3], velo[3]; };

__host__ __device__ inline float deskew_ori(const float x, const float y) { return -atan2f(y, x); }

// end orientation brought into (start + pi, start + 3 pi]
__host__ __device__ inline float deskew_end(const float start, float end) {
#pragma clang fp contract(off)
  if ((double)(end - start) > 3.0 * DESKEW_PI) end = (float)((double)end - 2.0 * DESKEW_PI);
  else if ((double)(end - start) < DESKEW_PI) end = (float)((double)end + 2.0 * DESKEW_PI);
  return end;
}

// first branch (half_passed still false): h_i and flag_i
__host__ __device__ inline float deskew_first_branch(const float ori, const float start, bool* flag) {
#pragma clang fp contract(off)
  float h = ori;
  if ((double)h < (double)start - DESKEW_PI * 0.5) h = (float)((double)h + 2.0 * DESKEW_PI);
  else if ((double)h > (double)start + DESKEW_PI * 1.5) h = (float)((double)h - 2.0 * DESKEW_PI);
  *flag = (double)(h - start) > DESKEW_PI;
  return h;
}

// second branch (half_passed true)
__host__ __device__ inline float deskew_second_branch(const float ori, const float end) {
#pragma clang fp contract(off)
  float h = (float)((double)ori + 2.0 * DESKEW_PI);
  if ((double)h < (double)end - 1.5 * DESKEW_PI) h = (float)((double)h + 2.0 * DESKEW_PI);
  else if ((double)h > (double)end + 0.5 * DESKEW_PI) h = (float)((double)h - 2.0 * DESKEW_PI);
  return h;
}

__host__ __device__ inline float deskew_rel_time(const float ori_h, const float start, const float diff, const double scan_period) {
#pragma clang fp contract(off)
  const float q = (ori_h - start) / diff;
  return (float)((double)q * scan_period);
}

// f: first entry k of entry[0 .. m) with t < stamp[k], m - 1 if there is none (a NaN t ends there too).  Stamps are
// non-decreasing, so the predicate is monotone and a bisection finds the first.  `entry` points at entry 0 (entry[-1] is valid).
__host__ __device__ inline int deskew_front(const ImuEntry* entry, const int m, const double t) {
  int lo = 0, hi = m - 1;   // answer in [lo, hi]; hi = m - 1 is the fallback
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t < entry[mid].stamp) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__host__ __device__ inline bool deskew_skips(const ImuEntry* entry, const int p, const double t, const double scan_period) {
  return fabs(t - entry[p].stamp) > scan_period;
}

// what point j contributes to the prefix maximum
__host__ __device__ inline int deskew_front_valid(const ImuEntry* entry, const int f, const double t, const double scan_period) {
  return deskew_skips(entry, f, t, scan_period) ? 0 : f;
}

// pose of a non-skipped point at entry p
__host__ __device__ inline void deskew_pose(const ImuEntry* entry, const int p, const double t, DeskewPose* out) {
#pragma clang fp contract(off)
  const ImuEntry& F = entry[p];
  if (t > F.stamp) {
    for (int k = 0; k < 3; k++) { out->rpy[k] = F.rpy[k]; out->shift[k] = F.shift[k]; out->velo[k] = F.velo[k]; }
    return;
  }
  const ImuEntry& B = entry[p - 1];
  const float rf = (float)((t - B.stamp) / (F.stamp - B.stamp));
  const float rb = (float)(1.0 - (double)rf);
  for (int k = 0; k < 3; k++) {
    out->rpy[k] = F.rpy[k] * rf + B.rpy[k] * rb;
    out->shift[k] = F.shift[k] * rf + B.shift[k] * rb;
    out->velo[k] = F.velo[k] * rf + B.velo[k] * rb;
  }
}

// R = Rz(yaw) * Ry(pitch) * Rx(roll), f32, row-major
__host__ __device__ inline void deskew_rotation(const float* rpy, float* R) {
#pragma clang fp contract(off)
  const float sr = sinf(rpy[0]), cr = cosf(rpy[0]);
  const float sp = sinf(rpy[1]), cp = cosf(rpy[1]);
  const float sy = sinf(rpy[2]), cy = cosf(rpy[2]);
  R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
  R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
  R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

// p' = R_s^-1 * (R_c * p + (shift_c - shift_s - velo_s * rel)); R_s^-1 is the transpose of R_s
__host__ __device__ inline void deskew_transform(const float* Rs, const DeskewPose& start, const DeskewPose& cur, const float rel,
                                                 const float x, const float y, const float z, float* out) {
#pragma clang fp contract(off)
  float Rc[9];
  deskew_rotation(cur.rpy, Rc);
  float v[3];
  for (int r = 0; r < 3; r++) {
    const float d = cur.shift[r] - start.shift[r] - start.velo[r] * rel;
    v[r] = ((Rc[3 * r] * x + Rc[3 * r + 1] * y) + Rc[3 * r + 2] * z) + d;
  }
  for (int c = 0; c < 3; c++) out[c] = (Rs[c] * v[0] + Rs[3 + c] * v[1]) + Rs[6 + c] * v[2];
}

}  // namespace lsr

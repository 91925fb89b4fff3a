// The head of the frontend's cloud callback and the use_odom guess of receiveCloud (include/lidarslam_reg.h):
//   lookupTransform(robot_frame_id_, msg->header.frame_id) + tf2::doTransform(*msg, transformed_msg, transform)
//   (scanmatcher/src/scanmatcher_component.cpp:188-199) — the sensor -> robot matrix and the records -> records transform of a raw
//   payload (the form fused into the source ingest is lsr_set_input_source_pc2_tf, inputs.hip);
//   sim_trans * previous_odom_mat_.inverse() * odom_mat (:333-348).
// Host-side orchestration only: the kernel is pc2_transform_kernel (cloud_codec.hip).
#include <cmath>
#include <cstring>

#include "api_internal.hpp"

using namespace lsr;

namespace {

// inverse of a general column-major 4x4 in double: adjugate over determinant (2x2 minors of the two row pairs)
void mat4_inverse(const double* m, double* inv) {
  const double a00 = m[0], a10 = m[1], a20 = m[2], a30 = m[3], a01 = m[4], a11 = m[5], a21 = m[6], a31 = m[7];
  const double a02 = m[8], a12 = m[9], a22 = m[10], a32 = m[11], a03 = m[12], a13 = m[13], a23 = m[14], a33 = m[15];
  const double s0 = a00 * a11 - a10 * a01, s1 = a00 * a12 - a10 * a02, s2 = a00 * a13 - a10 * a03;
  const double s3 = a01 * a12 - a11 * a02, s4 = a01 * a13 - a11 * a03, s5 = a02 * a13 - a12 * a03;
  const double c5 = a22 * a33 - a32 * a23, c4 = a21 * a33 - a31 * a23, c3 = a21 * a32 - a31 * a22;
  const double c2 = a20 * a33 - a30 * a23, c1 = a20 * a32 - a30 * a22, c0 = a20 * a31 - a30 * a21;
  const double d = 1.0 / (s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0);
  inv[0] = (a11 * c5 - a12 * c4 + a13 * c3) * d;
  inv[4] = (-a01 * c5 + a02 * c4 - a03 * c3) * d;
  inv[8] = (a31 * s5 - a32 * s4 + a33 * s3) * d;
  inv[12] = (-a21 * s5 + a22 * s4 - a23 * s3) * d;
  inv[1] = (-a10 * c5 + a12 * c2 - a13 * c1) * d;
  inv[5] = (a00 * c5 - a02 * c2 + a03 * c1) * d;
  inv[9] = (-a30 * s5 + a32 * s2 - a33 * s1) * d;
  inv[13] = (a20 * s5 - a22 * s2 + a23 * s1) * d;
  inv[2] = (a10 * c4 - a11 * c2 + a13 * c0) * d;
  inv[6] = (-a00 * c4 + a01 * c2 - a03 * c0) * d;
  inv[10] = (a30 * s4 - a31 * s2 + a33 * s0) * d;
  inv[14] = (-a20 * s4 + a21 * s2 - a23 * s0) * d;
  inv[3] = (-a10 * c3 + a11 * c1 - a12 * c0) * d;
  inv[7] = (a00 * c3 - a01 * c1 + a02 * c0) * d;
  inv[11] = (-a30 * s3 + a31 * s1 - a32 * s0) * d;
  inv[15] = (a20 * s3 - a21 * s1 + a22 * s0) * d;
}

void mat4_mul(const double* A, const double* B, double* C) {  // column-major C = A * B
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++) {
      double acc = 0;
      for (int k = 0; k < 4; k++) acc += A[r + 4 * k] * B[k + 4 * c];
      C[r + 4 * c] = acc;
    }
}

}  // namespace

extern "C" {

int lsr_sensor_transform_matrix(const lsr_sensor_transform* tf, float* out12) {
  if (!tf || !out12) { set_last_error("null sensor transform or output"); return LSR_ERR_INVALID_ARGUMENT; }
  lsr_submap pose;
  std::memset(&pose, 0, sizeof(pose));
  for (int k = 0; k < 3; k++) pose.position[k] = tf->translation[k];
  for (int k = 0; k < 4; k++) pose.orientation[k] = tf->rotation_xyzw[k];
  double M[16];
  submap_pose_matrix(pose, M);   // the expression order every pose message of the library goes through; no normalisation
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) out12[4 * r + c] = (float)M[r + 4 * c];
  return LSR_OK;
}

int lsr_transform_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, const lsr_sensor_transform* tf,
                      int on_device, void* out_data) {
  LSR_CHECK_HANDLE(h);
  int st = check_layout(layout);
  if (st) return st;
  SensorTf12 T;
  if ((st = lsr_sensor_transform_matrix(tf, T.m))) return st;
  if (n_points == 0) return LSR_OK;   // nothing to move: the pointers are not looked at (lsr_deskew_pc2 differs: it still reports)
  if ((st = arg_error(check_records_in_out(data, out_data, n_points, layout->point_step)))) return st;
  const int step = (int)layout->point_step, ox = (int)layout->offset_x, oy = (int)layout->offset_y, oz = (int)layout->offset_z;
  // device records: returns when the records are complete, for a reader on any stream — a mailbox word, no copy, no synchronisation;
  // host records: the copy down and its synchronisation are the wait
  return records_in_records_out(h, data, out_data, n_points * (size_t)layout->point_step, on_device != 0, [&](const void* d_in, void* d_out) {
    return pc2_transform(d_in, d_out, step, ox, oy, oz, n_points, T, h->scratch, h->stream, on_device != 0);
  });
}

int lsr_odom_guess(const float* sim_trans16, const float* previous_odom16, const float* odom16, float* guess16) {
  if (!sim_trans16 || !previous_odom16 || !odom16 || !guess16) { set_last_error("null matrix"); return LSR_ERR_INVALID_ARGUMENT; }
  // `previous_odom_mat_ != Eigen::Matrix4f::Identity()` (:344) is false: the first scan.  Entry by entry with ==, as Eigen compares
  // (the bits of the identity, and -0 for a 0; a NaN entry is "not the identity")
  bool is_identity = true;
  for (int k = 0; k < 16; k++) is_identity = is_identity && previous_odom16[k] == ((k % 5 == 0) ? 1.f : 0.f);
  if (is_identity) {
    std::memmove(guess16, sim_trans16, sizeof(float) * 16);
    return LSR_OK;
  }
  double S[16], P[16], O[16], Pi[16], SP[16], G[16];
  for (int k = 0; k < 16; k++) { S[k] = sim_trans16[k]; P[k] = previous_odom16[k]; O[k] = odom16[k]; }
  mat4_inverse(P, Pi);
  mat4_mul(S, Pi, SP);
  mat4_mul(SP, O, G);
  for (int k = 0; k < 16; k++) guess16[k] = (float)G[k];
  return LSR_OK;
}

}  // extern "C"

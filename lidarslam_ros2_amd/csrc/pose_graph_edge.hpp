// The per-edge arithmetic of the pose-graph optimisation — g2o's VertexSE3 / EdgeSE3 with identity information as
// GraphBasedSlamComponent::doPoseAdjustment sets them up (graph_based_slam_component.cpp:267-319), restated from knowledge of g2o
// (DESIGN.md 4 "Pose-graph optimisation": unpinned) — shared by the kernels of csrc/pose_graph.hip and, compiled for the host under
// LSR_HOST_EMU, by tools/pose_graph_host_emu (tests/test_pose_graph_cpu.py).  Everything is fp64; no FMA contraction (the host build and the device
// build then run the same operations).
//   pose        X = (R, t), R row-major
//   increment   delta = (dt, dq): w = 1 - |dq|^2; w < 0 -> identity rotation, else the rotation of the quaternion (sqrt(w), dq);
//               X <- X * Delta(delta)                                                                   (fromVectorMQT, oplus)
//   error       e = toVectorMQT(Zinv * Xfrom^-1 * Xto): its translation, and the vector part of its unit quaternion with w >= 0
//   Jacobians   the exact derivatives of e with respect to delta_from and delta_to at 0:
//               A = Xfrom^-1 Xto, E = Zinv A, q_e = s q_z (x) q_a with s = +-1 making w_e >= 0
//               de/dto   = [[R_E, 0], [0, w_e I + [v_e]x]]
//               de/dfrom = [[-R_Zinv, 2 R_Zinv [t_A]x], [0, columns -s vec(q_z (x) (0, u_a) (x) q_a)]]
#pragma once
#ifndef LSR_HOST_EMU
#include <hip/hip_runtime.h>
#endif

namespace lsr {

struct PgPose { double R[9]; double t[3]; };

// column-major 4x4 (the layout of lsr_loop_edge.relative_pose and of lsr_assemble_map's poses16) <-> PgPose
__host__ __device__ inline void pg_pose_from_col16(const double* M, PgPose* X) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) X->R[3 * r + c] = M[4 * c + r];
    X->t[r] = M[12 + r];
  }
}
__host__ __device__ inline void pg_pose_to_col16(const PgPose& X, double* M) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) M[4 * c + r] = X.R[3 * r + c];
    M[12 + r] = X.t[r];
    M[4 * r + 3] = 0.0;
  }
  M[15] = 1.0;
}

// Isometry3d::inverse(): (R^T, -R^T t)
__host__ __device__ inline void pg_inverse(const PgPose& X, PgPose* out) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) out->R[3 * r + c] = X.R[3 * c + r];
    out->t[r] = -((X.R[r] * X.t[0] + X.R[3 + r] * X.t[1]) + X.R[6 + r] * X.t[2]);
  }
}

// A * B
__host__ __device__ inline void pg_compose(const PgPose& A, const PgPose& B, PgPose* out) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) out->R[3 * r + c] = (A.R[3 * r] * B.R[c] + A.R[3 * r + 1] * B.R[3 + c]) + A.R[3 * r + 2] * B.R[6 + c];
    out->t[r] = ((A.R[3 * r] * B.t[0] + A.R[3 * r + 1] * B.t[1]) + A.R[3 * r + 2] * B.t[2]) + A.t[r];
  }
}

// Quaterniond(Matrix3d) then normalize(): q = (w, x, y, z); the sign is whatever the branch gives
__host__ __device__ inline void pg_quat_from_matrix(const double* R, double* q) {
#pragma clang fp contract(off)
  const double tr = (R[0] + R[4]) + R[8];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    q[0] = s / 4.0;
    q[1] = (R[7] - R[5]) / s;
    q[2] = (R[2] - R[6]) / s;
    q[3] = (R[3] - R[1]) / s;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    const double s = sqrt(((1.0 + R[4 * i]) - R[4 * j]) - R[4 * k]) * 2.0;
    q[1 + i] = s / 4.0;
    q[1 + j] = (R[3 * j + i] + R[3 * i + j]) / s;
    q[1 + k] = (R[3 * k + i] + R[3 * i + k]) / s;
    q[0] = (R[3 * k + j] - R[3 * j + k]) / s;
  }
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int a = 0; a < 4; a++) q[a] = q[a] / n;
}

// Quaterniond::toRotationMatrix()
__host__ __device__ inline void pg_matrix_from_quat(const double w, const double x, const double y, const double z, double* R) {
#pragma clang fp contract(off)
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w);       R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w);       R[7] = 2.0 * (y * z + x * w);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// Hamilton product, (w, x, y, z)
__host__ __device__ inline void pg_qmul(const double* a, const double* b, double* out) {
#pragma clang fp contract(off)
  out[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
  out[1] = ((a[0] * b[1] + b[0] * a[1]) + a[2] * b[3]) - a[3] * b[2];
  out[2] = ((a[0] * b[2] + b[0] * a[2]) + a[3] * b[1]) - a[1] * b[3];
  out[3] = ((a[0] * b[3] + b[0] * a[3]) + a[1] * b[2]) - a[2] * b[1];
}

// fromVectorMQT
__host__ __device__ inline void pg_increment(const double* d6, PgPose* D) {
#pragma clang fp contract(off)
  const double w = 1.0 - ((d6[3] * d6[3] + d6[4] * d6[4]) + d6[5] * d6[5]);
  if (w < 0.0) {
    for (int a = 0; a < 9; a++) D->R[a] = (a % 4 == 0) ? 1.0 : 0.0;
  } else {
    pg_matrix_from_quat(sqrt(w), d6[3], d6[4], d6[5], D->R);
  }
  for (int a = 0; a < 3; a++) D->t[a] = d6[a];
}

// X (+) delta = X * Delta(delta)
__host__ __device__ inline void pg_oplus(const PgPose& X, const double* d6, PgPose* out) {
  PgPose D;
  pg_increment(d6, &D);
  pg_compose(X, D, out);
}

// e6 of one edge; Zinv is the inverse of the measurement
__host__ __device__ inline void pg_edge_error(const PgPose& Zinv, const PgPose& Xf, const PgPose& Xt, double* e6) {
  PgPose Xfi, A, E;
  pg_inverse(Xf, &Xfi);
  pg_compose(Xfi, Xt, &A);
  pg_compose(Zinv, A, &E);
  double q[4];
  pg_quat_from_matrix(E.R, q);
  const double s = q[0] < 0.0 ? -1.0 : 1.0;
  for (int a = 0; a < 3; a++) { e6[a] = E.t[a]; e6[3 + a] = s * q[1 + a]; }
}

// e6 and both Jacobians (row-major 6x6: J[6 * row + col] = d e_row / d delta_col)
__host__ __device__ inline void pg_edge_linearize(const PgPose& Zinv, const PgPose& Xf, const PgPose& Xt, double* e6, double* Jf,
                                                  double* Jt) {
#pragma clang fp contract(off)
  PgPose Xfi, A, E;
  pg_inverse(Xf, &Xfi);
  pg_compose(Xfi, Xt, &A);
  pg_compose(Zinv, A, &E);
  double q[4];
  pg_quat_from_matrix(E.R, q);
  const double se = q[0] < 0.0 ? -1.0 : 1.0;
  for (int a = 0; a < 3; a++) { e6[a] = E.t[a]; e6[3 + a] = se * q[1 + a]; }

  double qz[4], qa[4], qe[4];
  pg_quat_from_matrix(Zinv.R, qz);
  pg_quat_from_matrix(A.R, qa);
  pg_qmul(qz, qa, qe);
  const double s = qe[0] >= 0.0 ? 1.0 : -1.0;
  for (int a = 0; a < 4; a++) qe[a] = s * qe[a];

  for (int a = 0; a < 36; a++) { Jf[a] = 0.0; Jt[a] = 0.0; }
  // de/dto
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) Jt[6 * r + c] = E.R[3 * r + c];
  Jt[6 * 3 + 3] = qe[0];  Jt[6 * 3 + 4] = -qe[3]; Jt[6 * 3 + 5] = qe[2];
  Jt[6 * 4 + 3] = qe[3];  Jt[6 * 4 + 4] = qe[0];  Jt[6 * 4 + 5] = -qe[1];
  Jt[6 * 5 + 3] = -qe[2]; Jt[6 * 5 + 4] = qe[1];  Jt[6 * 5 + 5] = qe[0];
  // de/dfrom
  const double* t = A.t;
  const double K[9] = {0.0, -t[2], t[1], t[2], 0.0, -t[0], -t[1], t[0], 0.0};   // [t_A]x
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      Jf[6 * r + c] = -Zinv.R[3 * r + c];
      Jf[6 * r + 3 + c] = 2.0 * ((Zinv.R[3 * r] * K[c] + Zinv.R[3 * r + 1] * K[3 + c]) + Zinv.R[3 * r + 2] * K[6 + c]);
    }
  for (int a = 0; a < 3; a++) {
    double u[4] = {0.0, 0.0, 0.0, 0.0}, zu[4], p[4];
    u[1 + a] = 1.0;
    pg_qmul(qz, u, zu);
    pg_qmul(zu, qa, p);
    for (int r = 0; r < 3; r++) Jf[6 * (3 + r) + 3 + a] = -s * p[1 + r];
  }
}

}  // namespace lsr

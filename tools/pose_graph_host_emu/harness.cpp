// TEST INFRASTRUCTURE.  csrc/pose_graph_edge.hpp compiled for the CPU: the edge error, both Jacobians and the vertex update of the
// pose-graph optimisation exactly as the kernels of csrc/pose_graph.hip evaluate them, checked against the numpy restatement
// (tests/pose_graph_numpy.py) without a GPU (tests/test_pose_graph_cpu.py).  Poses are column-major 4x4 fp64.
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off harness.cpp -o libposegraphemu.so
#include <cmath>

#define __device__
#define __host__
#define LSR_HOST_EMU 1
#include "../../lidarslam_ros2_amd/csrc/pose_graph_edge.hpp"

using namespace lsr;

namespace {
void load3(const double* Z16, const double* Xf16, const double* Xt16, PgPose* Zinv, PgPose* Xf, PgPose* Xt) {
  PgPose Z;
  pg_pose_from_col16(Z16, &Z);
  pg_inverse(Z, Zinv);
  pg_pose_from_col16(Xf16, Xf);
  pg_pose_from_col16(Xt16, Xt);
}
}  // namespace

extern "C" {

// Z16: the measurement from^-1 * to, as lsr_pose_edge carries it
void emu_pg_error(const double* Z16, const double* Xf16, const double* Xt16, double* e6) {
  PgPose Zinv, Xf, Xt;
  load3(Z16, Xf16, Xt16, &Zinv, &Xf, &Xt);
  pg_edge_error(Zinv, Xf, Xt, e6);
}

// Jf / Jt: row-major 6x6
void emu_pg_linearize(const double* Z16, const double* Xf16, const double* Xt16, double* e6, double* Jf, double* Jt) {
  PgPose Zinv, Xf, Xt;
  load3(Z16, Xf16, Xt16, &Zinv, &Xf, &Xt);
  pg_edge_linearize(Zinv, Xf, Xt, e6, Jf, Jt);
}

void emu_pg_oplus(const double* X16, const double* d6, double* out16) {
  PgPose X, Y;
  pg_pose_from_col16(X16, &X);
  pg_oplus(X, d6, &Y);
  pg_pose_to_col16(Y, out16);
}

// matrix -> unit quaternion (w, x, y, z), sign as the branch gives it, and back
void emu_pg_quat_from_matrix(const double* X16, double* q4) {
  PgPose X;
  pg_pose_from_col16(X16, &X);
  pg_quat_from_matrix(X.R, q4);
}

}  // extern "C"

// Pose-graph optimisation on the device (csrc/pose_graph.hip): what a handle keeps for it.
#pragma once
#include "common.hpp"
#include "pose_graph_edge.hpp"

namespace lsr {

constexpr int PG_MAX_VERTICES = LSR_POSE_GRAPH_MAX_VERTICES;
constexpr int PG_MAX_BAND = LSR_POSE_GRAPH_MAX_BAND;
constexpr int PG_MAX_OFFBAND = LSR_POSE_GRAPH_MAX_OFFBAND_EDGES;             // above it the dense part is blocked (pose_graph_dense.hip)
constexpr int PG_LONG_MAX_OFFBAND = LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES;
constexpr int PG_MAX_EDGES = 1 << 20;
constexpr int PG_MAX_TRIALS = 10;   // g2o's maxTrialsAfterFailure

// one edge as the kernels read it
struct PgEdge {
  int from, to;
  int slot;     // -1: inside the band (or into the fixed vertex); r >= 0: rows 6r .. 6r+5 of the low-rank factor U
  int pad;
  PgPose Zinv;  // inverse of the measurement
};

// what the host controller reads back: after a linearisation chi2 and max_diag, after a trial trial_chi2, scale and fail
struct PgScalars {
  double chi2, max_diag, trial_chi2, scale;
  int fail;     // 0: solved; 1: the band factor met a non-positive or non-finite pivot; 2: the dense factor did
  int pad;
};

struct PgWorkspace {
  DevBuf<PgPose> X, Xt;            // accepted / trial poses (g2o's push / pop)
  DevBuf<PgEdge> edges;
  DevBuf<int> inc_start, inc_edge; // CSR: the edges at every vertex, in edge order
  DevBuf<int> off_edge;            // edge of every slot of U
  DevBuf<double> e, Jf, Jt, ete;   // per edge
  DevBuf<double> AB, LB;           // H's band part, lower, column j at [j * (hw + 1)]; its Cholesky factor for the current lambda
  DevBuf<double> b, diag, x;       // b = -sum J^T e; the diagonal of the whole H; the increment
  DevBuf<double> W;                // [n][1 + 6L]: column 0 b -> B^-1 b, the others U^T -> B^-1 U^T
  DevBuf<double> C, g;             // I + U B^-1 U^T and U B^-1 b -> z
  DevBuf<double> z;                // the blocked path (more than PG_MAX_OFFBAND slots) keeps y in g and writes z here
  bool profile = false;            // LSR_PROFILE: three stages of every trial are bracketed with events ...
  double stage_ms[3] = {0, 0, 0};  // ... and summed over the call: band solve (right-hand sides included), dense part, row combine
  DevBuf<PgScalars> d_sc;
  PinBuf<PgScalars> h_sc;
  PinBuf<unsigned char> h_up;      // staging of the uploads
  PinBuf<double> h_out;            // the accepted poses on their way out
};

// The whole of optimizer.optimize(max_iterations) (graph_based_slam_component.cpp:317-318).  Arguments are checked by the caller.
// A host loop drives it: per linearisation and per trial it reads PgScalars back (one small copy) and decides accept / reject.
// max_offband: the caller's limit on the slots of U.  Up to PG_MAX_OFFBAND of them the dense part is pg_dense_solve and the rows are
// combined by pg_combine; above, pose_graph_dense_solve and pose_graph_combine_rows.
int pose_graph_optimize(PgWorkspace& ws, const double* poses16_in, int n_vertices, const lsr_pose_edge* edges, int n_edges, int max_iterations,
                        int band, int max_offband, double* poses16_out, lsr_pose_graph_result* result, lsr_pose_graph_trace* trace,
                        hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1);

// csrc/pose_graph_dense.hip.  C (m x m, row-major, lower triangle read) = L L^T in place by tiles, g -> y (L y = g) on the way, then
// L^T z = y into z: 3 ceil(m / 64) + ceil(m / 64) launches on `stream`, none of them waiting for another workgroup.
void pose_graph_dense_solve(double* C, double* g, double* z, int m, PgScalars* sc, hipStream_t stream);
// x[row] = W[row][0] - sum_c W[row][1 + c] z[c], a wave per row
void pose_graph_combine_rows(const double* W, int ldw, int m, const double* z, int n, double* x, const PgScalars* sc, hipStream_t stream);

// the odometry edges of graph_based_slam_component.cpp:289-303 (host only)
int pose_graph_adjacent_edges(const double* poses16, int n, int num_adjacent, lsr_pose_edge* out, size_t capacity, size_t* n_out);

}  // namespace lsr

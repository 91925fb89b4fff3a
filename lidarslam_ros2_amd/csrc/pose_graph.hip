// Pose-graph optimisation on the device: GraphBasedSlamComponent::doPoseAdjustment's optimizer.optimize(10)
// (graph_based_slam_component.cpp:267-319) without g2o — VertexSE3 / EdgeSE3 with identity information under g2o's
// Levenberg-Marquardt controller (DESIGN.md 4 "Pose-graph optimisation"; the per-edge arithmetic is csrc/pose_graph_edge.hpp).
//
// One linearisation:  pg_linearize (one thread per edge: e, J_from, J_to, e^T e)
//                     pg_gather    (one thread per vertex and block offset: walks the CSR list of the vertex's edges IN EDGE ORDER and
//                                   writes its columns of the band, b and the diagonal — no floating-point atomics)
//                     pg_reduce_linearized (chi2 and max diag(H), one workgroup, fixed order)
// One trial:          H + lambda I = B + U^T U, B the block band (edges with |from - to| <= band, and every edge into the fixed vertex),
//                     U the stacked Jacobian rows of the other L edges.  Woodbury:
//                     pg_band_factor (B = L L^T, one workgroup: the only long dependent chain)
//                     pg_fill_rhs, pg_band_solve (1 + 6L independent banded solves, one lane each)
//                     pg_small_system, pg_dense_solve (C = I + U B^-1 U^T, 6L x 6L, Cholesky, z = C^-1 U B^-1 b)
//                     pg_combine (x = B^-1 b - B^-1 U^T z), pg_update (X' = X (+) x), pg_error, pg_reduce_trial (chi2(X'), scale)
//                     With more than LSR_POSE_GRAPH_MAX_OFFBAND_EDGES slots of U (lsr_optimize_pose_graph_long) pg_dense_solve and
//                     pg_combine give way to the blocked Cholesky and the wave-per-row combine of csrc/pose_graph_dense.hip.
// Hang safety: every loop below runs to a vertex, edge, band, column or slot count; no workgroup waits for another; a pivot that is
// not positive and finite sets PgScalars::fail and the kernel returns; the kernels behind it return at once.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "pose_graph.hpp"

namespace lsr {
namespace {

constexpr int PG_WG = 256;

// ---- linearisation ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PG_WG) void pg_linearize(const PgPose* __restrict__ X, const PgEdge* __restrict__ edges, int n_edges,
                                                      double* __restrict__ e, double* __restrict__ Jf, double* __restrict__ Jt,
                                                      double* __restrict__ ete) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * PG_WG + threadIdx.x;
  if (k >= n_edges) return;
  const PgEdge E = edges[k];
  double e6[6], jf[36], jt[36];
  pg_edge_linearize(E.Zinv, X[E.from], X[E.to], e6, jf, jt);
  double s = 0.0;
  for (int a = 0; a < 6; a++) { e[6 * (size_t)k + a] = e6[a]; s = s + e6[a] * e6[a]; }
  for (int a = 0; a < 36; a++) { Jf[36 * (size_t)k + a] = jf[a]; Jt[36 * (size_t)k + a] = jt[a]; }
  ete[k] = s;
}

__global__ __launch_bounds__(PG_WG) void pg_error(const PgPose* __restrict__ X, const PgEdge* __restrict__ edges, int n_edges,
                                                  double* __restrict__ ete) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * PG_WG + threadIdx.x;
  if (k >= n_edges) return;
  const PgEdge E = edges[k];
  double e6[6];
  pg_edge_error(E.Zinv, X[E.from], X[E.to], e6);
  double s = 0.0;
  for (int a = 0; a < 6; a++) s = s + e6[a] * e6[a];
  ete[k] = s;
}

// Thread (v, d), v = 1 .. n_vertices - 1, d = 0 .. band: the 6x6 block H[v][v + d] of the band part, summed over the edges at v in edge
// order, written as its share of the six columns 6(v-1) .. 6(v-1)+5 of the lower band storage.  d = 0 also writes b and the diagonal
// of the WHOLE H (off-band edges included: lambda starts from it); d = band also writes the zeros above its block.
__global__ __launch_bounds__(PG_WG) void pg_gather(const PgEdge* __restrict__ edges, const int* __restrict__ inc_start,
                                                   const int* __restrict__ inc_edge, const double* __restrict__ e,
                                                   const double* __restrict__ Jf, const double* __restrict__ Jt, int n_vertices, int band,
                                                   double* __restrict__ AB, double* __restrict__ b, double* __restrict__ diag) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * PG_WG + threadIdx.x;
  const int per = band + 1;
  if (idx >= (n_vertices - 1) * per) return;
  const int v = 1 + idx / per, d = idx % per;
  double acc[36], bv[6], dg[6];
  for (int a = 0; a < 36; a++) acc[a] = 0.0;
  for (int a = 0; a < 6; a++) { bv[a] = 0.0; dg[a] = 0.0; }
  for (int s = inc_start[v]; s < inc_start[v + 1]; s++) {
    const int k = inc_edge[s];
    const int from = edges[k].from, to = edges[k].to, slot = edges[k].slot;
    const bool is_from = from == v;
    const int other = is_from ? to : from;
    const double* Jv = (is_from ? Jf : Jt) + 36 * (size_t)k;
    const double* Jo = (is_from ? Jt : Jf) + 36 * (size_t)k;
    if (d == 0) {
      const double* ek = e + 6 * (size_t)k;
      for (int c = 0; c < 6; c++) {
        double t = 0.0, q = 0.0;
        for (int r = 0; r < 6; r++) { t = t + Jv[6 * r + c] * ek[r]; q = q + Jv[6 * r + c] * Jv[6 * r + c]; }
        bv[c] = bv[c] - t;
        dg[c] = dg[c] + q;
      }
    }
    if (slot >= 0 || (d > 0 && other != v + d)) continue;
    const double* Jr = d == 0 ? Jv : Jo;
    for (int a = 0; a < 6; a++)
      for (int c = 0; c < 6; c++) {
        double t = 0.0;
        for (int r = 0; r < 6; r++) t = t + Jv[6 * r + a] * Jr[6 * r + c];
        acc[6 * a + c] = acc[6 * a + c] + t;
      }
  }
  const int hw = 6 * band + 5, ld = hw + 1;
  const int p = v - 1;
  for (int a = 0; a < 6; a++) {
    double* col = AB + (size_t)(6 * p + a) * ld;
    if (d == 0) {
      for (int c = a; c < 6; c++) col[c - a] = acc[6 * a + c];
      b[6 * p + a] = bv[a];
      diag[6 * p + a] = dg[a];
    } else {
      for (int c = 0; c < 6; c++) col[6 * d + c - a] = acc[6 * a + c];   // 6d + c - a in [6d - 5, 6d + 5], at most hw
    }
    if (d == band)
      for (int o = 6 * band + 6 - a; o <= hw; o++) col[o] = 0.0;
  }
}

// fixed-order sum of one value per thread over the workgroup (PG_WG threads): a tree in LDS
__device__ inline double pg_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = PG_WG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + s];
    __syncthreads();
  }
  const double out = sh[0];
  __syncthreads();
  return out;
}

// one workgroup: chi2 = sum e^T e (thread t takes edges t, t + 256, ... in order, then the tree), max diag(H)
__global__ __launch_bounds__(PG_WG) void pg_reduce_linearized(const double* __restrict__ ete, int n_edges, const double* __restrict__ diag,
                                                              int n, PgScalars* __restrict__ sc) {
  __shared__ double sh[PG_WG];
  double s = 0.0, m = 0.0;
  for (int k = threadIdx.x; k < n_edges; k += PG_WG) s = s + ete[k];
  for (int k = threadIdx.x; k < n; k += PG_WG) m = fmax(m, diag[k]);
  const double chi2 = pg_block_sum(s, sh);
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = PG_WG / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0) { sc->chi2 = chi2; sc->max_diag = sh[0]; }
}

// one workgroup: chi2 of the trial poses and scale = sum x_j (lambda x_j + b_j)
__global__ __launch_bounds__(PG_WG) void pg_reduce_trial(const double* __restrict__ ete, int n_edges, const double* __restrict__ x,
                                                         const double* __restrict__ b, int n, double lambda, PgScalars* __restrict__ sc) {
#pragma clang fp contract(off)
  __shared__ double sh[PG_WG];
  double s = 0.0, q = 0.0;
  for (int k = threadIdx.x; k < n_edges; k += PG_WG) s = s + ete[k];
  for (int k = threadIdx.x; k < n; k += PG_WG) q = q + x[k] * (lambda * x[k] + b[k]);
  const double chi2 = pg_block_sum(s, sh);
  const double scale = pg_block_sum(q, sh);
  if (threadIdx.x == 0) { sc->trial_chi2 = chi2; sc->scale = scale; }
}

// ---- the band factor ------------------------------------------------------------------------------------------------------------
// B = (band part of H) + lambda I = L L^T in lower band storage, right-looking, one workgroup of 256: a window of hw + 1 columns lives
// in LDS as a ring (column c in slot c mod (hw + 1)); per column: pivot, scale, rank-1 update of the window, next column in.
// hw <= 63 (band <= 9): the update maps lane -> row offset, wave -> column offset, no division.
__global__ __launch_bounds__(PG_WG) void pg_band_factor(const double* __restrict__ AB, double lambda, int n, int hw, double* __restrict__ LB,
                                                        PgScalars* __restrict__ sc) {
  extern __shared__ double ring[];   // (hw + 1)^2
  const int ld = hw + 1, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  if (tid == 0) sc->fail = 0;
  for (int i = tid; i < ld * ld; i += PG_WG) {
    const int c = i / ld, k = i - c * ld;
    ring[i] = (c < n && c + k < n) ? AB[(size_t)c * ld + k] + (k == 0 ? lambda : 0.0) : 0.0;
  }
  __syncthreads();
  int slot = 0;   // j mod ld
  for (int j = 0; j < n; j++) {
    double* col = ring + slot * ld;
    const double piv = col[0];
    if (!(piv > 0.0) || !(piv <= DBL_MAX)) {   // the same LDS word for every thread: a uniform exit
      if (tid == 0) sc->fail = 1;
      return;
    }
    const double l = sqrt(piv);
    const double mine = tid == 0 ? l : (tid < ld ? col[tid] / l : 0.0);
    __syncthreads();
    if (tid < ld) { col[tid] = mine; LB[(size_t)j * ld + tid] = mine; }
    __syncthreads();
    const int kmax = min(hw, n - 1 - j);
    const int r = 1 + lane;
    if (r <= kmax) {
      const double lr = col[r];
      for (int c = 1 + wave; c <= r; c += PG_WG / 64) {
        int s2 = slot + c;
        if (s2 >= ld) s2 -= ld;
        ring[s2 * ld + (r - c)] -= lr * col[c];
      }
    }
    __syncthreads();
    const int nc = j + ld;   // the column that takes the slot column j leaves
    if (nc < n && tid < ld) col[tid] = (nc + tid < n) ? AB[(size_t)nc * ld + tid] + (tid == 0 ? lambda : 0.0) : 0.0;
    slot = slot + 1 == ld ? 0 : slot + 1;
  }
}

// ---- the right-hand sides ---------------------------------------------------------------------------------------------------------
// W[row][0] = b[row]; W[row][1 + 6r + q] = U[6r + q][row]: row q of the Jacobian of slot r's edge with respect to the vertex of `row`
__global__ __launch_bounds__(PG_WG) void pg_fill_rhs(const PgEdge* __restrict__ edges, const int* __restrict__ off_edge,
                                                     const double* __restrict__ Jf, const double* __restrict__ Jt, const double* __restrict__ b,
                                                     int n, int ldw, double* __restrict__ W) {
  const size_t idx = (size_t)blockIdx.x * PG_WG + threadIdx.x;
  if (idx >= (size_t)n * ldw) return;
  const int row = (int)(idx / ldw), colw = (int)(idx - (size_t)row * ldw);
  double v;
  if (colw == 0) {
    v = b[row];
  } else {
    const int r = (colw - 1) / 6, q = (colw - 1) - 6 * r;
    const int k = off_edge[r];
    const int vtx = 1 + row / 6, c = row % 6;
    v = edges[k].from == vtx ? Jf[36 * (size_t)k + 6 * q + c] : (edges[k].to == vtx ? Jt[36 * (size_t)k + 6 * q + c] : 0.0);
  }
  W[idx] = v;
}

__device__ inline double pg_readlane(double v, int lane) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(bits & 0xffffffffLL), lane);
  const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// L L^T w = rhs for every column of W, one lane per column, in place.  Both sweeps walk L column by column (contiguous): the forward
// one right-looking (the ring holds the running right-hand side of the next hw rows), the backward one left-looking (the ring holds the
// last hw solutions).  The ring is this lane's column of an LDS array [hw + 1][64]; lane k loads L[j + k][j] and the loop takes it from
// there by readlane (hw + 1 <= 64).  No lane depends on another: no barrier.
__global__ __launch_bounds__(64) void pg_band_solve(const double* __restrict__ LB, int n, int hw, double* __restrict__ W, int ldw, int nrhs,
                                                    const PgScalars* __restrict__ sc) {
  extern __shared__ double ring[];   // (hw + 1) * 64
  if (sc->fail) return;
  const int ld = hw + 1, lane = threadIdx.x;
  const int rhs = blockIdx.x * 64 + lane;
  const bool active = rhs < nrhs;
  double* w = W + (active ? rhs : 0);
  // forward
  for (int i = 0; i < ld; i++) ring[i * 64 + lane] = (active && i < n) ? w[(size_t)i * ldw] : 0.0;
  int slot = 0;
  double lk = lane < ld ? LB[lane] : 0.0;
  for (int j = 0; j < n; j++) {
    const int nc = j + ld;
    const double incoming = (active && nc < n) ? w[(size_t)nc * ldw] : 0.0;
    const double lnext = (j + 1 < n && lane < ld) ? LB[(size_t)(j + 1) * ld + lane] : 0.0;
    const double y = ring[slot * 64 + lane] / pg_readlane(lk, 0);
    if (active) w[(size_t)j * ldw] = y;
    const int kmax = min(hw, n - 1 - j);
    // six rows at a time: the loads first, then the updates, then the stores — the ring slots of one column are distinct, which the
    // compiler cannot see through the wrap-around, and one load -> fma -> store at a time is an LDS round trip per row
    for (int k0 = 1; k0 <= kmax; k0 += 6) {
      double v[6];
      int at[6];
#pragma unroll
      for (int u = 0; u < 6; u++) {
        const int k = k0 + u;
        int s2 = slot + (k <= kmax ? k : 0);
        if (s2 >= ld) s2 -= ld;
        at[u] = s2 * 64 + lane;
        v[u] = ring[at[u]];
      }
#pragma unroll
      for (int u = 0; u < 6; u++) v[u] = fma(-pg_readlane(lk, (k0 + u) & 63), y, v[u]);
#pragma unroll
      for (int u = 0; u < 6; u++)
        if (k0 + u <= kmax) ring[at[u]] = v[u];
    }
    ring[slot * 64 + lane] = incoming;
    slot = slot + 1 == ld ? 0 : slot + 1;
    lk = lnext;
  }
  // backward
  slot = (n - 1) % ld;
  lk = lane < ld ? LB[(size_t)(n - 1) * ld + lane] : 0.0;
  double cur = active ? w[(size_t)(n - 1) * ldw] : 0.0;
  for (int j = n - 1; j >= 0; j--) {
    const double below = (active && j > 0) ? w[(size_t)(j - 1) * ldw] : 0.0;
    const double lnext = (j > 0 && lane < ld) ? LB[(size_t)(j - 1) * ld + lane] : 0.0;
    const int kmax = min(hw, n - 1 - j);
    double acc = cur;
    for (int k0 = 1; k0 <= kmax; k0 += 6) {
      double v[6];
#pragma unroll
      for (int u = 0; u < 6; u++) {
        const int k = k0 + u;
        int s2 = slot + (k <= kmax ? k : 0);
        if (s2 >= ld) s2 -= ld;
        v[u] = ring[s2 * 64 + lane];
      }
#pragma unroll
      for (int u = 0; u < 6; u++)
        if (k0 + u <= kmax) acc = fma(-pg_readlane(lk, (k0 + u) & 63), v[u], acc);   // k in order: the sum of the one-row loop
    }
    const double xj = acc / pg_readlane(lk, 0);
    ring[slot * 64 + lane] = xj;
    if (active) w[(size_t)j * ldw] = xj;
    slot = slot == 0 ? ld - 1 : slot - 1;
    lk = lnext;
    cur = below;
  }
}

// ---- the low-rank correction --------------------------------------------------------------------------------------------------------
// thread (i, c), i = 0 .. m - 1, c = 0 .. m: sum over the twelve entries of row i of U times column c of W; c = 0 -> g[i] = (U B^-1 b)[i],
// c >= 1 -> C[i][c - 1] = (I + U B^-1 U^T)[i][c - 1]
__global__ __launch_bounds__(PG_WG) void pg_small_system(const PgEdge* __restrict__ edges, const int* __restrict__ off_edge,
                                                         const double* __restrict__ Jf, const double* __restrict__ Jt,
                                                         const double* __restrict__ W, int ldw, int m, double* __restrict__ C,
                                                         double* __restrict__ g, const PgScalars* __restrict__ sc) {
  if (sc->fail) return;
  const int idx = blockIdx.x * PG_WG + threadIdx.x;
  if (idx >= m * (m + 1)) return;
  const int i = idx / (m + 1), c = idx - i * (m + 1);
  const int r = i / 6, q = i - 6 * r;
  const int k = off_edge[r];
  const double* jf = Jf + 36 * (size_t)k + 6 * q;
  const double* jt = Jt + 36 * (size_t)k + 6 * q;
  const size_t rf = 6 * (size_t)(edges[k].from - 1), rt = 6 * (size_t)(edges[k].to - 1);
  double s = 0.0;
  for (int a = 0; a < 6; a++) s = fma(jf[a], W[(rf + a) * ldw + c], s);
  for (int a = 0; a < 6; a++) s = fma(jt[a], W[(rt + a) * ldw + c], s);
  if (c == 0) g[i] = s;
  else C[(size_t)i * m + (c - 1)] = s + (i == c - 1 ? 1.0 : 0.0);
}

// one workgroup: C = L L^T in place (lower), then g <- C^-1 g.  Every element has one writer per step; steps are separated by barriers.
__global__ __launch_bounds__(PG_WG) void pg_dense_solve(double* __restrict__ C, double* __restrict__ g, int m, PgScalars* __restrict__ sc) {
  __shared__ double s_piv;
  if (sc->fail) return;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int j = 0; j < m; j++) {
    if (tid == 0) s_piv = C[(size_t)j * m + j];
    __syncthreads();
    const double piv = s_piv;
    if (!(piv > 0.0) || !(piv <= DBL_MAX)) {
      if (tid == 0) sc->fail = 2;
      return;
    }
    const double l = sqrt(piv);
    if (tid == 0) C[(size_t)j * m + j] = l;
    for (int i = j + 1 + tid; i < m; i += PG_WG) C[(size_t)i * m + j] = C[(size_t)i * m + j] / l;
    __syncthreads();
    for (int k = j + 1 + ty; k < m; k += 16) {
      const double lkj = C[(size_t)k * m + j];
      for (int i = k + tx; i < m; i += 16) C[(size_t)i * m + k] = fma(-C[(size_t)i * m + j], lkj, C[(size_t)i * m + k]);
    }
    __syncthreads();
  }
  for (int j = 0; j < m; j++) {
    if (tid == 0) g[j] = g[j] / C[(size_t)j * m + j];
    __syncthreads();
    const double gj = g[j];
    for (int i = j + 1 + tid; i < m; i += PG_WG) g[i] = fma(-C[(size_t)i * m + j], gj, g[i]);
    __syncthreads();
  }
  for (int j = m - 1; j >= 0; j--) {
    if (tid == 0) g[j] = g[j] / C[(size_t)j * m + j];
    __syncthreads();
    const double gj = g[j];
    for (int i = tid; i < j; i += PG_WG) g[i] = fma(-C[(size_t)j * m + i], gj, g[i]);
    __syncthreads();
  }
}

// x[row] = W[row][0] - sum_c W[row][1 + c] z[c], c in order
__global__ __launch_bounds__(PG_WG) void pg_combine(const double* __restrict__ W, int ldw, int m, const double* __restrict__ z, int n,
                                                    double* __restrict__ x, const PgScalars* __restrict__ sc) {
  if (sc->fail) return;
  const int row = blockIdx.x * PG_WG + threadIdx.x;
  if (row >= n) return;
  const double* w = W + (size_t)row * ldw;
  double s = w[0];
  for (int c = 0; c < m; c++) s = fma(-w[1 + c], z[c], s);
  x[row] = s;
}

// X'[v] = X[v] (+) x[6(v-1) ..]; the fixed vertex is copied
__global__ __launch_bounds__(PG_WG) void pg_update(const PgPose* __restrict__ X, const double* __restrict__ x, int n_vertices,
                                                   PgPose* __restrict__ Xt, const PgScalars* __restrict__ sc) {
  if (sc->fail) return;
  const int v = blockIdx.x * PG_WG + threadIdx.x;
  if (v >= n_vertices) return;
  if (v == 0) { Xt[0] = X[0]; return; }
  double d6[6];
  for (int a = 0; a < 6; a++) d6[a] = x[6 * (size_t)(v - 1) + a];
  PgPose out;
  pg_oplus(X[v], d6, &out);
  Xt[v] = out;
}

inline int blocks(size_t n, int wg = PG_WG) { return (int)((n + wg - 1) / wg); }

// the four events that bracket the three profiled stages of a trial (LSR_PROFILE)
struct StageEvents {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int create() {
    for (auto& e : ev) LSR_HIP(hipEventCreate(&e));
    return LSR_OK;
  }
  ~StageEvents() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

int pose_graph_adjacent_edges(const double* poses16, int n, int num_adjacent, lsr_pose_edge* out, size_t capacity, size_t* n_out) {
  const int k = num_adjacent;
  const size_t total = n > k + 1 ? (size_t)(n - k - 1) * (size_t)k : 0;
  if (total > capacity || (total > 0 && !out)) {
    *n_out = total;
    set_last_error("pose graph: edge capacity too small");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  size_t at = 0;
  for (int i = 0; i < n; i++) {
    if (!(i > k)) continue;
    PgPose Xi;
    pg_pose_from_col16(poses16 + 16 * (size_t)i, &Xi);
    for (int j = 0; j < k; j++) {
      const int from = i - k + j;
      PgPose Xf, Xfi, Z;
      pg_pose_from_col16(poses16 + 16 * (size_t)from, &Xf);
      pg_inverse(Xf, &Xfi);
      pg_compose(Xfi, Xi, &Z);
      out[at].from = from;
      out[at].to = i;
      pg_pose_to_col16(Z, out[at].measurement);
      at++;
    }
  }
  *n_out = total;
  return LSR_OK;
}

int pose_graph_optimize(PgWorkspace& ws, const double* poses16_in, int n_vertices, const lsr_pose_edge* edges, int n_edges, int max_iterations,
                        int band, int max_offband, double* poses16_out, lsr_pose_graph_result* result, lsr_pose_graph_trace* trace,
                        hipStream_t stream, hipEvent_t ev0, hipEvent_t ev1) {
  const int N = n_vertices, E = n_edges;
  const int n = 6 * (N - 1), hw = 6 * band + 5, ld = hw + 1;

  // host side of the graph: edges as the kernels read them, the slots of U, the CSR list of every vertex's edges in edge order
  std::vector<PgEdge> he((size_t)E);
  std::vector<int> off_edge, inc_start((size_t)N + 1, 0), inc_edge((size_t)2 * E);
  for (int k = 0; k < E; k++) {
    PgEdge& D = he[(size_t)k];
    D.from = edges[k].from; D.to = edges[k].to; D.pad = 0;
    const int gap = D.from > D.to ? D.from - D.to : D.to - D.from;
    const bool in_band = D.from == 0 || D.to == 0 || gap <= band;
    D.slot = in_band ? -1 : (int)off_edge.size();
    if (!in_band) off_edge.push_back(k);
    PgPose Z;
    pg_pose_from_col16(edges[k].measurement, &Z);
    pg_inverse(Z, &D.Zinv);
    inc_start[(size_t)D.from + 1]++;
    inc_start[(size_t)D.to + 1]++;
  }
  for (int v = 0; v < N; v++) inc_start[(size_t)v + 1] += inc_start[(size_t)v];
  {
    std::vector<int> fill(inc_start.begin(), inc_start.end() - 1);
    for (int k = 0; k < E; k++) { inc_edge[(size_t)fill[(size_t)he[(size_t)k].from]++] = k; inc_edge[(size_t)fill[(size_t)he[(size_t)k].to]++] = k; }
  }
  const int L = (int)off_edge.size(), m = 6 * L, ldw = 1 + m;
  if (L > max_offband) { set_last_error("pose graph: more off-band edges than the entry point's limit"); return LSR_ERR_INVALID_ARGUMENT; }
  const bool blocked = L > PG_MAX_OFFBAND;   // the dense part by tiles over many workgroups (pose_graph_dense.hip)

  int st;
  if ((st = ws.X.reserve(N)) || (st = ws.Xt.reserve(N)) || (st = ws.edges.reserve(E)) || (st = ws.inc_start.reserve((size_t)N + 1)) ||
      (st = ws.inc_edge.reserve((size_t)2 * E)) || (st = ws.off_edge.reserve(std::max(L, 1))) || (st = ws.e.reserve(6 * (size_t)E)) ||
      (st = ws.Jf.reserve(36 * (size_t)E)) || (st = ws.Jt.reserve(36 * (size_t)E)) || (st = ws.ete.reserve(E)) ||
      (st = ws.AB.reserve((size_t)n * ld)) || (st = ws.LB.reserve((size_t)n * ld)) || (st = ws.b.reserve(n)) || (st = ws.diag.reserve(n)) ||
      (st = ws.x.reserve(n)) || (st = ws.W.reserve((size_t)n * ldw)) || (st = ws.C.reserve(std::max((size_t)m * m, (size_t)1))) ||
      (st = ws.g.reserve(std::max(m, 1))) || (blocked && (st = ws.z.reserve(m))) || (st = ws.d_sc.reserve(1)) || (st = ws.h_sc.reserve(1)) ||
      (st = ws.h_out.reserve(12 * (size_t)N)))
    return st;
  // uploads through one pinned staging buffer: poses | edges | inc_start | inc_edge | off_edge
  const size_t b_pose = sizeof(PgPose) * (size_t)N, b_edge = sizeof(PgEdge) * (size_t)E, b_is = sizeof(int) * ((size_t)N + 1),
               b_ie = sizeof(int) * (size_t)2 * E, b_off = sizeof(int) * (size_t)L;
  if ((st = ws.h_up.reserve(b_pose + b_edge + b_is + b_ie + b_off + 64))) return st;
  unsigned char* up = ws.h_up.p;
  {
    PgPose* hp = reinterpret_cast<PgPose*>(up);
    for (int v = 0; v < N; v++) pg_pose_from_col16(poses16_in + 16 * (size_t)v, hp + v);
    std::memcpy(up + b_pose, he.data(), b_edge);
    std::memcpy(up + b_pose + b_edge, inc_start.data(), b_is);
    std::memcpy(up + b_pose + b_edge + b_is, inc_edge.data(), b_ie);
    if (L) std::memcpy(up + b_pose + b_edge + b_is + b_ie, off_edge.data(), b_off);
  }
  LSR_HIP(hipEventRecord(ev0, stream));
  LSR_HIP(hipMemcpyAsync(ws.X.p, up, b_pose, hipMemcpyHostToDevice, stream));
  LSR_HIP(hipMemcpyAsync(ws.edges.p, up + b_pose, b_edge, hipMemcpyHostToDevice, stream));
  LSR_HIP(hipMemcpyAsync(ws.inc_start.p, up + b_pose + b_edge, b_is, hipMemcpyHostToDevice, stream));
  LSR_HIP(hipMemcpyAsync(ws.inc_edge.p, up + b_pose + b_edge + b_is, b_ie, hipMemcpyHostToDevice, stream));
  if (L) LSR_HIP(hipMemcpyAsync(ws.off_edge.p, up + b_pose + b_edge + b_is + b_ie, b_off, hipMemcpyHostToDevice, stream));

  PgPose *X = ws.X.p, *Xt = ws.Xt.p;
  PgScalars* sc = ws.d_sc.p;
  auto read_scalars = [&]() -> int {
    LSR_HIP(hipMemcpyAsync(ws.h_sc.p, sc, sizeof(PgScalars), hipMemcpyDeviceToHost, stream));
    LSR_HIP(hipStreamSynchronize(stream));
    return LSR_OK;
  };
  const size_t factor_lds = sizeof(double) * (size_t)ld * ld, solve_lds = sizeof(double) * (size_t)ld * 64;
  // LSR_PROFILE: three stages of every trial between events, read after the trial's own synchronisation
  StageEvents sev;
  const bool staged = ws.profile;
  ws.stage_ms[0] = ws.stage_ms[1] = ws.stage_ms[2] = 0.0;
  if (staged && (st = sev.create())) return st;
  auto mark = [&](int i) -> int {
    if (staged) LSR_HIP(hipEventRecord(sev.ev[i], stream));
    return LSR_OK;
  };

  lsr_pose_graph_result R;
  std::memset(&R, 0, sizeof(R));
  R.stop_reason = LSR_POSE_GRAPH_STOP_MAX_ITERATIONS;
  std::vector<lsr_pose_graph_trace> tr;
  double lambda = 0.0, nu = 2.0, cur = 0.0;
  for (int it = 0; it < max_iterations; it++) {
    hipLaunchKernelGGL(pg_linearize, dim3(blocks(E)), dim3(PG_WG), 0, stream, X, ws.edges.p, E, ws.e.p, ws.Jf.p, ws.Jt.p, ws.ete.p);
    hipLaunchKernelGGL(pg_gather, dim3(blocks((size_t)(N - 1) * (band + 1))), dim3(PG_WG), 0, stream, ws.edges.p, ws.inc_start.p,
                       ws.inc_edge.p, ws.e.p, ws.Jf.p, ws.Jt.p, N, band, ws.AB.p, ws.b.p, ws.diag.p);
    hipLaunchKernelGGL(pg_reduce_linearized, dim3(1), dim3(PG_WG), 0, stream, ws.ete.p, E, ws.diag.p, n, sc);
    LSR_HIP(hipGetLastError());
    if ((st = read_scalars())) return st;
    cur = ws.h_sc.p->chi2;
    if (it == 0) {
      R.chi2_before = cur;
      lambda = 1e-5 * ws.h_sc.p->max_diag;
      nu = 2.0;
    }
    int q = 0;
    double rho = 0.0;
    do {
      hipLaunchKernelGGL(pg_band_factor, dim3(1), dim3(PG_WG), factor_lds, stream, ws.AB.p, lambda, n, hw, ws.LB.p, sc);
      if ((st = mark(0))) return st;
      hipLaunchKernelGGL(pg_fill_rhs, dim3(blocks((size_t)n * ldw)), dim3(PG_WG), 0, stream, ws.edges.p, ws.off_edge.p, ws.Jf.p, ws.Jt.p,
                         ws.b.p, n, ldw, ws.W.p);
      hipLaunchKernelGGL(pg_band_solve, dim3(blocks(ldw, 64)), dim3(64), solve_lds, stream, ws.LB.p, n, hw, ws.W.p, ldw, ldw, sc);
      if ((st = mark(1))) return st;
      if (m > 0) {
        hipLaunchKernelGGL(pg_small_system, dim3(blocks((size_t)m * (m + 1))), dim3(PG_WG), 0, stream, ws.edges.p, ws.off_edge.p, ws.Jf.p,
                           ws.Jt.p, ws.W.p, ldw, m, ws.C.p, ws.g.p, sc);
        if (blocked) pose_graph_dense_solve(ws.C.p, ws.g.p, ws.z.p, m, sc, stream);
        else hipLaunchKernelGGL(pg_dense_solve, dim3(1), dim3(PG_WG), 0, stream, ws.C.p, ws.g.p, m, sc);
      }
      if ((st = mark(2))) return st;
      if (blocked) pose_graph_combine_rows(ws.W.p, ldw, m, ws.z.p, n, ws.x.p, sc, stream);
      else hipLaunchKernelGGL(pg_combine, dim3(blocks(n)), dim3(PG_WG), 0, stream, ws.W.p, ldw, m, ws.g.p, n, ws.x.p, sc);
      if ((st = mark(3))) return st;
      hipLaunchKernelGGL(pg_update, dim3(blocks(N)), dim3(PG_WG), 0, stream, X, ws.x.p, N, Xt, sc);
      hipLaunchKernelGGL(pg_error, dim3(blocks(E)), dim3(PG_WG), 0, stream, Xt, ws.edges.p, E, ws.ete.p);
      hipLaunchKernelGGL(pg_reduce_trial, dim3(1), dim3(PG_WG), 0, stream, ws.ete.p, E, ws.x.p, ws.b.p, n, lambda, sc);
      LSR_HIP(hipGetLastError());
      if ((st = read_scalars())) return st;
      if (staged)
        for (int i = 0; i < 3; i++) {
          float part = 0.f;
          LSR_HIP(hipEventElapsedTime(&part, sev.ev[i], sev.ev[i + 1]));
          ws.stage_ms[i] += part;
        }
      // a failed factorisation counts as a trial whose chi2 is the largest double and whose step is zero (g2o: tmp = max)
      const bool failed = ws.h_sc.p->fail != 0;
      const double tmp = failed ? DBL_MAX : ws.h_sc.p->trial_chi2;
      const double scale = (failed ? 0.0 : ws.h_sc.p->scale) + 1e-3;
      rho = (cur - tmp) / scale;
      if (rho > 0.0 && std::isfinite(tmp)) {
        const double a = 1.0 - std::pow(2.0 * rho - 1.0, 3);
        lambda *= std::max(1.0 / 3.0, std::min(a, 2.0 / 3.0));
        nu = 2.0;
        cur = tmp;
        std::swap(X, Xt);
      } else {
        lambda *= nu;
        nu *= 2.0;
      }
      q++;
    } while (rho < 0.0 && q < PG_MAX_TRIALS);
    lsr_pose_graph_trace T;
    std::memset(&T, 0, sizeof(T));
    T.trials = q; T.chi2 = cur; T.lambda = lambda; T.rho = rho;
    tr.push_back(T);
    R.iterations++;
    R.trials += q;
    if (q == PG_MAX_TRIALS || rho == 0.0 || !std::isfinite(lambda)) {
      R.stop_reason = q == PG_MAX_TRIALS ? LSR_POSE_GRAPH_STOP_TRIALS : (rho == 0.0 ? LSR_POSE_GRAPH_STOP_RHO_ZERO : LSR_POSE_GRAPH_STOP_LAMBDA);
      break;
    }
  }
  LSR_HIP(hipMemcpyAsync(ws.h_out.p, X, sizeof(PgPose) * (size_t)N, hipMemcpyDeviceToHost, stream));
  LSR_HIP(hipEventRecord(ev1, stream));
  LSR_HIP(hipStreamSynchronize(stream));
  float ms = 0.f;
  LSR_HIP(hipEventElapsedTime(&ms, ev0, ev1));
  R.chi2_after = cur;
  R.lambda = lambda;
  R.device_ms = ms;
  // outputs last: nothing is written on an error above
  const PgPose* hx = reinterpret_cast<const PgPose*>(ws.h_out.p);
  for (int v = 0; v < N; v++) pg_pose_to_col16(hx[v], poses16_out + 16 * (size_t)v);
  *result = R;
  if (trace) std::memcpy(trace, tr.data(), sizeof(lsr_pose_graph_trace) * tr.size());
  return LSR_OK;
}

}  // namespace lsr

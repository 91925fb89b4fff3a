// Pose-graph optimisation past 64 edges outside the band (lsr_optimize_pose_graph_long): the dense part of the Woodbury split of
// csrc/pose_graph.hip as a blocked fp64 Cholesky over many workgroups.  C = I + U B^-1 U^T is m x m, m = 6L up to 6144, row-major, lower
// triangle; it is worked on in 64 x 64 tiles staged in LDS, right-looking, three launches per block column k:
//   pgd_potrf   one workgroup: the diagonal tile C_kk = L_kk L_kk^T in LDS
//   pgd_trsm    one wave per tile below it: C_ik <- C_ik L_kk^-T, the tile in LDS, a row per lane (forward substitution)
//   pgd_update  one workgroup per tile of the trailing lower triangle: C_ij <- C_ij - L_ik L_jk^T, 4 x 4 results per thread
// g = U B^-1 b rides along as one more row of the matrix: pgd_trsm's last workgroup solves its block (L y = g), pgd_update's last row of
// workgroups subtracts L_jk y_k from the blocks below.  L^T z = y is one launch per block column, last to first (pgd_back): every
// workgroup solves the 64 x 64 triangle itself, one writes z_k, the others take L_ki^T z_k off the blocks above.
// pgd_combine is pg_combine with a wave per row of W: lanes stride the row (coalesced), then a fixed tree over the lanes.
// m need not be a multiple of 64: the loads return the identity outside m x m (pgd_load) and the stores are bounded, so the last
// block column factors a tile whose tail is the identity.
// Determinism: every element has one writer per launch and a fixed summation order; no atomics.
// Hang safety (the rule of pose_graph.hip): every loop runs to the tile edge or to a count known at launch; no workgroup waits for
// another; a pivot that is not positive and finite sets PgScalars::fail = 2 and the kernel returns; the kernels behind it return at once.
#include <cfloat>
#include <cmath>

#include "pose_graph.hpp"

namespace lsr {
namespace {

constexpr int PGD_T = 64;           // tile edge: one lane per row or column of a tile
constexpr int PGD_LD = PGD_T + 1;   // LDS row stride of a tile read down a column by the lanes
constexpr int PGD_KC = 32;          // pgd_update stages its operands in two halves of 32 columns
constexpr int PGD_KLD = PGD_T + 2;  // ... column-major, this stride (even: the four values a thread reads stay 16-byte aligned)

__device__ inline double pgd_readlane(double v, int lane) {
  const long long bits = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(bits & 0xffffffffLL), lane);
  const int hi = __builtin_amdgcn_readlane((int)(bits >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// C padded to a multiple of the tile edge: the identity outside m x m
__device__ inline double pgd_load(const double* __restrict__ C, int m, int i, int j) {
  return (i < m && j < m) ? C[(size_t)i * m + j] : (i == j ? 1.0 : 0.0);
}

// one workgroup: the diagonal tile of block column k, factored in LDS (lane -> row, wave -> column of the rank-1 update)
__global__ __launch_bounds__(256) void pgd_potrf(double* __restrict__ C, int m, int k, PgScalars* __restrict__ sc) {
  __shared__ double S[PGD_T * PGD_LD];
  if (sc->fail) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k0 = k * PGD_T;
  for (int r = wave; r < PGD_T; r += 4) S[r * PGD_LD + lane] = pgd_load(C, m, k0 + r, k0 + lane);
  __syncthreads();
  for (int j = 0; j < PGD_T; j++) {
    const double piv = S[j * PGD_LD + j];
    if (!(piv > 0.0) || !(piv <= DBL_MAX)) {   // the same LDS word for every thread: a uniform exit
      if (tid == 0) sc->fail = 2;
      return;
    }
    const double l = sqrt(piv);
    const double mine = tid == j ? l : ((tid > j && tid < PGD_T) ? S[tid * PGD_LD + j] / l : 0.0);
    __syncthreads();
    if (tid >= j && tid < PGD_T) S[tid * PGD_LD + j] = mine;
    __syncthreads();
    if (lane > j) {
      const double lr = S[lane * PGD_LD + j];
      for (int c = j + 1 + wave; c <= lane; c += 4) S[lane * PGD_LD + c] = fma(-lr, S[c * PGD_LD + j], S[lane * PGD_LD + c]);
    }
    __syncthreads();
  }
  for (int r = wave; r < PGD_T; r += 4)
    if (lane <= r && k0 + r < m) C[(size_t)(k0 + r) * m + k0 + lane] = S[r * PGD_LD + lane];
}

// workgroup b < t (t = nb - 1 - k tiles below the diagonal one): tile (k + 1 + b, k), x L_kk^T = a by forward substitution, the tile in LDS
// and a row per lane: x[c] = (a[c] - sum_{j < c} x[j] L[c][j]) / L[c][c], the sum as four interleaved partial sums (j mod 4) joined as
// (s0 + s1) + (s2 + s3) — a quarter of the dependent chain.  Workgroup t: block k of g as row 0 of a tile of zeros.
__global__ __launch_bounds__(64) void pgd_trsm(double* __restrict__ C, double* __restrict__ g, int m, int k, int nb,
                                               const PgScalars* __restrict__ sc) {
  __shared__ double Ls[PGD_T * (PGD_T + 1) / 2];   // the lower triangle packed by rows: read at one address by all lanes
  __shared__ double As[PGD_T * PGD_LD];
  if (sc->fail) return;
  const int lane = threadIdx.x, k0 = k * PGD_T;
  const bool is_g = (int)blockIdx.x == nb - 1 - k;
  const int i0 = (k + 1 + (int)blockIdx.x) * PGD_T;
  const bool col_ok = k0 + lane < m;
  for (int r = 0; r < PGD_T; r++) {
    if (lane <= r) Ls[r * (r + 1) / 2 + lane] = pgd_load(C, m, k0 + r, k0 + lane);
    double a = 0.0;
    if (is_g) {
      if (r == 0 && col_ok) a = g[k0 + lane];
    } else if (i0 + r < m && col_ok) {
      a = C[(size_t)(i0 + r) * m + k0 + lane];
    }
    As[r * PGD_LD + lane] = a;
  }
  __syncthreads();
  double* mine = As + lane * PGD_LD;
  for (int c = 0; c < PGD_T; c++) {
    const double* lc = Ls + c * (c + 1) / 2;
    double s0 = mine[c], s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int j = 0;
    for (; j + 3 < c; j += 4) {
      s0 = fma(-mine[j], lc[j], s0);
      s1 = fma(-mine[j + 1], lc[j + 1], s1);
      s2 = fma(-mine[j + 2], lc[j + 2], s2);
      s3 = fma(-mine[j + 3], lc[j + 3], s3);
    }
    for (; j < c; j++) s0 = fma(-mine[j], lc[j], s0);
    mine[c] = ((s0 + s1) + (s2 + s3)) / lc[c];
  }
  __syncthreads();
  for (int r = 0; r < PGD_T; r++) {
    if (is_g) {
      if (r == 0 && col_ok) g[k0 + lane] = As[lane];
    } else if (i0 + r < m && col_ok) {
      C[(size_t)(i0 + r) * m + k0 + lane] = As[r * PGD_LD + lane];
    }
  }
}

// grid (t, t + 1), t = nb - 1 - k >= 1 (so block column k is whole).  Row y < t: tile (k + 1 + y, k + 1 + x) for x <= y, the sum over
// the 64 columns of block k in order, then one subtraction (the workgroups with x > y return at once).  Row t: block k + 1 + x of g,
// g_j <- g_j - L_jk y_k, a row per thread.
__global__ __launch_bounds__(256) void pgd_update(double* __restrict__ C, double* __restrict__ g, int m, int k, int nb,
                                                  const PgScalars* __restrict__ sc) {
  __shared__ double As[PGD_KC * PGD_KLD], Bs[PGD_KC * PGD_KLD];
  if (sc->fail) return;
  const int t = nb - 1 - k, bx = blockIdx.x, by = blockIdx.y, tid = threadIdx.x, k0 = k * PGD_T;
  if (by == t) {
    const int j = (k + 1 + bx) * PGD_T + tid;
    if (tid < PGD_T && j < m) {
      const double* l = C + (size_t)j * m + k0;
      double s = g[j];
      for (int c = 0; c < PGD_T; c++) s = fma(-l[c], g[k0 + c], s);
      g[j] = s;
    }
    return;
  }
  if (bx > by) return;
  const int i0 = (k + 1 + by) * PGD_T, j0 = (k + 1 + bx) * PGD_T;
  const int tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) acc[u][v] = 0.0;
  for (int h = 0; h < PGD_T / PGD_KC; h++) {
    __syncthreads();
    for (int e = tid; e < PGD_T * PGD_KC; e += 256) {
      const int r = e / PGD_KC, kk = e - r * PGD_KC;
      const int col = k0 + h * PGD_KC + kk;
      As[kk * PGD_KLD + r] = i0 + r < m ? C[(size_t)(i0 + r) * m + col] : 0.0;
      Bs[kk * PGD_KLD + r] = j0 + r < m ? C[(size_t)(j0 + r) * m + col] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int kk = 0; kk < PGD_KC; kk++) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { a[u] = As[kk * PGD_KLD + 4 * ty + u]; b[u] = Bs[kk * PGD_KLD + 4 * tx + u]; }
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int v = 0; v < 4; v++) acc[u][v] = fma(a[u], b[v], acc[u][v]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const int i = i0 + 4 * ty + u, j = j0 + 4 * tx + v;
      if (i < m && j < m) C[(size_t)i * m + j] = C[(size_t)i * m + j] - acc[u][v];
    }
}

// L^T z = y, block column k, grid k + 1: every workgroup solves L_kk^T z_k = y_k (lane -> column, right-looking, the solved entry
// handed round by readlane); workgroup k writes z_k, workgroup i < k takes L_ki^T z_k off block i of y
__global__ __launch_bounds__(64) void pgd_back(const double* __restrict__ C, double* __restrict__ g, double* __restrict__ z, int m, int k,
                                               const PgScalars* __restrict__ sc) {
  __shared__ double Ls[PGD_T * PGD_LD];
  if (sc->fail) return;
  const int lane = threadIdx.x, k0 = k * PGD_T;
  for (int r = 0; r < PGD_T; r++) Ls[r * PGD_LD + lane] = lane <= r ? pgd_load(C, m, k0 + r, k0 + lane) : 0.0;
  __syncthreads();
  double v = k0 + lane < m ? g[k0 + lane] : 0.0, zv = 0.0;
  for (int j = PGD_T - 1; j >= 0; j--) {
    const double zj = pgd_readlane(v, j) / Ls[j * PGD_LD + j];
    if (lane == j) zv = zj;
    if (lane < j) v = fma(-Ls[j * PGD_LD + lane], zj, v);
  }
  const int i = blockIdx.x;
  if (i == k) {
    if (k0 + lane < m) z[k0 + lane] = zv;
    return;
  }
  const int i0 = i * PGD_T;   // i < k: a whole block
  double s = g[i0 + lane];
  for (int r = 0; r < PGD_T; r++) {
    const double zr = pgd_readlane(zv, r);
    if (k0 + r < m) s = fma(-C[(size_t)(k0 + r) * m + i0 + lane], zr, s);
  }
  g[i0 + lane] = s;
}

// x[row] = W[row][0] - sum_c W[row][1 + c] z[c]: a wave per row, lane l sums c = l, l + 64, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void pgd_combine(const double* __restrict__ W, int ldw, int m, const double* __restrict__ z, int n,
                                                   double* __restrict__ x, const PgScalars* __restrict__ sc) {
  if (sc->fail) return;
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;   // a whole wave
  const double* w = W + (size_t)row * ldw;
  double s = 0.0;
  for (int c = lane; c < m; c += 64) s = fma(w[1 + c], z[c], s);
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_down(s, o, 64);
  if (lane == 0) x[row] = w[0] - s;
}

}  // namespace

void pose_graph_dense_solve(double* C, double* g, double* z, int m, PgScalars* sc, hipStream_t stream) {
  const int nb = (m + PGD_T - 1) / PGD_T;
  for (int k = 0; k < nb; k++) {
    const int t = nb - 1 - k;
    hipLaunchKernelGGL(pgd_potrf, dim3(1), dim3(256), 0, stream, C, m, k, sc);
    hipLaunchKernelGGL(pgd_trsm, dim3(t + 1), dim3(64), 0, stream, C, g, m, k, nb, sc);
    if (t > 0) hipLaunchKernelGGL(pgd_update, dim3(t, t + 1), dim3(256), 0, stream, C, g, m, k, nb, sc);
  }
  for (int k = nb - 1; k >= 0; k--) hipLaunchKernelGGL(pgd_back, dim3(k + 1), dim3(64), 0, stream, C, g, z, m, k, sc);
}

void pose_graph_combine_rows(const double* W, int ldw, int m, const double* z, int n, double* x, const PgScalars* sc, hipStream_t stream) {
  hipLaunchKernelGGL(pgd_combine, dim3((n + 3) / 4), dim3(256), 0, stream, W, ldw, m, z, n, x, sc);
}

}  // namespace lsr

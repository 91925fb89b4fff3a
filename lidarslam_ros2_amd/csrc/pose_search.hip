// NDT pose search: where is the scan, when no guess inside NDT's basin of convergence exists?  The NDT score of the source at every
// pose of a candidate list in ONE launch (lsr_ndt_score_poses), the pose lattice and the greedy choice of the distinct best on the
// host (lsr_pose_lattice_poses, lsr_select_poses), and the whole procedure — lattice, scores, choice, refinement of the kept
// candidates as one candidate set through align_ndt_batch, winner by trans_probability — as lsr_ndt_search_pose.
// No reference site exists (the reference's answer is a person clicking `initial_pose` in rviz): the definitions are this project's,
// stated in include/lidarslam_reg.h.  The score of a pose is DEFINED as what a derivative pass at that pose returns
// (lsr_ndt_derivatives_pairs with T16 = the pose), bit for bit: the per-pair arithmetic is ndt_point.hpp's, the sum is the canonical
// one (ndt_canon.hpp), so nothing here can drift from the registration that refines the candidates.
#include <algorithm>
#include <cmath>
#include <numeric>

#include "api_internal.hpp"
#include "ndt_canon.hpp"
#include "ndt_point.hpp"

using namespace lsr;

namespace lsr {
namespace {

// Score and pair count of ONE point at one pose: the point's neighbours dealt to four partial sums (partial q takes neighbours
// q, q + 4, q + 8, ...), added as (p0 + p1) + (p2 + p3) — the lane kernel's loop (ndt.hip) without the A / E sums, which the compiler
// drops from pair_terms as dead code.  T: row-major 3x4, wave-uniform.  (A function of its own and not the lane kernel's loop made
// callable: that loop also carries the KDTREE and two-waves-per-chunk forms and the 11 sums of a point, and its register allocation
// is what the derivative pass's time hangs on; what the two must agree on — offsets, table layout, pair arithmetic, deal order — is
// in the shared headers or asserted bit for bit by tests/test_pose_search_gpu.py.)
template <int NOFF, int TAB>
__device__ __forceinline__ void score_point(const NdtProblem& P, const uint4* s_table, const bool have, const float px, const float py,
                                            const float pz, const float* T, const float d2, const double d1d, float& score_out,
                                            float& pairs_out) {
  constexpr int NT = (NOFF + 3) / 4;   // neighbours per partial sum
  constexpr int GROUP = 4;             // records fetched per gather round trip
  const float tx = xform_ref(T[0], T[1], T[2], T[3], px, py, pz);
  const float ty = xform_ref(T[4], T[5], T[6], T[7], px, py, pz);
  const float tz = xform_ref(T[8], T[9], T[10], T[11], px, py, pz);
  const float leaf = P.leaf;
  const float fx = floorf(tx / leaf), fy = floorf(ty / leaf), fz = floorf(tz / leaf);
  const bool finite_ok = have && (fabsf(fx) < 1.0e9f) && (fabsf(fy) < 1.0e9f) && (fabsf(fz) < 1.0e9f);
  const int ci = finite_ok ? (int)fx : INT_MIN / 2, cj = finite_ok ? (int)fy : INT_MIN / 2, ck = finite_ok ? (int)fz : INT_MIN / 2;
  const int mb0 = P.min_b[0], mb1 = P.min_b[1], mb2 = P.min_b[2];
  const int xb0 = P.max_b[0], xb1 = P.max_b[1], xb2 = P.max_b[2];
  const int mul1 = P.mul1, mul2 = P.mul2;
  // a cell outside the grid's bounding box has no leaf: per-axis tests of the centre cell and its two neighbours
  bool inx[3], iny[3], inz[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    inx[d] = (ci + d - 1 >= mb0) & (ci + d - 1 <= xb0);
    iny[d] = (cj + d - 1 >= mb1) & (cj + d - 1 <= xb1);
    inz[d] = (ck + d - 1 >= mb2) & (ck + d - 1 <= xb2);
  }
  const int centre = (ci - mb0) + (cj - mb1) * mul1 + (ck - mb2) * mul2;
  bool nb_ok[NOFF];
  int nb_rec[NOFF];   // LDS table: byte offset of the record inside the table image; global tables: record index
#pragma unroll
  for (int o = 0; o < NOFF; o++) {
    int dx, dy, dz;
    Offsets<NOFF>::get(o, dx, dy, dz);
    const bool in = inx[dx + 1] & iny[dy + 1] & inz[dz + 1];
    nb_ok[o] = in;
    nb_rec[o] = in ? centre + dx + dy * mul1 + dz * mul2 : 0;
  }
  const GlbV4* g_rec = (const GlbV4*)P.rec;
  const GlbInt* g_cell_slot = (const GlbInt*)P.cell_slot;
  (void)g_rec; (void)g_cell_slot;
  if (TAB == NDT_TAB_LDS) {
    const __attribute__((address_space(3))) unsigned short* s_map = (const __attribute__((address_space(3))) unsigned short*)s_table;
    const int map_bytes = P.lds_map_bytes;
    int sl[NOFF];
#pragma unroll
    for (int o = 0; o < NOFF; o++) sl[o] = (int)s_map[nb_rec[o]];
#pragma unroll
    for (int o = 0; o < NOFF; o++) {
      nb_ok[o] = nb_ok[o] & (sl[o] != 0xFFFF);    // the LDS table only holds usable leaves
      nb_rec[o] = map_bytes + (nb_ok[o] ? sl[o] : 0) * NDT_LDS_REC_BYTES;
    }
  } else if (TAB == NDT_TAB_COMPACT) {
    int sl[NOFF];
#pragma unroll
    for (int o = 0; o < NOFF; o++) sl[o] = g_cell_slot[nb_rec[o]];
#pragma unroll
    for (int o = 0; o < NOFF; o++) {
      nb_ok[o] = nb_ok[o] & (sl[o] >= 0);
      nb_rec[o] = sl[o] >= 0 ? sl[o] : 0;
    }
  }
  // a neighbour no lane of the wave can use is skipped by the whole wave (a pair that is not ok leaves every sum as it was)
  bool nb_any[NOFF];
#pragma unroll
  for (int o = 0; o < NOFF; o++) nb_any[o] = __builtin_amdgcn_ballot_w64(nb_ok[o]) != 0ull;

  float S0 = 0.f, S1 = 0.f;
#pragma unroll
  for (int half = 0; half < 2; half++) {
    float Pq[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int e0 = 0; e0 < 2 * NT; e0 += GROUP) {
      v4f r0[GROUP], r1[GROUP], r2[GROUP];
#pragma unroll
      for (int u = 0; u < GROUP; u++) {
        const int e = e0 + u, ql = e / NT, t = e % NT, o = 2 * half + ql + 4 * t;
        if (e < 2 * NT && o < NOFF) {
          if (TAB == NDT_TAB_LDS) {
            const LdsV4* rp = (const LdsV4*)((const __attribute__((address_space(3))) unsigned char*)s_table + nb_rec[o]);
            r0[u] = rp[0]; r1[u] = rp[1]; r2[u] = rp[2];
          } else {
            const GlbV4* rp = g_rec + (size_t)nb_rec[o] * 4;   // empty / unusable cells hold NaN records
            r0[u] = rp[0]; r1[u] = rp[1]; r2[u] = rp[2];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < GROUP; u++) {
        const int e = e0 + u, ql = e / NT, t = e % NT, o = 2 * half + ql + 4 * t;
        if (e < 2 * NT && o < NOFF && nb_any[o]) {
          float A0 = 0.f, A1 = 0.f, A2 = 0.f, E00 = 0.f, E01 = 0.f, E02 = 0.f, E11 = 0.f, E12 = 0.f, E22 = 0.f;   // unused sums
          pair_terms(nb_ok[o], false, tx, ty, tz, make_float4(r0[u].x, r0[u].y, r0[u].z, r0[u].w), make_float4(r1[u].x, r1[u].y, r1[u].z, r1[u].w),
                     make_float4(r2[u].x, r2[u].y, r2[u].z, r2[u].w), d2, d1d, Pq[ql][0], Pq[ql][1], A0, A1, A2, E00, E01, E02, E11, E12, E22);
        }
      }
    }
    if (half == 0) {
      S0 = Pq[0][0] + Pq[1][0];
      S1 = Pq[0][1] + Pq[1][1];
    } else {
      S0 = S0 + (Pq[0][0] + Pq[1][0]);
      S1 = S1 + (Pq[0][1] + Pq[1][1]);
    }
  }
  score_out = S0;
  pairs_out = S1;
}

// One workgroup owns PS_TILE candidate poses over ALL chunks of the source: wave w walks chunks w, w + 8, ... with its 64 points in
// registers and, per chunk, loops over the tile's candidates (their 12 transform floats are wave-uniform: scalar loads).  The
// per-point terms of PS_BATCH candidates go through the wave's staging tile together (two rows each: score, pair count), are
// reduced by the gradient-pass tree (canon::reduce_grad) and split into the exact integer pieces, which meet in the workgroup's LDS
// bins; the workgroup folds its candidates' bins itself and stores two doubles per candidate.  No global atomics, no accumulator
// bank to clear, no second launch; the candidate index is blockIdx.x alone (2^20 candidates = 65 536 workgroups).
// dynamic LDS: [voxel table image: tab_bytes | eight staging tiles of canon::TILE_FLOATS floats]
constexpr int PS_BIN_SLOTS = 8;   // per (candidate, value): pieces 0-4, slot 5 = poison
template <int NOFF, int TAB>
__global__ __launch_bounds__(PS_THREADS) void ndt_score_poses_kernel(const NdtProblem P, const float* __restrict__ poses, const int count,
                                                                     const double d1d, const float d2, double* __restrict__ score,
                                                                     double* __restrict__ pairs, const int tab_bytes) {
  constexpr int NWAVES = PS_THREADS / 64;
  static_assert(2 * PS_BATCH == canon::TILE_ROWS && PS_TILE % PS_BATCH == 0 && PS_TILE * 2 * PS_BIN_SLOTS <= PS_THREADS, "tile geometry");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = (int)blockIdx.x * PS_TILE;
  if (c0 >= count) return;
  const int nc = min(PS_TILE, count - c0);
  __shared__ unsigned long long s_ibin[PS_TILE * 2 * PS_BIN_SLOTS];
  extern __shared__ uint4 s_table[];
  if (tid < PS_TILE * 2 * PS_BIN_SLOTS) s_ibin[tid] = 0ull;
  if (TAB == NDT_TAB_LDS) {   // the whole valid-voxel table -> LDS by wave-wide 16-byte DMA (the image is padded to whole KiB)
    const int nkib = P.lds_bytes >> 10;
    const unsigned char* img = reinterpret_cast<const unsigned char*>(P.lds_image) + (size_t)lane * 16;
    unsigned char* dst = reinterpret_cast<unsigned char*>(s_table);
    for (int c = wave; c < nkib; c += NWAVES)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(img + (size_t)c * 1024),
                                       (__attribute__((address_space(3))) void*)(dst + (size_t)c * 1024), 16, 0, 0);
  }
  __syncthreads();   // bins cleared, table landed (vmcnt(0) + barrier)

  float* s_tile = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(s_table) + tab_bytes) + wave * canon::TILE_FLOATS;
  const GlbFloat* g_sx = (const GlbFloat*)P.sx;
  const GlbFloat* g_sy = (const GlbFloat*)P.sy;
  const GlbFloat* g_sz = (const GlbFloat*)P.sz;
  const int n = P.n, nchunks = (n + 63) >> 6;
  for (int chunk = wave; chunk < nchunks; chunk += NWAVES) {   // one canonical chunk per wave and trip (absent points: zeros, no pairs)
    const int i = chunk * 64 + lane;
    const bool have = i < n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (have) { px = g_sx[i]; py = g_sy[i]; pz = g_sz[i]; }
    for (int jb = 0; jb < nc; jb += PS_BATCH) {
      const int nj = min(PS_BATCH, nc - jb);
      for (int j = 0; j < nj; j++) {
        const float* __restrict__ M = poses + 16 * (size_t)(c0 + jb + j);   // column-major 4x4, as ndt_fill_diag_state reads T16
        const float T[12] = {M[0], M[4], M[8], M[12], M[1], M[5], M[9], M[13], M[2], M[6], M[10], M[14]};
        float sc, np;
        score_point<NOFF, TAB>(P, s_table, have, px, py, pz, T, d2, d1d, sc, np);
        s_tile[(2 * j) * canon::TILE_PITCH + lane] = sc;
        s_tile[(2 * j + 1) * canon::TILE_PITCH + lane] = np;
      }
      wave_lds_fence();
#pragma unroll
      for (int r = 0; r < 2; r++) {
        if (8 * r >= 2 * nj) break;   // wave-uniform: rows of candidates this batch does not hold
        const int row = 8 * r + (lane >> 3), g = lane & 7;
        const double t = canon::reduce_grad(s_tile + row * canon::TILE_PITCH + 8 * g);   // every lane: the tree's DPP steps read their neighbours
        const int j = row >> 1;
        if (j < nj && g < NDT_NBINS) {
          bool poison;
          const int m = canon::piece(t, g, &poison);
          unsigned long long* b = &s_ibin[((jb + j) * 2 + (row & 1)) * PS_BIN_SLOTS];
          if (m != 0) atomicAdd(&b[g], (unsigned long long)(long long)m);
          if (poison && g == 0) atomicAdd(&b[5], 1ull);
        }
      }
      wave_lds_fence();   // the tile is read before the next batch writes it again
    }
  }

  __syncthreads();
  if (tid < 2 * nc) {   // (candidate, value): the fold of a derivative launch's head; a poisoned value poisons the pose, as it does a pass
    const int j = tid >> 1;
    const unsigned long long* b = &s_ibin[tid * PS_BIN_SLOTS];
    const bool poisoned = (s_ibin[(2 * j) * PS_BIN_SLOTS + 5] | s_ibin[(2 * j + 1) * PS_BIN_SLOTS + 5]) != 0ull;
    double t = canon::fold(canon::bin_value((long long)b[0], 0), canon::bin_value((long long)b[1], 1), canon::bin_value((long long)b[2], 2),
                           canon::bin_value((long long)b[3], 3), canon::bin_value((long long)b[4], 4));
    if (poisoned) t = canon::poisoned();
    if (tid & 1) pairs[c0 + j] = t; else score[c0 + j] = t;
  }
}

template <int NOFF, int TAB>
int launch_score_variant(const NdtProblem& P, const float* d_poses, int count, double d1, float d2, double* d_score, double* d_pairs,
                         int tab_bytes, hipStream_t stream) {
  const size_t dyn = (size_t)tab_bytes + (size_t)ndt_lane_tile_bytes(PS_THREADS);
  static bool allowed[64] = {};
  int dev = 0;
  LSR_HIP(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && !allowed[dev]) {   // table image + staging tiles, bounded by what a workgroup can have on gfx950
    LSR_HIP(hipFuncSetAttribute((const void*)ndt_score_poses_kernel<NOFF, TAB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024 - 4 * 1024));
    allowed[dev] = true;
  }
  const unsigned int nwg = (unsigned int)((count + PS_TILE - 1) / PS_TILE);
  hipLaunchKernelGGL((ndt_score_poses_kernel<NOFF, TAB>), dim3(nwg), dim3(PS_THREADS), dyn, stream, P, d_poses, count, d1, d2, d_score,
                     d_pairs, tab_bytes);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

template <int NOFF>
int launch_score(int tab, const NdtProblem& P, const float* d_poses, int count, double d1, float d2, double* d_score, double* d_pairs,
                 int tab_bytes, hipStream_t stream) {
  switch (tab) {
    case NDT_TAB_LDS: return launch_score_variant<NOFF, NDT_TAB_LDS>(P, d_poses, count, d1, d2, d_score, d_pairs, tab_bytes, stream);
    case NDT_TAB_COMPACT: return launch_score_variant<NOFF, NDT_TAB_COMPACT>(P, d_poses, count, d1, d2, d_score, d_pairs, 0, stream);
    default: return launch_score_variant<NOFF, NDT_TAB_DENSE>(P, d_poses, count, d1, d2, d_score, d_pairs, 0, stream);
  }
}

bool all_finite(const float* v, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// what lsr_ndt_derivatives checks before it runs, in its order; then the neighbourhoods this unit serves
int check_score_inputs(lsr_handle h) {
  if (!h->target || h->target->n == 0) { set_last_error("pose search before setInputTarget"); return LSR_ERR_NO_TARGET; }
  if (!h->has_source) { set_last_error("pose search before setInputSource"); return LSR_ERR_NO_SOURCE; }
  if (h->ndt.neighborhood == LSR_KDTREE) { set_last_error("pose search serves DIRECT7, DIRECT1 and DIRECT26, not KDTREE"); return LSR_ERR_NOT_IMPLEMENTED; }
  return LSR_OK;
}

// the scores of `count` checked poses (host, finite) -> score / pairs (host; pairs nullable); the object's answers stay as they were
int score_poses(lsr_handle h, const float* poses16, size_t count, double* score, double* pairs) {
  int st = ensure_ndt_grid(h);
  if (st) return st;
  if (h->target->grid.ncells == 0) { set_last_error("the input target holds no finite point"); return LSR_ERR_NO_TARGET; }
  NdtProblem P;
  int tab = NDT_TAB_DENSE, tab_bytes = 0;
  if ((st = ndt_score_problem(h, ndt_lane_tile_bytes(PS_THREADS) + 4 * 1024, &P, &tab, &tab_bytes))) return st;
  PoseSearchState& S = h->pose_search;
  S.ms = 0.0;
  if ((st = S.poses.reserve(16 * count))) return st;
  if ((st = S.out.reserve(2 * count))) return st;
  LSR_HIP(hipMemcpyAsync(S.poses.p, poses16, sizeof(float) * 16 * count, hipMemcpyHostToDevice, h->stream));
  double d1, d2;
  ndt_gauss_constants(h->ndt.resolution, h->ndt.outlier_ratio, &d1, &d2);
  if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));
  switch (h->ndt.neighborhood) {
    case LSR_DIRECT1: st = launch_score<1>(tab, P, S.poses.p, (int)count, d1, (float)d2, S.out.p, S.out.p + count, tab_bytes, h->stream); break;
    case LSR_DIRECT26: st = launch_score<27>(tab, P, S.poses.p, (int)count, d1, (float)d2, S.out.p, S.out.p + count, tab_bytes, h->stream); break;
    default: st = launch_score<7>(tab, P, S.poses.p, (int)count, d1, (float)d2, S.out.p, S.out.p + count, tab_bytes, h->stream); break;
  }
  if (st) return st;
  if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
  StreamDrain drain{h->stream};
  LSR_HIP(hipMemcpyAsync(score, S.out.p, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
  if (pairs) LSR_HIP(hipMemcpyAsync(pairs, S.out.p + count, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (h->profile && (st = add_ms(h->ev0, h->ev1, &S.ms))) return st;
  return LSR_OK;
}

bool lattice_count(const lsr_pose_lattice* L, size_t* count) {
  size_t c = 1;
  const int32_t n[4] = {L->n[0], L->n[1], L->n[2], L->n_yaw};
  for (int k = 0; k < 4; k++) {
    if (n[k] < 1) return false;
    c *= (size_t)n[k];
    if (c > PS_MAX_POSES) return false;
  }
  *count = c;
  return true;
}

}  // namespace
}  // namespace lsr

extern "C" {

int lsr_ndt_score_poses(lsr_handle h, const float* poses16, size_t count, double* score, double* pairs) {
  LSR_CHECK_HANDLE(h);
  if (!poses16 || !score || count == 0 || count > PS_MAX_POSES) { set_last_error("poses16 / score null, or count outside 1 .. LSR_POSE_SEARCH_MAX_POSES"); return LSR_ERR_INVALID_ARGUMENT; }
  if (!all_finite(poses16, 16 * count)) { set_last_error("poses16: an entry is not finite"); return LSR_ERR_INVALID_ARGUMENT; }
  if (int st = check_score_inputs(h)) return st;
  return score_poses(h, poses16, count, score, pairs);
}

int lsr_pose_lattice_poses(const float* center16, const lsr_pose_lattice* L, float* poses16, size_t capacity, size_t* count) {
#pragma clang fp contract(off)
  if (!center16 || !L || !count) { set_last_error("center16, lattice or count is null"); return LSR_ERR_INVALID_ARGUMENT; }
  size_t total = 0;
  if (!lattice_count(L, &total)) { set_last_error("pose lattice: every n is at least 1 and their product at most LSR_POSE_SEARCH_MAX_POSES"); return LSR_ERR_INVALID_ARGUMENT; }
  if (!all_finite(center16, 16) || !std::isfinite(L->step[0]) || !std::isfinite(L->step[1]) || !std::isfinite(L->step[2]) || !std::isfinite(L->yaw_step)) {
    set_last_error("pose lattice: the centre and the steps must be finite");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  *count = total;
  if (!poses16) return LSR_OK;
  if (capacity < total) { set_last_error("pose lattice: capacity below the count"); return LSR_ERR_INVALID_ARGUMENT; }
  double R[3][3], t[3];   // the float centre, widened
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r][c] = (double)center16[4 * c + r];
    t[r] = (double)center16[12 + r];
  }
  float* out = poses16;
  for (int m = 0; m < L->n_yaw; m++) {
    const double psi = ((double)m - (double)(L->n_yaw - 1) / 2.0) * L->yaw_step;
    const double cs = std::cos(psi), sn = std::sin(psi);
    double Rc[3][3];   // Rz(psi) * R_center
    for (int c = 0; c < 3; c++) {
      Rc[0][c] = cs * R[0][c] - sn * R[1][c];
      Rc[1][c] = sn * R[0][c] + cs * R[1][c];
      Rc[2][c] = R[2][c];
    }
    for (int k = 0; k < L->n[2]; k++) {
      const double tz = t[2] + ((double)k - (double)(L->n[2] - 1) / 2.0) * L->step[2];
      for (int j = 0; j < L->n[1]; j++) {
        const double ty = t[1] + ((double)j - (double)(L->n[1] - 1) / 2.0) * L->step[1];
        for (int i = 0; i < L->n[0]; i++, out += 16) {
          const double tx = t[0] + ((double)i - (double)(L->n[0] - 1) / 2.0) * L->step[0];
          for (int c = 0; c < 3; c++) {
            out[4 * c + 0] = (float)Rc[0][c]; out[4 * c + 1] = (float)Rc[1][c]; out[4 * c + 2] = (float)Rc[2][c]; out[4 * c + 3] = 0.f;
          }
          out[12] = (float)tx; out[13] = (float)ty; out[14] = (float)tz; out[15] = 1.f;
        }
      }
    }
  }
  return LSR_OK;
}

int lsr_select_poses(const double* score, const float* poses16, size_t count, int top_k, double min_sep_m, double min_sep_rad,
                     int32_t* kept, int* n_kept) {
#pragma clang fp contract(off)
  if (!score || !poses16 || !kept || !n_kept || count == 0 || count > PS_MAX_POSES) { set_last_error("score / poses16 / kept / n_kept null, or count outside 1 .. LSR_POSE_SEARCH_MAX_POSES"); return LSR_ERR_INVALID_ARGUMENT; }
  if (top_k < 1 || top_k > LSR_POSE_SEARCH_MAX_KEPT) { set_last_error("top_k must be in 1 .. 16"); return LSR_ERR_INVALID_ARGUMENT; }
  if (min_sep_m != min_sep_m || min_sep_rad != min_sep_rad) { set_last_error("the separations must not be NaN"); return LSR_ERR_INVALID_ARGUMENT; }
  try {
    std::vector<int32_t> order;
    order.reserve(count);
    for (size_t c = 0; c < count; c++)
      if (score[c] > 0) order.push_back((int32_t)c);   // NaN and anything not > 0 is never kept
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return score[a] > score[b]; });   // ties: ascending index
    const double cos_sep = std::cos(min_sep_rad);
    int nk = 0;
    for (int32_t c : order) {
      const float* A = poses16 + 16 * (size_t)c;
      bool close = false;
      for (int e = 0; e < nk && !close; e++) {
        const float* B = poses16 + 16 * (size_t)kept[e];
        const double dx = (double)A[12] - (double)B[12], dy = (double)A[13] - (double)B[13], dz = (double)A[14] - (double)B[14];
        const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
        double tr = 0.0;   // trace(R_a^T R_b): the nine products in storage order
        for (int col = 0; col < 3; col++)
          for (int r = 0; r < 3; r++) tr += (double)A[4 * col + r] * (double)B[4 * col + r];
        close = (dist < min_sep_m) && ((tr - 1.0) / 2.0 > cos_sep);
      }
      if (close) continue;
      kept[nk++] = c;
      if (nk == top_k) break;
    }
    *n_kept = nk;
  } catch (const std::exception& e) {
    set_last_error(std::string("pose selection: host allocation failed: ") + e.what());
    return LSR_ERR_HIP;
  }
  return LSR_OK;
}

int lsr_ndt_search_pose(lsr_handle h, const float* center16, const lsr_pose_search_params* p, float* best16, lsr_result* result,
                        lsr_pose_search_report* report) {
  LSR_CHECK_HANDLE(h);
  if (!center16 || !p || !best16 || !result) { set_last_error("center16, params, best16 or result is null"); return LSR_ERR_INVALID_ARGUMENT; }
  if (h->method != LSR_METHOD_NDT) { set_last_error("lsr_ndt_search_pose on a GICP object"); return LSR_ERR_INVALID_ARGUMENT; }
  if (p->top_k < 1 || p->top_k > LSR_POSE_SEARCH_MAX_KEPT) { set_last_error("top_k must be in 1 .. 16"); return LSR_ERR_INVALID_ARGUMENT; }
  size_t count = 0;
  int st = lsr_pose_lattice_poses(center16, &p->lattice, nullptr, 0, &count);
  if (st) return st;
  if ((st = check_score_inputs(h))) return st;
  std::vector<float> poses;
  std::vector<double> score;
  try {
    poses.resize(16 * count);
    score.resize(count);
  } catch (const std::exception& e) {
    set_last_error(std::string("pose search: host allocation failed: ") + e.what());
    return LSR_ERR_HIP;
  }
  if ((st = lsr_pose_lattice_poses(center16, &p->lattice, poses.data(), count, &count))) return st;
  if ((st = score_poses(h, poses.data(), count, score.data(), nullptr))) return st;
  int32_t kept[LSR_POSE_SEARCH_MAX_KEPT];
  int n_kept = 0;
  if ((st = lsr_select_poses(score.data(), poses.data(), count, p->top_k, p->min_sep_m, p->min_sep_rad, kept, &n_kept))) return st;
  if (report) {
    std::memset(report, 0, sizeof(*report));
    report->n_candidates = (int32_t)count;
    report->n_kept = n_kept;
    report->winner = -1;
    for (int e = 0; e < n_kept; e++) { report->kept[e] = kept[e]; report->coarse_score[e] = score[kept[e]]; }
  }
  if (n_kept == 0) {   // no pose of the lattice puts a point into a voxel: nothing to refine, the object keeps its last result
    std::memset(result, 0, sizeof(*result));
    return LSR_OK;
  }

  // One worker object per kept candidate, as lsr_search_loop(top_k > 1) keeps them (loop_search.hip): on the object's stream, sharing
  // its target (lsr_share_target's mechanism: the same TargetData), each with a device copy of the source; the set goes through
  // align_ndt_batch as one launch chain, and every member ends on the bits lsr_align(h, candidate) gives alone (canonical sums).
  while ((int)h->aux.size() < n_kept) {
    std::unique_ptr<lsr_handle_s> a(new (std::nothrow) lsr_handle_s());
    if (!a) return LSR_ERR_HIP;
    a->method = h->method; a->device = h->device; a->stream = h->stream; a->own_stream = false;
    if (a->d_T16.reserve(16) != LSR_OK) return LSR_ERR_HIP;
    h->aux.push_back(std::move(a));
  }
  struct Unshare {   // the workers let go of the target on every way out: `h` alone holds it again, as before the call
    lsr_handle h; int n;
    ~Unshare() { for (int e = 0; e < n; e++) h->aux[e]->target.reset(); }
  } unshare{h, n_kept};
  lsr_handle workers[LSR_POSE_SEARCH_MAX_KEPT];
  float guesses[16 * LSR_POSE_SEARCH_MAX_KEPT], finals[16 * LSR_POSE_SEARCH_MAX_KEPT];
  lsr_result results[LSR_POSE_SEARCH_MAX_KEPT];
  for (int e = 0; e < n_kept; e++) {
    lsr_handle a = h->aux[e].get();
    a->ndt = h->ndt; a->gicp = h->gicp;
    a->ndt_threads = h->ndt_threads; a->ndt_table_mode = h->ndt_table_mode; a->ndt_quad = h->ndt_quad; a->ndt_split = h->ndt_split;
    a->scratch.wait_mode = h->scratch.wait_mode; a->scratch.force_sort_path = h->scratch.force_sort_path;
    a->target = h->target;
    if ((st = a->source.resize(h->source.n))) return st;
    if (h->source.n) {
      LSR_HIP(hipMemcpyAsync(a->source.x(), h->source.x(), sizeof(float) * h->source.n, hipMemcpyDeviceToDevice, h->stream));
      LSR_HIP(hipMemcpyAsync(a->source.y(), h->source.y(), sizeof(float) * h->source.n, hipMemcpyDeviceToDevice, h->stream));
      LSR_HIP(hipMemcpyAsync(a->source.z(), h->source.z(), sizeof(float) * h->source.n, hipMemcpyDeviceToDevice, h->stream));
    }
    a->has_source = true;
    a->source_cov_valid = false;
    workers[e] = a;
    std::memcpy(guesses + 16 * e, poses.data() + 16 * (size_t)kept[e], sizeof(float) * 16);
    std::memset(&results[e], 0, sizeof(lsr_result));
  }
  if ((st = align_ndt_batch(workers, n_kept, guesses, finals, results))) return st;
  int winner = 0;   // the largest trans_probability, ties to the lower rank
  for (int e = 1; e < n_kept; e++)
    if (results[e].score > results[winner].score) winner = e;
  std::memcpy(best16, finals + 16 * winner, sizeof(float) * 16);
  *result = results[winner];
  std::memcpy(h->final_T, finals + 16 * winner, sizeof(float) * 16);   // as after align
  h->converged = results[winner].converged;
  if (report) {
    report->winner = winner;
    std::memcpy(report->refined16, finals, sizeof(float) * 16 * n_kept);
    for (int e = 0; e < n_kept; e++) report->refined[e] = results[e];
  }
  return LSR_OK;
}

}  // extern "C"

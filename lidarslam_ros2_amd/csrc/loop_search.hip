// ---- N3: loop-closure gate ---------------------------------------------------------------------
// lsr_search_loop of the C ABI (include/lidarslam_reg.h): candidate selection and relative poses in host fp64, the candidates'
// windows, registrations and scores through the object's own entries.  Host-side orchestration only.
#include <algorithm>
#include <cmath>

#include "api_internal.hpp"

using namespace lsr;

// tf2::fromMsg(geometry_msgs::Pose) -> Eigen::Affine3d = Translation * Quaterniond (Eigen's toRotationMatrix, no
// normalisation), column-major 4x4 (graph_based_slam_component.cpp:171,177,219,236-238)
void lsr::submap_pose_matrix(const lsr_submap& s, double M[16]) {
  const double x = s.orientation[0], y = s.orientation[1], z = s.orientation[2], w = s.orientation[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y,
               tzz = tz * z;
  M[0] = 1 - (tyy + tzz); M[4] = txy - twz;       M[8] = txz + twy;        M[12] = s.position[0];
  M[1] = txy + twz;       M[5] = 1 - (txx + tzz); M[9] = tyz - twx;        M[13] = s.position[1];
  M[2] = txz - twy;       M[6] = tyz + twx;       M[10] = 1 - (txx + tyy); M[14] = s.position[2];
  M[3] = 0; M[7] = 0; M[11] = 0; M[15] = 1;
}

namespace {
void mat4_mul(const double* A, const double* B, double* C) {  // column-major C = A * B
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++) {
      double acc = 0;
      for (int k = 0; k < 4; k++) acc += A[r + 4 * k] * B[k + 4 * c];
      C[r + 4 * c] = acc;
    }
}
void isometry_inverse(const double* M, double* I) {  // Eigen::Isometry3d::inverse(): [R^T | -R^T t]
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) I[r + 4 * c] = M[c + 4 * r];
  for (int r = 0; r < 3; r++) I[r + 12] = -(I[r] * M[12] + I[r + 4] * M[13] + I[r + 8] * M[14]);
  I[3] = I[7] = I[11] = 0; I[15] = 1;
}
// source = latest submap moved by its own pose (:171-181); init_M = that pose
int set_loop_source(lsr_handle h, const lsr_submap& latest, size_t stride_bytes, int on_device, double* init_M) {
  if (latest.n_points == 0 || !latest.cloud) { set_last_error("latest submap has no points"); return LSR_ERR_NO_SOURCE; }
  submap_pose_matrix(latest, init_M);
  float pose_f[16];
  for (int k = 0; k < 16; k++) pose_f[k] = (float)init_M[k];
  const void* fr[1] = {latest.cloud};
  const size_t cn[1] = {latest.n_points};
  int st = assemble_frames(h, 1, fr, cn, stride_bytes, pose_f, on_device != 0, h->source);
  if (st) return st;
  h->has_source = true;
  h->source_cov_valid = false;
  return LSR_OK;
}

// G = M_cand Rz(shift 2 pi / S) M_latest^-1 in fp64, cast to float element by element (include/lidarslam_reg.h)
void appearance_guess(const lsr_submap& candidate, const lsr_submap& latest, int shift, int num_sectors, float* guess16) {
  double Mc[16], Ml[16], Mli[16], Rz[16] = {0}, A[16], G[16];
  submap_pose_matrix(candidate, Mc);
  submap_pose_matrix(latest, Ml);
  isometry_inverse(Ml, Mli);
  const double a = (double)shift * (2.0 * 3.141592653589793) / (double)num_sectors;
  const double cs = std::cos(a), sn = std::sin(a);
  Rz[0] = cs; Rz[1] = sn; Rz[4] = -sn; Rz[5] = cs; Rz[10] = 1; Rz[15] = 1;
  mat4_mul(Mc, Rz, A);
  mat4_mul(A, Mli, G);
  for (int k = 0; k < 16; k++) guess16[k] = (float)G[k];
}

// The part of the gate behind candidate selection, shared by lsr_search_loop and lsr_search_loop_appearance: the first k_eval entries
// of `cand` (position distance, submap index), each with its window target, a registration of the source `h` already holds, the
// fitness, the threshold and the relative pose.  guesses16 == nullptr: align without guess, as the reference (:230); k_eval > 1 with
// NDT then runs as one candidate set.  guesses16 != nullptr (16 floats per candidate): one after another on `h`; NDT searches the
// lattice `search` around the guess (lsr_ndt_search_pose), GICP aligns once from it.
int evaluate_candidates(lsr_handle h, const lsr_submap* submaps, int num_submaps, size_t stride_bytes, int on_device,
                        const lsr_loop_params* params, const double* init_M, const std::vector<std::pair<double, int>>& cand, int k_eval,
                        const float* guesses16, const lsr_pose_search_params* search, lsr_loop_edge* edges, int* n_evaluated) {
  // One worker registration object per candidate evaluated together.  top_k = 1 (the reference) uses `h` itself; with
  // top_k > 1 and NDT the k windows are assembled into k auxiliary objects (own target, a device copy of the source, the
  // caller's stream) and advanced in ONE shared launch chain (align_ndt_batch) instead of k chains one after another.
  const bool batched = (!guesses16 && k_eval > 1 && h->method == LSR_METHOD_NDT);
  std::vector<lsr_handle> workers((size_t)k_eval, h);
  if (batched) {
    while ((int)h->aux.size() < k_eval) {
      std::unique_ptr<lsr_handle_s> a(new (std::nothrow) lsr_handle_s());
      if (!a) return LSR_ERR_HIP;
      a->method = h->method; a->device = h->device; a->stream = h->stream; a->own_stream = false;
      if (a->d_T16.reserve(16) != LSR_OK) return LSR_ERR_HIP;
      h->aux.push_back(std::move(a));
    }
    for (int e = 0; e < k_eval; e++) {
      lsr_handle a = h->aux[e].get();
      a->ndt = h->ndt; a->gicp = h->gicp;
      a->ndt_threads = h->ndt_threads; a->ndt_table_mode = h->ndt_table_mode; a->ndt_quad = h->ndt_quad;
      a->scratch.wait_mode = h->scratch.wait_mode; a->scratch.force_sort_path = h->scratch.force_sort_path;
      int st = a->source.resize(h->source.n);
      if (st) return st;
      if (h->source.n) {
        LSR_HIP(hipMemcpyAsync(a->source.x(), h->source.x(), sizeof(float) * h->source.n, hipMemcpyDeviceToDevice, h->stream));
        LSR_HIP(hipMemcpyAsync(a->source.y(), h->source.y(), sizeof(float) * h->source.n, hipMemcpyDeviceToDevice, h->stream));
        LSR_HIP(hipMemcpyAsync(a->source.z(), h->source.z(), sizeof(float) * h->source.n, hipMemcpyDeviceToDevice, h->stream));
      }
      a->has_source = true;
      a->source_cov_valid = false;
      workers[e] = a;
    }
  }

  std::vector<const void*> frames;
  std::vector<size_t> counts;
  std::vector<float> poses;
  std::vector<lsr_result> results((size_t)k_eval);
  std::vector<int> n_target((size_t)k_eval, 0);
  std::shared_ptr<TargetData> first_target;   // with guesses and k_eval > 1: the first candidate's window, handed back to `h` at the end
  for (int e = 0; e < k_eval; e++) std::memset(&results[e], 0, sizeof(lsr_result));
  // ---- targets: window assembly (:207-222), voxelgrid_.filter + setInputTarget (:224-227)
  for (int e = 0; e < k_eval; e++) {
    lsr_handle w = workers[e];
    const int id_min = cand[e].second;
    // The reference only guards the lower end of the window; an index past the last submap would read out of bounds
    // there, so it is skipped here.
    frames.clear(); counts.clear(); poses.clear();
    for (int j = 0; j <= 2 * params->search_submap_num; j++) {
      const int idx = id_min + j - params->search_submap_num;
      if (idx < 0 || idx >= num_submaps) continue;
      double M[16];
      submap_pose_matrix(submaps[idx], M);
      frames.push_back(submaps[idx].cloud);
      counts.push_back(submaps[idx].n_points);
      for (int k = 0; k < 16; k++) poses.push_back((float)M[k]);
    }
    int st = assemble_frames(w, (int)frames.size(), frames.data(), counts.data(), stride_bytes, poses.data(), on_device != 0, w->raw);
    if (st) return st;
    auto t = fresh_target(w);
    if ((st = voxel_grid_filter(w->raw, params->voxel_leaf_size, t->cloud, w->scratch, w->stream))) return st;
    t->n = t->cloud.n;
    w->target = t;
    n_target[e] = (int)t->n;
    st = (w->method == LSR_METHOD_NDT) ? ensure_ndt_grid(w) : ensure_target_hash(w);
    if (st) { w->target.reset(); return st; }
    if (!batched) {  // serial: align(output) without guess (:230) right away — the next candidate re-uses `h`'s target slot
      lsr_loop_edge& E = edges[e];
      std::memset(&E, 0, sizeof(E));
      const float* G = guesses16 ? guesses16 + 16 * (size_t)e : nullptr;
      if (h->method == LSR_METHOD_NDT && G) {
        std::memcpy(E.final_transformation, G, sizeof(float) * 16);   // what stands when the search keeps no pose of the lattice
        if ((st = lsr_ndt_search_pose(h, G, search, E.final_transformation, &results[e], nullptr))) return st;
        std::memcpy(h->final_T, E.final_transformation, sizeof(float) * 16);
        h->converged = results[e].converged;
      } else if (h->method == LSR_METHOD_NDT) {
        lsr_handle hs[1] = {h};
        st = align_ndt_batch(hs, 1, nullptr, E.final_transformation, &results[e]);
      } else {
        st = gicp_align(h, G, E.final_transformation, &results[e]);
      }
      if (st) return st;
      if ((st = ensure_target_hash(h))) return st;
      double fitness = 0;   // getFitnessScore() (:231)
      if ((st = nn_fitness_score(h->source, h->final_T, h->target->hash, 1.7976931348623157e308, &fitness, h->scratch, h->d_T16, h->stream)))
        return st;
      E.fitness_score = fitness;
      if (guesses16 && e == 0 && k_eval > 1) first_target = h->target;   // kept from the next candidates' fresh_target
    }
  }
  if (first_target) {   // `h` answers for the first candidate and holds its window, as after one candidate
    h->target = first_target;
    h->spare_target = first_target;
    std::memcpy(h->final_T, edges[0].final_transformation, sizeof(float) * 16);
    h->converged = results[0].converged;
  }
  if (batched) {
    std::vector<float> finals((size_t)k_eval * 16);
    // align + getFitnessScore of the k candidates (graph_based_slam_component.cpp:230-231): the searches of the candidates that
    // finish early run under the launch chain of the others
    std::vector<double> fit((size_t)k_eval);
    int st = align_ndt_batch(workers.data(), k_eval, nullptr, finals.data(), results.data(), fit.data(), 1.7976931348623157e308);
    if (st) return st;
    for (int e = 0; e < k_eval; e++) {
      lsr_handle w = workers[e];
      lsr_loop_edge& E = edges[e];
      std::memset(&E, 0, sizeof(E));
      std::memcpy(E.final_transformation, finals.data() + 16 * e, sizeof(float) * 16);
      double fitness = fit[e];
      if (fitness != fitness) {   // not served under the chain (its grid is not a refinement of a counting-sort voxel grid)
        if ((st = ensure_target_hash(w))) return st;
        if ((st = nn_fitness_score(w->source, w->final_T, w->target->hash, 1.7976931348623157e308, &fitness, w->scratch, w->d_T16, w->stream)))
          return st;
      }
      E.fitness_score = fitness;
    }
    // `h` reports the best candidate like a single registration would (getFinalTransformation / hasConverged)
    std::memcpy(h->final_T, edges[0].final_transformation, sizeof(float) * 16);
    h->converged = results[0].converged;
    // ... and it holds that candidate's window as its input target, exactly as after top_k = 1 (where the one candidate is
    // registered on `h` itself, graph_based_slam_component.cpp:227): a later getFitnessScore() / align() on `h` pairs the pose
    // just stored with the window it was registered against.  The worker takes `h`'s previous target object in exchange, so
    // both keep recycling one set of device buffers each.
    {
      lsr_handle w0 = workers[0];
      std::shared_ptr<TargetData> best = w0->target, old = h->target ? h->target : h->spare_target;
      h->target = best;
      h->spare_target = best;
      w0->target.reset();
      w0->spare_target = old;
    }
  }
  for (int e = 0; e < k_eval; e++) {
    const int id_min = cand[e].second;
    lsr_loop_edge& E = edges[e];
    E.id_from = id_min;
    E.id_to = num_submaps - 1;
    E.converged = results[e].converged;
    E.iterations = results[e].iterations;
    E.n_target_points = n_target[e];
    E.candidate_distance = cand[e].first;
    E.accepted = E.fitness_score < params->threshold_loop_closure_score ? 1 : 0;
    // relative pose of the loop edge (:236-245): from^-1 * (final * init)
    double fin[16], to[16], from[16], from_inv[16];
    for (int k = 0; k < 16; k++) fin[k] = (double)E.final_transformation[k];
    mat4_mul(fin, init_M, to);
    submap_pose_matrix(submaps[id_min], from);
    isometry_inverse(from, from_inv);
    mat4_mul(from_inv, to, E.relative_pose);
    (*n_evaluated)++;
  }
  return LSR_OK;
}
}  // namespace

extern "C" {

int lsr_search_loop(lsr_handle h, const lsr_submap* submaps, int num_submaps, size_t stride_bytes, int on_device,
                    const lsr_loop_params* params, lsr_loop_edge* edges, int edge_capacity, int* n_evaluated) {
  LSR_CHECK_HANDLE(h);
  if (!submaps || num_submaps <= 0 || !params || !n_evaluated || stride_bytes < 12 || (stride_bytes % 4) ||
      (edge_capacity > 0 && !edges) || edge_capacity < 0) {
    set_last_error("bad argument");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (!(params->voxel_leaf_size > 0) || params->search_submap_num < 0) {
    set_last_error("voxel_leaf_size must be > 0 and search_submap_num >= 0");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  *n_evaluated = 0;
  const lsr_submap& latest = submaps[num_submaps - 1];
  double init_M[16];
  if (int st = set_loop_source(h, latest, stride_bytes, on_device, init_M)) return st;

  // candidates (:188-205): enough travel since, close enough now; nearest first (ties: lower index, as the
  // strict `dist < min_dist` of the reference keeps the first minimum)
  std::vector<std::pair<double, int>> cand;
  for (int i = 0; i < num_submaps; i++) {
    const double dx = latest.position[0] - submaps[i].position[0], dy = latest.position[1] - submaps[i].position[1],
                 dz = latest.position[2] - submaps[i].position[2];
    const double dist = std::sqrt(dx * dx + dy * dy + dz * dz);
    if (latest.distance - submaps[i].distance > params->distance_loop_closure && dist < params->range_of_searching_loop_closure)
      cand.emplace_back(dist, i);
  }
  if (cand.empty()) return LSR_OK;
  std::stable_sort(cand.begin(), cand.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
  const int k_eval = std::min({std::max(params->top_k, 1), (int)cand.size(), edge_capacity});

  return evaluate_candidates(h, submaps, num_submaps, stride_bytes, on_device, params, init_M, cand, k_eval, nullptr, nullptr, edges, n_evaluated);
}

int lsr_scan_context_guess(const lsr_submap* candidate, const lsr_submap* latest, int shift, int num_sectors, float* guess16) {
  if (!candidate || !latest || !guess16) { set_last_error("candidate, latest or guess16 is null"); return LSR_ERR_INVALID_ARGUMENT; }
  if (num_sectors < 2 || num_sectors > LSR_SCAN_CONTEXT_MAX_SECTORS || (num_sectors & 1) || shift < 0 || shift >= num_sectors) {
    set_last_error("num_sectors must be even and in 2 .. 120, shift in 0 .. num_sectors - 1");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  appearance_guess(*candidate, *latest, shift, num_sectors, guess16);
  return LSR_OK;
}

// ---- N10: the loop gate by appearance ----------------------------------------------------------
// Candidate and heading from the Scan Context comparison of the latest descriptor with every stored one (one launch), the translation
// from the pose search around the guess that follows from them.  The range gate of searchLoop (:196) is NOT applied: the stored
// positions are what has drifted.
int lsr_search_loop_appearance(lsr_handle h, const lsr_submap* submaps, int num_submaps, size_t stride_bytes, int on_device,
                               const float* descriptors, int num_descriptors, int desc_on_device,
                               const lsr_appearance_loop_params* params, lsr_loop_edge* edges, int32_t* shifts, float* sc_dist,
                               int edge_capacity, int* n_evaluated) {
  LSR_CHECK_HANDLE(h);
  if (!submaps || num_submaps <= 0 || !params || !n_evaluated || stride_bytes < 12 || (stride_bytes % 4) ||
      (edge_capacity > 0 && !edges) || edge_capacity < 0 || !descriptors) {
    set_last_error("bad argument");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  const lsr_loop_params* lp = &params->loop;
  if (!(lp->voxel_leaf_size > 0) || lp->search_submap_num < 0) {
    set_last_error("voxel_leaf_size must be > 0 and search_submap_num >= 0");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (num_descriptors != num_submaps) { set_last_error("num_descriptors: one descriptor per submap"); return LSR_ERR_INVALID_ARGUMENT; }
  if ((uintptr_t)descriptors & 3) { set_last_error("descriptors: must be 4-byte aligned"); return LSR_ERR_INVALID_ARGUMENT; }
  ScTables T;
  int st = scan_context_tables(&params->sc, &T);
  if (st) return st;
  if (params->sc_distance_threshold != params->sc_distance_threshold) { set_last_error("sc_distance_threshold is NaN"); return LSR_ERR_INVALID_ARGUMENT; }
  if (h->method == LSR_METHOD_NDT && (params->search.top_k < 1 || params->search.top_k > LSR_POSE_SEARCH_MAX_KEPT)) {
    set_last_error("search.top_k must be in 1 .. 16");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  *n_evaluated = 0;
  const lsr_submap& latest = submaps[num_submaps - 1];
  double init_M[16];
  if ((st = set_loop_source(h, latest, stride_bytes, on_device, init_M))) return st;

  // the latest descriptor against every stored one, all shifts, one launch
  const size_t cells = (size_t)T.R * (size_t)T.S, n = (size_t)num_submaps;
  ScanContextState& W = h->scan_context;
  W.match_ms = 0.0;
  std::vector<float> dist(n);
  std::vector<int32_t> shift(n);
  {
    if ((st = W.dist.reserve(n)) || (st = W.shift.reserve(n))) return st;
    const float* d_all = descriptors;
    StreamDrain drain{h->stream};
    if (!desc_on_device) {
      if ((st = W.cand.reserve(cells * n))) return st;
      LSR_HIP(hipMemcpyAsync(W.cand.p, descriptors, sizeof(float) * cells * n, hipMemcpyHostToDevice, h->stream));
      d_all = W.cand.p;
    }
    if (h->profile) LSR_HIP(hipEventRecord(h->ev0, h->stream));
    if ((st = scan_context_match(d_all + cells * (n - 1), 1, d_all, num_submaps, T.R, T.S, W.dist.p, W.shift.p, h->stream))) return st;
    if (h->profile) LSR_HIP(hipEventRecord(h->ev1, h->stream));
    LSR_HIP(hipMemcpyAsync(dist.data(), W.dist.p, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipMemcpyAsync(shift.data(), W.shift.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
    LSR_HIP(hipStreamSynchronize(h->stream));
    if (h->profile && (st = add_ms(h->ev0, h->ev1, &W.match_ms))) return st;
  }

  // candidates: enough travel since (:195) and alike enough; most alike first (ties: lower index)
  std::vector<int> order;
  for (int i = 0; i < num_submaps; i++)
    if (latest.distance - submaps[i].distance > lp->distance_loop_closure && (double)dist[i] < params->sc_distance_threshold) order.push_back(i);
  if (order.empty()) return LSR_OK;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return dist[a] < dist[b]; });
  const int k_eval = std::min({std::max(lp->top_k, 1), (int)order.size(), edge_capacity});
  std::vector<std::pair<double, int>> cand;
  std::vector<float> guesses((size_t)k_eval * 16);
  for (int e = 0; e < k_eval; e++) {
    const int i = order[e];
    const double dx = latest.position[0] - submaps[i].position[0], dy = latest.position[1] - submaps[i].position[1],
                 dz = latest.position[2] - submaps[i].position[2];
    cand.emplace_back(std::sqrt(dx * dx + dy * dy + dz * dz), i);   // candidate_distance stays the position distance
    appearance_guess(submaps[i], latest, shift[i], T.S, guesses.data() + 16 * (size_t)e);
  }
  if ((st = evaluate_candidates(h, submaps, num_submaps, stride_bytes, on_device, lp, init_M, cand, k_eval, guesses.data(), &params->search,
                                edges, n_evaluated)))
    return st;
  for (int e = 0; e < k_eval; e++) {
    if (shifts) shifts[e] = shift[order[e]];
    if (sc_dist) sc_dist[e] = dist[order[e]];
  }
  return LSR_OK;
}

}  // extern "C"

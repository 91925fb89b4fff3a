// C ABI of the registration core (include/lidarslam_reg.h): the object itself, its keys, align / fitness / accessor dispatch and the
// thin pose-graph, GICP inspection and profile entries.  Host-side orchestration only; the other entries live with their subsystem
// (inputs.hip, ndt_align.hip, loop_search.hip, map_output.hip, comm.hip, deskew.hip).  No CPU fallback exists — every compute
// entry point runs HIP kernels on a gfx950 device or returns an error status.
#include <cmath>
#include <cstdlib>

#include "api_internal.hpp"

namespace lsr {
static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }
}  // namespace lsr

using namespace lsr;

extern "C" {

const char* lsr_version(void) { return "lidarslam_reg 0.1.0 (gfx950)"; }

const char* lsr_status_string(int status) {
  switch (status) {
    case LSR_OK: return "ok";
    case LSR_ERR_INVALID_ARGUMENT: return "invalid argument";
    case LSR_ERR_NO_DEVICE: return "no usable gfx950 device";
    case LSR_ERR_HIP: return "HIP runtime error";
    case LSR_ERR_NO_TARGET: return "input target not set";
    case LSR_ERR_NO_SOURCE: return "input source not set";
    case LSR_ERR_NOT_IMPLEMENTED: return "not implemented";
    case LSR_ERR_INDEX_OVERFLOW: return "voxel index overflow";
    case LSR_ERR_TOO_FEW_POINTS: return "too few points";
    case LSR_ERR_IO: return "file input/output error";
    default: return "unknown status";
  }
}

const char* lsr_last_error(void) { return g_last_error.c_str(); }

int lsr_device_count(int* count) {
  if (!count) return LSR_ERR_INVALID_ARGUMENT;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    *count = 0;
    return LSR_ERR_NO_DEVICE;
  }
  *count = n;
  return LSR_OK;
}

int lsr_create(int method, int device_id, void* stream, lsr_handle* out) {
  if (!out || (method != LSR_METHOD_NDT && method != LSR_METHOD_GICP)) {
    set_last_error("invalid registration method");  // scanmatcher_component.cpp:121-124
    return LSR_ERR_INVALID_ARGUMENT;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) {
    set_last_error("no HIP device available (this library has no CPU path)");
    return LSR_ERR_NO_DEVICE;
  }
  DeviceGuard guard(device_id);
  if (!guard.ok) return LSR_ERR_NO_DEVICE;
  lsr_handle h = new (std::nothrow) lsr_handle_s();
  if (!h) return LSR_ERR_HIP;
  h->method = method;
  h->device = device_id;
  // pclomp ctor defaults
  h->ndt.resolution = 1.0; h->ndt.step_size = 0.1; h->ndt.outlier_ratio = 0.55; h->ndt.trans_eps = 0.1;
  h->ndt.max_iterations = 35; h->ndt.neighborhood = LSR_DIRECT7; h->ndt.d1_sign = 1;
  // tuning defaults may be preset from the environment (A/B runs without touching the caller)
  if (const char* e = std::getenv("LSR_NDT_WORKGROUP")) {
    const int v = std::atoi(e);
    if (v == 64 || v == 128 || v == 512 || v == 1024) h->ndt_threads = v;
    else if (v != 0) fprintf(stderr, "[lidarslam_reg] LSR_NDT_WORKGROUP=%d ignored: 64 / 128 (quad kernel, points) or 512 / 1024 (lane kernel, threads)\n", v);
  }
  if (const char* e = std::getenv("LSR_NDT_TABLE_MODE")) { const int v = std::atoi(e); if (v >= -1 && v <= 2) h->ndt_table_mode = v; }
  if (const char* e = std::getenv("LSR_NDT_QUAD")) { const int v = std::atoi(e); if (v >= -1 && v <= 1) h->ndt_quad = v; }
  if (const char* e = std::getenv("LSR_NDT_SPLIT")) { const int v = std::atoi(e); if (v >= -1 && v <= 1) h->ndt_split = v; }
  if (const char* e = std::getenv("LSR_WAIT_MODE")) {   // 0 | 1 | 2 or spin | yield | sleep
    const std::string w(e);
    const int v = (w == "spin") ? 0 : (w == "yield") ? 1 : (w == "sleep") ? 2 : (w.size() == 1 && w[0] >= '0' && w[0] <= '2') ? w[0] - '0' : -1;
    if (v >= 0) h->scratch.wait_mode = v;
  }
  if (const char* e = std::getenv("LSR_GRID_BUILDER")) { h->scratch.force_sort_path = (std::atoi(e) == 1); }
  if (stream) {
    h->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
      set_last_error("hipStreamCreateWithFlags failed");
      delete h;
      return LSR_ERR_HIP;
    }
    h->own_stream = true;
  }
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess || h->d_T16.reserve(16) != LSR_OK) {
    set_last_error("handle resources could not be created");
    (void)lsr_destroy(h);  // releases whatever was created so far
    return LSR_ERR_HIP;
  }
  *out = h;
  return LSR_OK;
}

// Streams and events of one handle object (the public handle and the worker objects lsr_search_loop(top_k > 1) keeps in h->aux: a
// worker that led a batch owns a side stream, chain streams and their events just like a public handle).
static void release_handle_streams(lsr_handle h) {
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->side_stream) { (void)hipStreamSynchronize(h->side_stream); (void)hipStreamDestroy(h->side_stream); h->side_stream = nullptr; }
  if (h->side_ev) { (void)hipEventDestroy(h->side_ev); h->side_ev = nullptr; }
  if (h->chain_fork_ev) { (void)hipEventDestroy(h->chain_fork_ev); h->chain_fork_ev = nullptr; }
  for (int c = 0; c < 3; c++) {
    if (h->chain_stream[c]) { (void)hipStreamSynchronize(h->chain_stream[c]); (void)hipStreamDestroy(h->chain_stream[c]); h->chain_stream[c] = nullptr; }
    if (h->chain_ev[c]) { (void)hipEventDestroy(h->chain_ev[c]); h->chain_ev[c] = nullptr; }
  }
  h->n_chain_streams = 0;
  if (h->side_fork_ev) { (void)hipEventDestroy(h->side_fork_ev); h->side_fork_ev = nullptr; }
  if (h->ev0) { (void)hipEventDestroy(h->ev0); h->ev0 = nullptr; }
  if (h->ev1) { (void)hipEventDestroy(h->ev1); h->ev1 = nullptr; }
  if (h->own_stream && h->stream) { (void)hipStreamDestroy(h->stream); h->stream = nullptr; }
}

int lsr_destroy(lsr_handle h) {
  if (!h) return LSR_OK;
  DeviceGuard guard(h->device);
  for (auto& w : h->aux)   // the workers first: their launches may still read buffers the handle owns
    if (w) { release_handle_streams(w.get()); w->target.reset(); }
  release_handle_streams(h);
  h->target.reset();
  delete h;
  return LSR_OK;
}

int lsr_set_f64(lsr_handle h, int key, double v) {
  LSR_CHECK_HANDLE(h);
  switch (key) {
    case LSR_RESOLUTION:
      if (!(v > 0)) { set_last_error("resolution must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
      h->ndt.resolution = v;  // pclomp rebuilds the grid lazily when the resolution changes
      return LSR_OK;
    case LSR_TRANSFORMATION_EPSILON: h->ndt.trans_eps = v; h->gicp.trans_eps = v; return LSR_OK;
    case LSR_STEP_SIZE: h->ndt.step_size = v; return LSR_OK;
    case LSR_OUTLIER_RATIO: h->ndt.outlier_ratio = v; return LSR_OK;
    case LSR_MAX_CORRESPONDENCE_DISTANCE: h->gicp.max_corr_dist = v; return LSR_OK;
    case LSR_ROTATION_EPSILON: h->gicp.rot_eps = v; return LSR_OK;
    case LSR_EUCLIDEAN_FITNESS_EPSILON: h->euclidean_fitness_eps = v; return LSR_OK;
    case LSR_GICP_EPSILON: h->gicp.gicp_eps = v; h->source_cov_valid = false; if (h->target) h->target->has_cov = false; return LSR_OK;
    default: set_last_error("unknown f64 key"); return LSR_ERR_INVALID_ARGUMENT;
  }
}

int lsr_get_f64(lsr_handle h, int key, double* v) {
  LSR_CHECK_HANDLE(h);
  if (!v) return LSR_ERR_INVALID_ARGUMENT;
  switch (key) {
    case LSR_RESOLUTION: *v = h->ndt.resolution; return LSR_OK;
    case LSR_TRANSFORMATION_EPSILON: *v = (h->method == LSR_METHOD_NDT) ? h->ndt.trans_eps : h->gicp.trans_eps; return LSR_OK;
    case LSR_STEP_SIZE: *v = h->ndt.step_size; return LSR_OK;
    case LSR_OUTLIER_RATIO: *v = h->ndt.outlier_ratio; return LSR_OK;
    case LSR_MAX_CORRESPONDENCE_DISTANCE: *v = h->gicp.max_corr_dist; return LSR_OK;
    case LSR_ROTATION_EPSILON: *v = h->gicp.rot_eps; return LSR_OK;
    case LSR_EUCLIDEAN_FITNESS_EPSILON: *v = h->euclidean_fitness_eps; return LSR_OK;
    case LSR_GICP_EPSILON: *v = h->gicp.gicp_eps; return LSR_OK;
    case LSR_MAP_ASSEMBLY_MS: *v = h->map_ms; return LSR_OK;
    case LSR_POSE_GRAPH_BAND_SOLVE_MS: *v = h->pose_graph.stage_ms[0]; return LSR_OK;
    case LSR_POSE_GRAPH_DENSE_MS: *v = h->pose_graph.stage_ms[1]; return LSR_OK;
    case LSR_POSE_GRAPH_COMBINE_MS: *v = h->pose_graph.stage_ms[2]; return LSR_OK;
    case LSR_PCD_FORMAT_MS: *v = h->pcd.format_ms; return LSR_OK;
    case LSR_PCD_PARSE_MS: *v = h->pcd_read.parse_ms; return LSR_OK;
    case LSR_PCD_INFLATE_MS: *v = h->pcd_read.inflate_ms; return LSR_OK;
    case LSR_PCD_DEFLATE_MS: *v = h->pcd_deflate.deflate_ms; return LSR_OK;
    case LSR_MAP_FILTER_BBOX_MS: case LSR_MAP_FILTER_KEY_MS: case LSR_MAP_FILTER_SORT_MS: case LSR_MAP_FILTER_RUNS_MS:
    case LSR_MAP_FILTER_CENTROID_MS: case LSR_MAP_FILTER_WRITE_MS:
      *v = h->map_filter.ms[key - LSR_MAP_FILTER_BBOX_MS]; return LSR_OK;
    case LSR_MAP_WINDOW_MS: *v = h->map_window.ms; return LSR_OK;
    case LSR_POSE_SEARCH_MS: *v = h->pose_search.ms; return LSR_OK;
    case LSR_SCAN_CONTEXT_BUILD_MS: *v = h->scan_context.build_ms; return LSR_OK;
    case LSR_SCAN_CONTEXT_MATCH_MS: *v = h->scan_context.match_ms; return LSR_OK;
    case LSR_DEPTH_IMAGES_MS: *v = h->visibility.images_ms; return LSR_OK;
    case LSR_VISIBILITY_MS: *v = h->visibility.votes_ms; return LSR_OK;
    default: set_last_error("unknown f64 key"); return LSR_ERR_INVALID_ARGUMENT;
  }
}

int lsr_set_i32(lsr_handle h, int key, int v) {
  LSR_CHECK_HANDLE(h);
  switch (key) {
    case LSR_MAX_ITERATIONS:
      if (v < 0) { set_last_error("max_iterations must be >= 0"); return LSR_ERR_INVALID_ARGUMENT; }
      h->ndt.max_iterations = v; h->gicp.max_iterations = v; return LSR_OK;
    case LSR_NEIGHBORHOOD:
      if (v < LSR_KDTREE || v > LSR_DIRECT1) { set_last_error("unknown neighbourhood"); return LSR_ERR_INVALID_ARGUMENT; }
      h->ndt.neighborhood = v; return LSR_OK;
    case LSR_NUM_THREADS: h->num_threads = v; return LSR_OK;          // CPU-only hint: accepted, ignored
    case LSR_K_CORRESPONDENCES:
      if (v < 3 || v > GICP_MAX_K) { set_last_error("k_correspondences out of range"); return LSR_ERR_INVALID_ARGUMENT; }
      h->gicp.k = v; h->source_cov_valid = false; if (h->target) h->target->has_cov = false; return LSR_OK;
    case LSR_MAX_INNER_ITERATIONS: h->gicp.max_inner = v; return LSR_OK;
    case LSR_GICP_SOLVER:
      if (v != LSR_GICP_GAUSS_NEWTON && v != LSR_GICP_BFGS) { set_last_error("unknown GICP solver"); return LSR_ERR_INVALID_ARGUMENT; }
      h->gicp.solver = v; return LSR_OK;
    case LSR_RANSAC_ITERATIONS: h->ransac_iterations = v; return LSR_OK;  // no effect on NDT/GICP maths
    case LSR_HESSIAN_D1_SIGN: h->ndt.d1_sign = (v >= 0) ? 1 : -1; return LSR_OK;
    case LSR_PROFILE: h->profile = v ? 1 : 0; return LSR_OK;
    case LSR_NDT_WORKGROUP:
      if (v == 256) {   // rounds 1-3: the one-lane kernel's workgroup size (then the default).  That kernel is gone: automatic, said once.
        static bool warned = false;
        if (!warned) { warned = true; fprintf(stderr, "[lidarslam_reg] LSR_NDT_WORKGROUP = 256 is a geometry of an earlier kernel: using the automatic choice (0)\n"); }
        h->ndt_threads = 0; return LSR_OK;
      }
      if (v != 0 && v != 64 && v != 128 && v != 512 && v != 1024) { set_last_error("NDT workgroup key must be 0 (auto), 64 / 128 (quad kernel: points) or 512 / 1024 (lane kernel: threads)"); return LSR_ERR_INVALID_ARGUMENT; }
      h->ndt_threads = v; return LSR_OK;
    case LSR_NDT_TABLE_MODE:
      if (v < -1 || v > 2) { set_last_error("NDT table mode must be in -1 .. 2: -1 (auto), 0 dense, 1 compact, 2 LDS"); return LSR_ERR_INVALID_ARGUMENT; }
      h->ndt_table_mode = v; return LSR_OK;
    case LSR_NDT_QUAD:
      if (v < -1 || v > 1) { set_last_error("NDT quad mode must be -1 (auto), 0 or 1"); return LSR_ERR_INVALID_ARGUMENT; }
      h->ndt_quad = v; return LSR_OK;
    case LSR_NDT_SPLIT:
      if (v < -1 || v > 1) { set_last_error("NDT split mode must be -1 (auto), 0 or 1"); return LSR_ERR_INVALID_ARGUMENT; }
      h->ndt_split = v; return LSR_OK;
    case LSR_GRID_BUILDER:
      if (v < 0 || v > 1) { set_last_error("grid builder must be 0 (auto) or 1 (radix-sort builder)"); return LSR_ERR_INVALID_ARGUMENT; }
      h->scratch.force_sort_path = (v == 1);
      if (h->target) h->target->has_grid = h->target->has_centroids = false;
      return LSR_OK;
    case LSR_WAIT_MODE:
      if (v < 0 || v > 2) { set_last_error("wait mode must be 0 (spin), 1 (yield) or 2 (sleep)"); return LSR_ERR_INVALID_ARGUMENT; }
      h->scratch.wait_mode = v; return LSR_OK;
    case LSR_PCD_PIECE_RECORDS:
      if (v < PCD_PIECE_MIN || v > PCD_PIECE_MAX) { set_last_error("PCD piece size must be in 64 .. 1 << 22 records"); return LSR_ERR_INVALID_ARGUMENT; }
      h->pcd.piece_records = v; return LSR_OK;
    case LSR_PCD_READ_PIECE_BYTES:
      if (v < PCDR_PIECE_MIN || v > PCDR_PIECE_MAX) { set_last_error("PCD read piece size must be in 2048 .. 1 << 28 bytes"); return LSR_ERR_INVALID_ARGUMENT; }
      h->pcd_read.piece_bytes = v; return LSR_OK;
    case LSR_PCD_READ_COMPRESSED:
      if (v != 0 && v != 1) { set_last_error("LSR_PCD_READ_COMPRESSED must be 0 or 1"); return LSR_ERR_INVALID_ARGUMENT; }
      h->pcd_read.read_compressed = v; return LSR_OK;
    case LSR_VISIBILITY_PIECE_BYTES:
      if (v < VIS_PIECE_MIN || v > VIS_PIECE_MAX) { set_last_error("visibility piece size must be in 256 .. 1 << 30 bytes"); return LSR_ERR_INVALID_ARGUMENT; }
      h->visibility.piece_bytes = v; return LSR_OK;
    default: set_last_error("unknown i32 key"); return LSR_ERR_INVALID_ARGUMENT;
  }
}

int lsr_get_i32(lsr_handle h, int key, int* v) {
  LSR_CHECK_HANDLE(h);
  if (!v) return LSR_ERR_INVALID_ARGUMENT;
  switch (key) {
    case LSR_MAX_ITERATIONS: *v = (h->method == LSR_METHOD_NDT) ? h->ndt.max_iterations : h->gicp.max_iterations; return LSR_OK;
    case LSR_NEIGHBORHOOD: *v = h->ndt.neighborhood; return LSR_OK;
    case LSR_NUM_THREADS: *v = h->num_threads; return LSR_OK;
    case LSR_K_CORRESPONDENCES: *v = h->gicp.k; return LSR_OK;
    case LSR_MAX_INNER_ITERATIONS: *v = h->gicp.max_inner; return LSR_OK;
    case LSR_GICP_SOLVER: *v = h->gicp.solver; return LSR_OK;
    case LSR_RANSAC_ITERATIONS: *v = h->ransac_iterations; return LSR_OK;
    case LSR_HESSIAN_D1_SIGN: *v = h->ndt.d1_sign; return LSR_OK;
    case LSR_PROFILE: *v = h->profile; return LSR_OK;
    case LSR_NDT_WORKGROUP: *v = h->ndt_threads; return LSR_OK;
    case LSR_NDT_TABLE_MODE: *v = h->ndt_table_mode; return LSR_OK;
    case LSR_NDT_QUAD: *v = h->ndt_quad; return LSR_OK;
    case LSR_NDT_SPLIT: *v = h->ndt_split; return LSR_OK;
    case LSR_GRID_BUILDER: *v = h->scratch.force_sort_path ? 1 : 0; return LSR_OK;
    case LSR_WAIT_MODE: *v = h->scratch.wait_mode; return LSR_OK;
    case LSR_VOXEL_FILTER_FORM: *v = h->scratch.vg_form; return LSR_OK;
    case LSR_MAP_ASSEMBLY_FORM: *v = h->map_form; return LSR_OK;
    case LSR_MAP_FILTER_KEY_BITS: *v = h->map_filter.key_bits; return LSR_OK;
    case LSR_PCD_PIECE_RECORDS: *v = h->pcd.piece_records; return LSR_OK;
    case LSR_PCD_READ_PIECE_BYTES: *v = h->pcd_read.piece_bytes; return LSR_OK;
    case LSR_VISIBILITY_PIECE_BYTES: *v = h->visibility.piece_bytes; return LSR_OK;
    case LSR_PCD_READ_COMPRESSED: *v = h->pcd_read.read_compressed; return LSR_OK;
    case LSR_PCD_UNRESOLVED_TOKENS: *v = h->pcd_read.unresolved; return LSR_OK;
    case LSR_TARGET_PREPARED:
      if (h->method == LSR_METHOD_GICP) *v = gicp_target_prepared(h) ? 1 : 0;
      else *v = (h->target && h->target->n > 0 && h->target->has_grid && h->target->grid_leaf == (float)h->ndt.resolution &&
                 (h->ndt.neighborhood != LSR_KDTREE || h->target->has_centroids || h->target->grid.ncells == 0)) ? 1 : 0;
      return LSR_OK;
    default: set_last_error("unknown i32 key"); return LSR_ERR_INVALID_ARGUMENT;
  }
}

int lsr_wait_stream(lsr_handle h, void* producer_stream) {
  LSR_CHECK_HANDLE(h);
  if ((hipStream_t)producer_stream == h->stream) return LSR_OK;  // same stream: already ordered
  LSR_HIP(hipEventRecord(h->ev0, (hipStream_t)producer_stream));
  LSR_HIP(hipStreamWaitEvent(h->stream, h->ev0, 0));
  return LSR_OK;
}

int lsr_share_target(lsr_handle h, lsr_handle owner) {
  LSR_CHECK_HANDLE(h);
  if (!owner || !owner->target) { set_last_error("owner has no target"); return LSR_ERR_NO_TARGET; }
  if (owner->device != h->device) { set_last_error("handles live on different devices"); return LSR_ERR_INVALID_ARGUMENT; }
  // The frontend's hand-over (scanmatcher_component.cpp:298-320: the target the map thread assembled is taken over at the start of a
  // callback): the target h held until now goes back to the owner as its SPARE when nobody else holds it, so that the owner's next
  // setInputTarget recycles its buffers (fresh_target) instead of allocating while h still reads the new one — two TargetData
  // objects then alternate for the life of the node, no hipMalloc / hipFree per map update.  The caller must not be inside another
  // call on `owner` at this moment (the hand-over happens after the map thread's job has finished).
  std::shared_ptr<TargetData> old = h->target;
  h->target = owner->target;
  if (old && old != owner->target) {
    if (h->spare_target == old) h->spare_target.reset();
    if (old.use_count() == 1 && (!owner->spare_target || owner->spare_target == owner->target)) owner->spare_target = old;
  }
  return LSR_OK;
}

int lsr_align_batch(lsr_handle* handles, int batch, const float* guesses, float* finals, lsr_result* results) {
  if (!handles || batch <= 0) { set_last_error("empty batch"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_batch_members(handles, batch, true, false);
  if (st) return st;
  lsr_handle lead = handles[0];
  LSR_CHECK_HANDLE(lead);
  // NDT: the shared chain's stream is ordered after whatever the members still have in flight (align_ndt_batch), no host wait
  if (lead->method == LSR_METHOD_NDT) return align_ndt_batch(handles, batch, guesses, finals, results);
  // GICP: every registration is a chain of small dependent launches on its own object's stream; the chains of the batch are fed
  // side by side by one host loop (an object may appear only once: a chain owns its object's workspace and mailbox)
  if ((st = check_batch_members(handles, batch, true, true))) return st;
  for (int b = 1; b < batch; b++)
    if (settle_dep(handles[b])) return LSR_ERR_HIP;   // each member runs on its own stream
  return gicp_align_batch(handles, batch, guesses, finals, results);
}

// registration_->align() followed by registration_->getFitnessScore() for every candidate of a set
// (graph_based_slam_component.cpp:230-231): what lsr_align_batch + lsr_get_fitness_score_batch return, with the searches of the
// members that finish early running under the launch chain of the others.
int lsr_align_fitness_batch(lsr_handle* handles, int batch, const float* guesses, float* finals, lsr_result* results, double max_range,
                            double* fitness) {
  if (!handles || batch <= 0 || !fitness) { set_last_error("empty batch"); return LSR_ERR_INVALID_ARGUMENT; }
  // an object can hold ONE result: a handle listed twice would be scored at whichever of its poses was written last
  int st = check_batch_members(handles, batch, true, true);
  if (st) return st;
  lsr_handle lead = handles[0];
  LSR_CHECK_HANDLE(lead);
  if (lead->method != LSR_METHOD_NDT) {
    st = lsr_align_batch(handles, batch, guesses, finals, results);
    return st ? st : lsr_get_fitness_score_batch(handles, batch, max_range, fitness);
  }
  if ((st = align_ndt_batch(handles, batch, guesses, finals, results, fitness, max_range))) return st;
  std::vector<lsr_handle> rest;
  std::vector<int> where;
  for (int b = 0; b < batch; b++)
    if (fitness[b] != fitness[b]) { rest.push_back(handles[b]); where.push_back(b); }   // not served under the chain
  if (!rest.empty()) {
    std::vector<double> v(rest.size());
    if ((st = lsr_get_fitness_score_batch(rest.data(), (int)rest.size(), max_range, v.data()))) return st;
    for (size_t k = 0; k < rest.size(); k++) fitness[where[k]] = v[k];
  }
  return LSR_OK;
}

int lsr_align(lsr_handle h, const float* guess, float* final_transformation, lsr_result* result, void* output_pts,
              size_t out_stride_bytes) {
  LSR_CHECK_HANDLE(h);
  int st;
  if (h->method == LSR_METHOD_NDT) {
    lsr_handle hs[1] = {h};
    st = align_ndt_batch(hs, 1, guess, final_transformation, result);
  } else {
    st = gicp_align(h, guess, final_transformation, result);
  }
  if (st) return st;
  if (output_pts) {
    if ((st = arg_error(check_stride_arg(out_stride_bytes, "out_stride_bytes")))) return st;
    // PCL's align() first copies the source records into `output` and then overwrites x, y, z with the transformed
    // coordinates; every other field (intensity, ...) stays.  Same here: only the 12 xyz bytes of each record are written,
    // whatever the caller put in the rest of the record survives (12 bytes per point cross PCIe, packed).
    const size_t n = h->source.n;
    if ((st = h->out_xyz.reserve(n * 3))) return st;
    if ((st = stage_out(h, h->out_xyz.p, n * 12, false, [&](unsigned char* d) -> int {
          LSR_HIP(hipMemcpyAsync(h->d_T16.p, h->final_T, 16 * sizeof(float), hipMemcpyHostToDevice, h->stream));
          return transform_to_strided(h->source, h->d_T16.p, d, 12, h->stream);
        })))
      return st;
    unsigned char* o = static_cast<unsigned char*>(output_pts);
    for (size_t i = 0; i < n; i++) std::memcpy(o + i * out_stride_bytes, h->out_xyz.p + 3 * i, 12);
  }
  return LSR_OK;
}

int lsr_get_final_transformation(lsr_handle h, float* out16) {
  LSR_CHECK_HANDLE(h);
  if (!out16) return LSR_ERR_INVALID_ARGUMENT;
  std::memcpy(out16, h->final_T, sizeof(float) * 16);
  return LSR_OK;
}

int lsr_has_converged(lsr_handle h, int* out) {
  LSR_CHECK_HANDLE(h);
  if (!out) return LSR_ERR_INVALID_ARGUMENT;
  *out = h->converged;
  return LSR_OK;
}

int lsr_get_fitness_score(lsr_handle h, double max_range, double* out) {
  LSR_CHECK_HANDLE(h);
  if (!out) return LSR_ERR_INVALID_ARGUMENT;
  if (!h->target || h->target->n == 0) { set_last_error("getFitnessScore before setInputTarget"); return LSR_ERR_NO_TARGET; }
  if (!h->has_source) { set_last_error("getFitnessScore before setInputSource"); return LSR_ERR_NO_SOURCE; }
  int st = ensure_target_hash(h);
  if (st) return st;
  return nn_fitness_score(h->source, h->final_T, h->target->hash, max_range, out, h->scratch, h->d_T16, h->stream);
}

// getFitnessScore for a set of candidates (graph_based_slam_component.cpp:231 per candidate): every search + reduction is
// enqueued on its object's stream before the first result is waited for.
int lsr_get_fitness_score_batch(lsr_handle* handles, int count, double max_range, double* out) {
  if (count < 0 || (count > 0 && (!handles || !out))) { set_last_error("bad batch arguments"); return LSR_ERR_INVALID_ARGUMENT; }
  int st;
  if (count == 0) return LSR_OK;
  for (int b = 0; b < count; b++) {
    // member by member, so that the first member at fault decides the status; an object's scratch, mailbox and transform buffer
    // hold ONE reduction in flight
    if ((st = check_batch_member(handles, b, false, true))) return st;
    lsr_handle h = handles[b];
    if (!h->target || h->target->n == 0) { set_last_error("getFitnessScore before setInputTarget"); return LSR_ERR_NO_TARGET; }
    if (!h->has_source) { set_last_error("getFitnessScore before setInputSource"); return LSR_ERR_NO_SOURCE; }
  }
  DeviceGuard guard(handles[0]->device);
  if (!guard.ok) { set_last_error("hipSetDevice failed"); return LSR_ERR_HIP; }
  // Members whose neighbour grid can be refined from their voxel grid (NDT, counting-sort builder) are served by GROUP launches
  // on the first member's stream: one launch for the grids, three per group for search + reduction.  The others keep the
  // staged per-member path on their own streams.
  hipStream_t lead_stream = handles[0]->stream;
  std::vector<int> grouped, single;
  std::vector<const VoxelGridDev*> vgs;
  std::vector<HashGridDev*> hgs;
  for (int b = 0; b < count; b++) {
    lsr_handle h = handles[b];
    if (hash_from_grid_possible(h) && !target_is_shared(h)) {
      grouped.push_back(b);
      if (!h->target->has_hash) { vgs.push_back(&h->target->grid); hgs.push_back(&h->target->hash); }
      if ((st = order_lead_after(lead_stream, h))) return st;   // the member's source upload / anything else in flight on its own stream
    } else {
      single.push_back(b);
    }
  }
  int first_error = LSR_OK;
  if (!vgs.empty()) {
    if ((st = nn_build_hash_from_grids(vgs.data(), hgs.data(), (int)vgs.size(), lead_stream))) return st;
    for (int b : grouped) handles[b]->target->has_hash = true;
  }
  if (!grouped.empty()) {
    std::vector<FitJob> jobs;
    for (int b : grouped) jobs.push_back(FitJob{&handles[b]->source, handles[b]->final_T, &handles[b]->target->hash, max_range, &handles[b]->scratch});
    if ((st = nn_fitness_begin_group(jobs.data(), (int)jobs.size(), lead_stream))) return st;
  }
  int begun = 0;
  for (; begun < (int)single.size(); begun++) {
    lsr_handle h = handles[single[begun]];
    if ((st = settle_dep(h))) break;   // used on its own stream here
    if ((st = ensure_target_hash(h))) break;
    if ((st = nn_fitness_begin(h->source, h->final_T, h->target->hash, max_range, h->scratch, h->d_T16, h->stream))) break;
  }
  if (begun < (int)single.size()) first_error = st;
  for (int b : grouped) {   // collect what was enqueued even after an error: no reduction stays in flight
    double v = 0;
    st = nn_fitness_end(handles[b]->scratch, lead_stream, &v);
    if (st && !first_error) first_error = st;
    out[b] = v;
  }
  for (int k = 0; k < begun; k++) {
    const int b = single[k];
    double v = 0;
    st = nn_fitness_end(handles[b]->scratch, handles[b]->stream, &v);
    if (st && !first_error) first_error = st;
    out[b] = v;
  }
  return first_error;
}

int lsr_pose_graph_edges(const double* poses16, int n, int num_adjacent, lsr_pose_edge* out, size_t capacity, size_t* n_out) {
  if (!poses16 || !n_out || n < 1 || num_adjacent < 1) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  return pose_graph_adjacent_edges(poses16, n, num_adjacent, out, capacity, n_out);   // allocates nothing
}

// both pose-graph entries: the arguments checked against `max_offband` edges outside the band (named `limit_name` in the refusal), the
// trivial graphs served, then the optimiser
static int optimize_pose_graph_checked(lsr_handle h, const double* poses16_in, int n, const lsr_pose_edge* edges, int n_edges,
                                       const lsr_pose_graph_params* params, double* poses16_out, lsr_pose_graph_result* result,
                                       lsr_pose_graph_trace* trace, int max_offband, const char* limit_name) {
  LSR_CHECK_HANDLE(h);
  if (!poses16_in || !poses16_out || !result || n < 1 || n_edges < 0 || (n_edges > 0 && !edges)) {
    set_last_error("bad argument");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  const int max_iterations = params ? params->max_iterations : 10, band = params ? params->band : 5;
  if (n > PG_MAX_VERTICES || n_edges > PG_MAX_EDGES || max_iterations < 1 || band < 1 || band > PG_MAX_BAND) {
    set_last_error("pose graph: vertices, edges, max_iterations or band outside the documented limits");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  int off_band = 0;
  for (int k = 0; k < n_edges; k++) {
    const int a = edges[k].from, b = edges[k].to;
    if (a < 0 || b < 0 || a >= n || b >= n || a == b) {
      set_last_error("pose graph: edge " + std::to_string(k) + " joins a vertex to itself or names one that does not exist");
      return LSR_ERR_INVALID_ARGUMENT;
    }
    if (a != 0 && b != 0 && std::abs(a - b) > band) off_band++;
  }
  if (off_band > max_offband) {
    set_last_error(std::string("pose graph: more than ") + limit_name + " edges outside the band");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  if (n == 1 || n_edges == 0) {
    if (poses16_out != poses16_in) std::memmove(poses16_out, poses16_in, sizeof(double) * 16 * (size_t)n);
    std::memset(result, 0, sizeof(*result));
    return LSR_OK;
  }
  // the host side of the graph lives in std::vectors (up to 2^20 edges): nothing they throw crosses the C ABI
  try {
    h->pose_graph.profile = h->profile != 0;
    return pose_graph_optimize(h->pose_graph, poses16_in, n, edges, n_edges, max_iterations, band, max_offband, poses16_out, result, trace,
                               h->stream, h->ev0, h->ev1);
  } catch (const std::exception& e) {
    set_last_error(std::string("pose graph: host allocation failed: ") + e.what());
    return LSR_ERR_HIP;
  }
}

int lsr_optimize_pose_graph(lsr_handle h, const double* poses16_in, int n, const lsr_pose_edge* edges, int n_edges,
                            const lsr_pose_graph_params* params, double* poses16_out, lsr_pose_graph_result* result,
                            lsr_pose_graph_trace* trace) {
  return optimize_pose_graph_checked(h, poses16_in, n, edges, n_edges, params, poses16_out, result, trace, PG_MAX_OFFBAND,
                                     "LSR_POSE_GRAPH_MAX_OFFBAND_EDGES");
}

int lsr_optimize_pose_graph_long(lsr_handle h, const double* poses16_in, int n, const lsr_pose_edge* edges, int n_edges,
                                 const lsr_pose_graph_params* params, double* poses16_out, lsr_pose_graph_result* result,
                                 lsr_pose_graph_trace* trace) {
  return optimize_pose_graph_checked(h, poses16_in, n, edges, n_edges, params, poses16_out, result, trace, PG_LONG_MAX_OFFBAND,
                                     "LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES");
}

int lsr_nearest_neighbors(lsr_handle h, const float* T16, int32_t* idx, float* d2) {
  LSR_CHECK_HANDLE(h);
  if (!h->target || h->target->n == 0) return LSR_ERR_NO_TARGET;
  if (!h->has_source) return LSR_ERR_NO_SOURCE;
  int st = ensure_target_hash(h);
  if (st) return st;
  float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  return nn_search_host(h->source, T16 ? T16 : I16, h->target->hash, idx, d2, h->scratch, h->d_T16, h->stream);
}

int lsr_gicp_covariances(lsr_handle h, int which, double* cov) {
  LSR_CHECK_HANDLE(h);
  if (!cov) return LSR_ERR_INVALID_ARGUMENT;
  return gicp_get_covariances(h, which, cov);
}

int lsr_gicp_linearize(lsr_handle h, const float* guess16, const float* trans16, int use_seeds, float* out, int32_t* nn_idx,
                       int32_t* valid, double* M6, float* q, double* x6, float* T12, double* dR27, int32_t* m, double* sums28) {
  LSR_CHECK_HANDLE(h);
  if (h->method != LSR_METHOD_GICP) { set_last_error("lsr_gicp_linearize on an NDT object"); return LSR_ERR_INVALID_ARGUMENT; }
  const GicpLinearizeOut o{out, nn_idx, valid, M6, q, x6, T12, dR27, m, sums28};
  return gicp_linearize(h, guess16, trans16, use_seeds, o);
}

int lsr_gicp_bfgs_trace(lsr_handle h, const float* guess16, const float* trans16, int32_t capacity, double* x6, double* f, double* g6,
                        int32_t* inner, int32_t* n_evals, int32_t* n_inner, int32_t* reason, double* x6_final, int32_t* m) {
  LSR_CHECK_HANDLE(h);
  if (h->method != LSR_METHOD_GICP) { set_last_error("lsr_gicp_bfgs_trace on an NDT object"); return LSR_ERR_INVALID_ARGUMENT; }
  if (capacity < 0) { set_last_error("capacity must be >= 0"); return LSR_ERR_INVALID_ARGUMENT; }
  const GicpBfgsTraceOut o{x6, f, g6, inner, n_evals, n_inner, reason, x6_final, m};
  return gicp_bfgs_trace(h, guess16, trans16, capacity, o);
}

int lsr_get_profile(lsr_handle h, lsr_profile* out, int reset) {
  LSR_CHECK_HANDLE(h);
  if (out) *out = h->prof;
  if (reset) h->prof = lsr_profile{0, 0, 0, 0};
  return LSR_OK;
}

}  // extern "C"

// setInputTarget / setInputSource in all their forms, the voxel filter entries and the PointCloud2 codec entries of the C ABI
// (include/lidarslam_reg.h).  Host-side orchestration only: uploads, the launches of cloud_codec / grid_build, the object's state.
#include <algorithm>
#include <cstdlib>

#include "api_internal.hpp"

using namespace lsr;

namespace {

int upload_cloud(lsr_handle h, const void* pts, size_t stride, size_t n, bool on_device, DeviceCloud& out) {
  int st;
  if ((st = check_stride(stride)) || (st = arg_error(check_records(pts, n, INGEST_RECORD_LIMIT, false, "points")))) return st;
  const void* d_aos = nullptr;
  if ((st = stage_in(h, pts, n * stride, on_device, h->stream, &d_aos))) return st;
  return deinterleave(d_aos, stride, n, out, h->stream);
}

// A PointCloud2 payload (or strided xyz records: a payload without intensity) -> SoA planes through pc2_ingest: ONE launch that also applies
// the frontend's range filter (do_range) and leaves the bounding-box records for what follows
// (tf: the payload is in the sensor frame and is moved into the robot frame as it is read, lsr_set_input_source_pc2_tf)
int ingest_pc2(lsr_handle h, const void* data, size_t n, const lsr_pc2_layout* L, bool on_device, bool do_range, double rmin, double rmax,
               DeviceCloud& out, const SensorTf12* tf = nullptr) {
  int st = arg_error(check_records(data, n, INGEST_RECORD_LIMIT, false, "data"));
  if (st) return st;
  const void* d = nullptr;
  if ((st = stage_in(h, data, n * L->point_step, on_device, h->stream, &d))) return st;
  return pc2_ingest(d, (int)L->point_step, (int)L->offset_x, (int)L->offset_y, (int)L->offset_z, L->offset_intensity, n, do_range, rmin, rmax,
                    out, h->scratch, h->stream, tf);
}

int set_target_impl(lsr_handle h, const void* pts, size_t stride, size_t n, bool on_device) {
  LSR_CHECK_HANDLE(h);
  if (h->method == LSR_METHOD_NDT) {
    // pclomp::NDT::setInputTarget -> init(): the voxel-covariance grid is built right here, as a set of one — de-interleave and
    // bounding box in one launch, the group kernels of a candidate set (661k-point submap: 104 -> 94 us); grid_builder = 1 takes the
    // general builder from there (ndt_grid_geometry)
    lsr_handle one[1] = {h};
    const void* cloud[1] = {pts};
    const size_t count[1] = {n};
    return lsr_set_input_target_batch(one, 1, cloud, count, stride, on_device ? 1 : 0);
  }
  auto t = fresh_target(h);
  int st = upload_cloud(h, pts, stride, n, on_device, t->cloud);
  if (st) return st;
  t->n = n;
  h->target = t;
  // GICP: target covariances are computed lazily in align() by the reference; the NN structure is
  // what setInputTarget pays for (kd-tree there, hash grid here).
  st = ensure_target_hash(h);
  if (st) { h->target.reset(); return st; }
  LSR_HIP(hipStreamSynchronize(h->stream));
  return LSR_OK;
}

int set_source_impl(lsr_handle h, const void* pts, size_t stride, size_t n, bool on_device) {
  LSR_CHECK_HANDLE(h);
  int st = upload_cloud(h, pts, stride, n, on_device, h->source);
  if (st) return st;
  h->has_source = true;
  h->source_cov_valid = false;
  if (!on_device) LSR_HIP(hipStreamSynchronize(h->stream));  // the caller may reuse its host buffer
  return LSR_OK;
}

// How the filtered-source entries return.  voxel_grid_filter has polled a mailbox word written by a kernel that runs BEHIND the pass
// that read the caller's buffer (the run count; the bounding box when no point is finite): the caller's buffer — host or device — has
// been consumed and may be reused.  What can still be running is the centroid launch, which reads and writes buffers the object owns;
// everything that uses the source afterwards is enqueued on the object's stream (or orders itself behind it: order_lead_after), so
// the call does not wait for it — the align that follows in the frontend loop starts under it (env LSR_SOURCE_SYNC=1: wait, as until
// round 5).
int finish_source_call(lsr_handle h) {
  static const bool wait = [] { const char* e = std::getenv("LSR_SOURCE_SYNC"); return e && e[0] == '1'; }();
  if (wait) LSR_HIP(hipStreamSynchronize(h->stream));
  return LSR_OK;
}
// the filtered cloud in h->source is the object's input source from here on
int accept_source(lsr_handle h, size_t* n_out) {
  h->has_source = true;
  h->source_cov_valid = false;
  if (n_out) *n_out = h->source.n;
  return finish_source_call(h);
}

// ---- N4: PointCloud2 codec ---------------------------------------------------------------------
// payload -> SoA planes (+ intensity) on the device
// SoA planes -> host payload (bytes outside the four fields are zero)
int write_pc2_host(lsr_handle h, const DeviceCloud& cloud, void* out_data, size_t capacity, const lsr_pc2_layout* L, size_t* n_out) {
  *n_out = cloud.n;
  if (cloud.n > capacity) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
  if (cloud.n == 0) return LSR_OK;
  return stage_out(h, out_data, cloud.n * L->point_step, true, [&](unsigned char* d) {
    return pc2_write(cloud, d, (int)L->point_step, (int)L->offset_x, (int)L->offset_y, (int)L->offset_z, L->offset_intensity, h->stream);
  });
}

}  // namespace

// Submap assembly + setInputTarget without a host round trip of the assembled cloud
// (scanmatcher_component.cpp:449-464,307; graph_based_slam_component.cpp:208-227)
// Move every frame by its pose and concatenate them in order into `out` (device SoA).
int lsr::assemble_frames(lsr_handle h, int n_frames, const void* const* frames, const size_t* counts, size_t stride_bytes,
                         const float* poses16, bool on_device, DeviceCloud& out) {
  size_t total = 0, biggest = 0;
  int st = arg_error(check_frame_list(n_frames, frames, counts, stride_bytes, poses16, &total, &biggest));
  if (st) return st;
  if ((st = out.resize(total))) return st;
  if ((st = h->d_poses.reserve((size_t)n_frames * 16))) return st;
  LSR_HIP(hipMemcpyAsync(h->d_poses.p, poses16, sizeof(float) * 16 * n_frames, hipMemcpyHostToDevice, h->stream));
  if (!on_device && (st = h->staging.reserve(biggest * stride_bytes))) return st;
  size_t off = 0;
  for (int f = 0; f < n_frames; f++) {
    const void* d_aos = nullptr;
    if ((st = stage_in_at(h, frames[f], counts[f] * stride_bytes, on_device, h->stream, 0, &d_aos))) return st;
    if ((st = transform_append(d_aos, stride_bytes, counts[f], h->d_poses.p + 16 * f, out, off, h->stream))) return st;
    if (!on_device) LSR_HIP(hipStreamSynchronize(h->stream));  // the staging buffer is reused by the next frame
    off += counts[f];
  }
  // poses16 is caller memory read by an asynchronous copy: it must have landed before we return to the caller
  if (on_device) LSR_HIP(hipStreamSynchronize(h->stream));
  return LSR_OK;
}

extern "C" {

int lsr_set_input_target_frames(lsr_handle h, int n_frames, const void* const* frames, const size_t* counts, size_t stride_bytes,
                                const float* poses16, int on_device) {
  LSR_CHECK_HANDLE(h);
  int st = arg_error(check_frame_list(n_frames, frames, counts, stride_bytes, poses16));   // before the object is touched
  if (st) return st;
  auto t = fresh_target(h);
  st = assemble_frames(h, n_frames, frames, counts, stride_bytes, poses16, on_device != 0, t->cloud);
  if (st) return st;
  t->n = t->cloud.n;
  h->target = t;
  st = (h->method == LSR_METHOD_NDT) ? ensure_ndt_grid(h) : ensure_target_hash(h);
  if (st) { h->target.reset(); return st; }
  LSR_HIP(hipStreamSynchronize(h->stream));
  return LSR_OK;
}

// The GICP branch of a map update (scanmatcher_component.cpp:308-316,448-464): window -> pcl::VoxelGrid -> setInputTarget, in HBM.
// The window is assembled by ONE launch that also leaves its bounding-box records behind (assemble_frames_bbox), so the filter
// behind it starts without a bounding-box pass and, from the object's second update on, without a host wait for the dimensions.
int lsr_set_input_target_frames_filtered(lsr_handle h, int n_frames, const void* const* frames, const size_t* counts, size_t stride_bytes,
                                         const float* poses16, int on_device, float leaf, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (n_out) *n_out = 0;
  h->target.reset();   // on error the object keeps no target
  size_t total = 0;
  int st = arg_error(check_frame_list(n_frames, frames, counts, stride_bytes, poses16, &total));
  if (st) return st;
  if (!(leaf > 0)) { set_last_error("leaf size must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
  if ((st = h->h_frames.reserve((size_t)n_frames))) return st;
  if ((st = h->d_frames.reserve((size_t)n_frames))) return st;
  if (!on_device && (st = h->staging.reserve(total * stride_bytes))) return st;
  std::vector<int> first_slice((size_t)n_frames);
  const int n_slices = frames_slice_count(counts, n_frames, first_slice.data());
  // whatever was enqueued has finished before the call returns: the table, the staged frames and the caller's buffers are free again
  StreamDrain drain{h->stream};
  size_t off = 0;
  for (int f = 0; f < n_frames; f++) {   // host frames are staged back to back and go through the same launch
    FrameSlot& F = h->h_frames.p[f];
    const void* d_frame = nullptr;
    if ((st = stage_in_at(h, frames[f], counts[f] * stride_bytes, on_device != 0, h->stream, off * stride_bytes, &d_frame))) return st;
    F.records = static_cast<const unsigned char*>(d_frame);
    F.count = (int)counts[f];
    F.first_out = (int)off;
    F.first_slice = first_slice[f];
    F.pad = 0;
    std::memcpy(F.T16, poses16 + 16 * (size_t)f, sizeof(float) * 16);
    off += counts[f];
  }
  LSR_HIP(hipMemcpyAsync(h->d_frames.p, h->h_frames.p, sizeof(FrameSlot) * (size_t)n_frames, hipMemcpyHostToDevice, h->stream));
  if ((st = assemble_frames_bbox(h->d_frames.p, n_frames, n_slices, stride_bytes, total, h->raw, h->scratch, h->stream))) return st;
  auto t = fresh_target(h);
  if ((st = voxel_grid_filter(h->raw, leaf, t->cloud, h->scratch, h->stream))) return st;
  t->n = t->cloud.n;
  h->target = t;
  st = (h->method == LSR_METHOD_NDT) ? ensure_ndt_grid(h) : ensure_target_hash(h);
  if (st) { h->target.reset(); return st; }
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (n_out) *n_out = t->n;
  return LSR_OK;
}

// Everything the first align against the current target would still have to build, now (the map thread's object, before the
// hand-over: lsr_share_target then passes a target on that the callback thread's next scan only reads).
int lsr_prepare_target(lsr_handle h) {
  LSR_CHECK_HANDLE(h);
  if (!h->target || h->target->n == 0) { set_last_error("prepare before setInputTarget"); return LSR_ERR_NO_TARGET; }
  if (h->method == LSR_METHOD_GICP) return gicp_prepare_target(h);
  // NDT: setInputTarget built the voxel grid (pclomp's init()), so as a rule nothing is left; a resolution or neighbourhood
  // method set since then is served here as the next align would serve it
  int st = ensure_ndt_grid(h);
  if (st) return st;
  LSR_HIP(hipStreamSynchronize(h->stream));
  return LSR_OK;
}

int lsr_set_input_target(lsr_handle h, const void* pts, size_t stride_bytes, size_t n) {
  return set_target_impl(h, pts, stride_bytes, n, false);
}

// setInputTarget for a set of candidates (graph_based_slam_component.cpp:181-227 runs once per candidate): the same work
// per object as lsr_set_input_target, staged so that the builds overlap on the device — every upload and bounding-box
// pass is enqueued (each on its object's stream) before the first box is waited for, every grid build before the first
// result is read.
int lsr_set_input_target_batch(lsr_handle* handles, int count, const void* const* clouds, const size_t* counts, size_t stride_bytes,
                               int on_device) {
  if (count < 0 || (count > 0 && (!handles || !clouds || !counts))) { set_last_error("bad batch arguments"); return LSR_ERR_INVALID_ARGUMENT; }
  if (count == 0) return LSR_OK;
  int st;
  if ((st = check_batch_members(handles, count, false, true))) return st;
  DeviceGuard guard(handles[0]->device);   // for the whole call (the stages below enqueue on every member's stream)
  if (!guard.ok) { set_last_error("hipSetDevice failed"); return LSR_ERR_HIP; }
  auto fail = [&](int st) {
    for (int b = 0; b < count; b++) {   // nothing half-built stays behind
      (void)hipStreamSynchronize(handles[b]->stream);
      handles[b]->scratch.grid_pending = false;
      handles[b]->scratch.bbox_parts = 0;
      handles[b]->target.reset();
    }
    return st;
  };
  if ((st = check_stride(stride_bytes))) return st;
  // NDT members are built by GROUP launches on the first member's stream (one launch per stage for up to 16 members: a
  // candidate set is bound by the host's launch rate otherwise); GICP members keep their own path and stream.
  hipStream_t lead_stream = handles[0]->stream;
  std::vector<TargetBuildJob> jobs;
  std::vector<int> job_of((size_t)count, -1);
  for (int b = 0; b < count; b++) {   // stage 0: uploads (+ de-interleave and bounding boxes of the NDT members in group launches)
    lsr_handle h = handles[b];
    if ((st = arg_error(check_records(clouds[b], counts[b], INGEST_RECORD_LIMIT, false, "clouds[]")))) return fail(st);
    auto t = fresh_target(h);
    t->n = counts[b];
    h->target = t;
    if (h->method != LSR_METHOD_NDT) {
      if ((st = settle_dep(h))) return fail(st);   // used on its own stream here
      if ((st = upload_cloud(h, clouds[b], stride_bytes, counts[b], on_device != 0, t->cloud))) return fail(st);
      if ((st = cloud_bbox_begin(t->cloud, h->scratch, h->stream))) return fail(st);
      continue;
    }
    if ((st = order_lead_after(lead_stream, h))) return fail(st);   // whatever this member still has in flight on its own stream comes first
    const void* d_aos = nullptr;
    if ((st = stage_in(h, clouds[b], counts[b] * stride_bytes, on_device != 0, lead_stream, &d_aos))) return fail(st);
    job_of[b] = (int)jobs.size();
    jobs.push_back(TargetBuildJob{d_aos, stride_bytes, counts[b], &t->cloud, (float)h->ndt.resolution, &t->grid, &h->scratch, 0});
  }
  if (!jobs.empty() && (st = ndt_targets_ingest(jobs.data(), (int)jobs.size(), lead_stream))) return fail(st);
  // (Round 5 measured forking the neighbour-grid refinement of a small set onto the lead's side stream right after the scatter, under
  // the leaf sums and the host's work between the calls, instead of next to the first launches of the align chain: the refinement and
  // the leaf sums slow each other down — target + source stage of an 8-candidate share 0.44 ms against 0.28 ms, align 0.03-0.05 ms
  // faster, the share 0.14-0.17 ms slower.  Not done.)
  // stage 1: the rest of every build
  if (!jobs.empty() && (st = ndt_targets_build_begin(jobs.data(), (int)jobs.size(), lead_stream))) return fail(st);
  for (int b = 0; b < count; b++)
    if (handles[b]->method != LSR_METHOD_NDT && (st = ensure_target_hash(handles[b]))) return fail(st);
  for (int b = 0; b < count; b++) {   // stage 2: results
    lsr_handle h = handles[b];
    TargetData& t = *h->target;
    if (h->method == LSR_METHOD_NDT) {
      if ((st = ndt_build_grid_end(t.grid, h->scratch, lead_stream))) return fail(st);
      t.has_grid = true;
      t.has_centroids = false;
      t.grid_leaf = (float)h->ndt.resolution;
    } else if (hipStreamSynchronize(h->stream) != hipSuccess) {
      set_last_error("stream error in the target batch");
      return fail(LSR_ERR_HIP);
    }
  }
  if (hipStreamSynchronize(lead_stream) != hipSuccess) { set_last_error("stream error in the target batch"); return fail(LSR_ERR_HIP); }
  return LSR_OK;
}
int lsr_set_input_target_device(lsr_handle h, const void* dev_pts, size_t stride_bytes, size_t n) {
  return set_target_impl(h, dev_pts, stride_bytes, n, true);
}

int lsr_set_input_source(lsr_handle h, const void* pts, size_t stride_bytes, size_t n) {
  return set_source_impl(h, pts, stride_bytes, n, false);
}
int lsr_set_input_source_device(lsr_handle h, const void* dev_pts, size_t stride_bytes, size_t n) {
  return set_source_impl(h, dev_pts, stride_bytes, n, true);
}

// setInputSource of every candidate of a set (graph_based_slam_component.cpp:181 per candidate): the de-interleaves of up to 16
// members share one launch on the first member's stream.
int lsr_set_input_source_batch(lsr_handle* handles, int count, const void* const* clouds, const size_t* counts, size_t stride_bytes,
                               int on_device) {
  if (count < 0 || (count > 0 && (!handles || !clouds || !counts))) { set_last_error("bad batch arguments"); return LSR_ERR_INVALID_ARGUMENT; }
  if (count == 0) return LSR_OK;
  int st;
  if ((st = check_stride(stride_bytes))) return st;
  if ((st = check_batch_members(handles, count, false, true))) return st;
  for (int b = 0; b < count; b++)
    if ((st = arg_error(check_records(clouds[b], counts[b], INGEST_RECORD_LIMIT, false, "clouds[]")))) return st;
  DeviceGuard guard(handles[0]->device);
  if (!guard.ok) { set_last_error("hipSetDevice failed"); return LSR_ERR_HIP; }
  hipStream_t lead_stream = handles[0]->stream;
  std::vector<DeinterleaveJob> jobs((size_t)count);
  // No member may be left claiming a source it never received: the old clouds are being overwritten, so every member loses its
  // source up front and gets it back only when the whole set has been staged and de-interleaved.  On a failure the staging
  // copies already enqueued are drained before returning (the callers may reuse their host buffers).
  for (int b = 0; b < count; b++) { handles[b]->has_source = false; handles[b]->source_cov_valid = false; }
  auto fail = [&](int status) {
    (void)hipStreamSynchronize(lead_stream);
    return status;
  };
  for (int b = 0; b < count; b++) {
    lsr_handle h = handles[b];
    if ((st = order_lead_after(lead_stream, h))) return fail(st);
    const void* d_aos = nullptr;
    if ((st = stage_in(h, clouds[b], counts[b] * stride_bytes, on_device != 0, lead_stream, &d_aos))) return fail(st);
    jobs[b] = DeinterleaveJob{d_aos, stride_bytes, counts[b], &h->source};
  }
  if ((st = deinterleave_group(jobs.data(), count, lead_stream))) return fail(st);
  // every member's own stream continues after the shared launch (its next align / fitness call runs there): deferred — the members
  // remember the event, their streams wait for it when they are next used on their own (handle.hpp: StreamDep)
  if ((st = defer_members_behind(handles[0], handles, count))) return fail(st);
  if (!on_device && hipStreamSynchronize(lead_stream) != hipSuccess) { set_last_error("stream error in the source batch"); return LSR_ERR_HIP; }
  for (int b = 0; b < count; b++) handles[b]->has_source = true;
  return LSR_OK;
}

// pcl::VoxelGrid::filter + registration_->setInputSource, without the cloud leaving HBM
// (scanmatcher_component.cpp:324-329)
int lsr_set_input_source_filtered(lsr_handle h, const void* pts, size_t stride_bytes, size_t n, float leaf, int on_device,
                                  size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!(leaf > 0)) { set_last_error("leaf size must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = upload_cloud(h, pts, stride_bytes, n, on_device != 0, h->raw);
  if (st) return st;
  if ((st = voxel_grid_filter(h->raw, leaf, h->source, h->scratch, h->stream))) return st;
  return accept_source(h, n_out);
}

// The frontend's whole per-scan preprocessing in one call, on the device: min-max range filter
// (scanmatcher_component.cpp:210-218) -> VoxelGrid(vg_size_for_input) (:324-328) -> setInputSource (:329).
int lsr_set_input_source_frontend(lsr_handle h, const void* pts, size_t stride_bytes, size_t n, double scan_min_range,
                                  double scan_max_range, float vg_size_for_input, int on_device, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!(vg_size_for_input > 0)) { set_last_error("leaf size must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = check_stride(stride_bytes);
  if (st) return st;
  // strided xyz records are a PointCloud2 payload without an intensity field: the same one-launch ingest
  const lsr_pc2_layout rec_layout{(uint32_t)stride_bytes, 0u, 4u, 8u, -1};
  if ((st = ingest_pc2(h, pts, n, &rec_layout, on_device != 0, true, scan_min_range, scan_max_range, h->raw))) return st;
  if ((st = voxel_grid_filter(h->raw, vg_size_for_input, h->source, h->scratch, h->stream))) return st;
  return accept_source(h, n_out);
}

// pcl::VoxelGrid::filter as a stand-alone device operation (host in, host out)
int lsr_voxel_grid_filter(lsr_handle h, const void* pts, size_t stride_bytes, size_t n, float leaf, void* out_pts,
                          size_t out_stride_bytes, size_t out_capacity, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  if (!(leaf > 0) || !n_out) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  int st = arg_error(check_stride_arg(out_stride_bytes, "out_stride_bytes"));
  if (st) return st;
  st = upload_cloud(h, pts, stride_bytes, n, false, h->raw);
  if (st) return st;
  if ((st = voxel_grid_filter(h->raw, leaf, h->filtered, h->scratch, h->stream))) return st;
  *n_out = h->filtered.n;
  if (h->filtered.n > out_capacity) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
  if (h->filtered.n == 0) return LSR_OK;
  return stage_out(h, out_pts, h->filtered.n * out_stride_bytes, true,
                   [&](unsigned char* d) { return interleave(h->filtered, d, out_stride_bytes, h->stream); });
}

int lsr_set_input_source_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, double scan_min_range,
                             double scan_max_range, float vg_size_for_input, int on_device, size_t* n_out) {
  return lsr_set_input_source_pc2_tf(h, data, n_points, layout, nullptr, scan_min_range, scan_max_range, vg_size_for_input, on_device, n_out);
}

// the same from a payload in the SENSOR frame (tf2::doTransform, scanmatcher_component.cpp:195, applied as the records are read)
int lsr_set_input_source_pc2_tf(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, const lsr_sensor_transform* tf,
                                double scan_min_range, double scan_max_range, float vg_size_for_input, int on_device, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  int st = check_layout(layout);
  if (st) return st;
  if (!(vg_size_for_input > 0)) { set_last_error("leaf size must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
  SensorTf12 T;
  if (tf && (st = lsr_sensor_transform_matrix(tf, T.m))) return st;
  // payload -> planes (+ sensor -> robot frame) + range filter + bounding-box records in one launch; the voxel filter behind it reads
  // the records on the device
  if ((st = ingest_pc2(h, data, n_points, layout, on_device != 0, true, scan_min_range, scan_max_range, h->raw, tf ? &T : nullptr))) return st;
  if ((st = voxel_grid_filter(h->raw, vg_size_for_input, h->source, h->scratch, h->stream))) return st;
  return accept_source(h, n_out);
}

int lsr_get_source_pc2(lsr_handle h, void* out_data, size_t capacity_points, const lsr_pc2_layout* layout, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  int st = check_layout(layout);
  if (st) return st;
  if (!n_out || (capacity_points > 0 && !out_data)) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if (!h->has_source) { set_last_error("no input source"); return LSR_ERR_NO_SOURCE; }
  return write_pc2_host(h, h->source, out_data, capacity_points, layout, n_out);
}

// the same into a DEVICE buffer (a keyframe kept resident in HBM: what lsr_set_input_target_frames takes with on_device != 0):
// enqueued on the handle's stream, which is synchronised before returning so that any stream may read the records
int lsr_get_source_pc2_device(lsr_handle h, void* d_out, size_t capacity_points, const lsr_pc2_layout* layout, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  int st = check_layout(layout);
  if (st) return st;
  if (!n_out || (capacity_points > 0 && !d_out)) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if (!h->has_source) { set_last_error("no input source"); return LSR_ERR_NO_SOURCE; }
  const DeviceCloud& cloud = h->source;
  *n_out = cloud.n;
  if (cloud.n > capacity_points) { set_last_error("output buffer too small"); return LSR_ERR_INVALID_ARGUMENT; }
  if (cloud.n == 0) return LSR_OK;
  LSR_HIP(hipMemsetAsync(d_out, 0, cloud.n * layout->point_step, h->stream));
  if ((st = pc2_write(cloud, d_out, (int)layout->point_step, (int)layout->offset_x, (int)layout->offset_y, (int)layout->offset_z,
                      layout->offset_intensity, h->stream))) return st;
  LSR_HIP(hipStreamSynchronize(h->stream));
  return LSR_OK;
}

int lsr_voxel_grid_filter_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout, float leaf, void* out_data,
                              size_t capacity_points, const lsr_pc2_layout* out_layout, size_t* n_out) {
  LSR_CHECK_HANDLE(h);
  int st = check_layout(in_layout, "in_layout");
  if (st) return st;
  if ((st = check_layout(out_layout, "out_layout"))) return st;
  if (!(leaf > 0) || !n_out) { set_last_error("bad argument"); return LSR_ERR_INVALID_ARGUMENT; }
  if ((st = ingest_pc2(h, data, n_points, in_layout, false, false, 0.0, 0.0, h->raw))) return st;
  if ((st = voxel_grid_filter(h->raw, leaf, h->filtered, h->scratch, h->stream))) return st;
  return write_pc2_host(h, h->filtered, out_data, capacity_points, out_layout, n_out);
}

}  // extern "C"

// The clouds on their way into and out of the registration object: PointXYZI records or a PointCloud2
// payload -> SoA planes (+ the frontend's range filter and the bounding-box records in one pass), pcl::VoxelGrid (leaf keys with the
// grid dimensions worked out on the device, stable LSD sort, run heads, float centroids in ascending point index), SoA planes ->
// records / PointCloud2 payload, pcl::transformPointCloud into strided records, tf2::doTransform of a raw payload into the robot frame
// (fused into the ingest pass, or records -> records).  Reference call sites:
// scanmatcher_component.cpp:195,201-218,279-284,324-329,443-447.  (Split out of ndt.hip in round 6: same code.)
#include "ndt.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "build_kernels.hpp"
#include "grid_device.hpp"
#include "sort.hpp"
#include "xform_ref.hpp"

namespace lsr {

namespace {

// The same keys with the grid dimensions worked out ON THE DEVICE from the bounding-box records the ingest pass left in device memory
// (pc2_ingest): every workgroup folds the (<= 256) records itself — the arithmetic is voxel_grid_filter's host code: both call
// grid_dims and bits_for of voxel_device.hpp — and workgroup 0 leaves {sentinel, finite points, VG_FLAG_*, key bits} in dims[0..3]
// for the kernels behind the sort.  The host never sees the box: it enqueues key + sort + run heads + centroids without a wait in
// between.
// dims folded from the records of the ingest pass by ALL 256 threads of a workgroup (one barrier inside: box_fold_block's)
struct VgDims { int mb[3], dv[3]; unsigned int sentinel, flags, n_finite; int bits; };
__device__ __forceinline__ VgDims vg_fold_dims(const unsigned long long* __restrict__ parts, int nparts, float inv_leaf, int planned_bits) {
  const int tid = threadIdx.x;
  BoxAcc box;
  if (tid < nparts) {
    const unsigned long long* P = parts + (size_t)tid * 8;
#pragma unroll
    for (int k = 0; k < 3; k++) { box.mn[k] = __uint_as_float((unsigned int)P[k]); box.mx[k] = __uint_as_float((unsigned int)P[3 + k]); }
    box.cnt = (unsigned int)P[6];
  }
  const BoxFolded F = box_fold_block(box);
  VgDims D;
  D.n_finite = F.count();
  for (int k = 0; k < 3; k++) { D.mb[k] = 0; D.dv[k] = 0; }
  D.sentinel = 0u; D.flags = 0u; D.bits = 1;
  if (D.n_finite != 0u) {
    const float lo[3] = {F.lo(0), F.lo(1), F.lo(2)}, hi[3] = {F.hi(0), F.hi(1), F.hi(2)};
    const GridDims G = grid_dims(lo, hi, inv_leaf);
    for (int k = 0; k < 3; k++) { D.mb[k] = G.min_b[k]; D.dv[k] = G.div_b[k]; }
    if (G.volume > (long long)INT32_MAX) D.flags |= VG_FLAG_OVERFLOW;
    D.sentinel = (unsigned int)((long long)D.dv[0] * D.dv[1] * D.dv[2]);
    D.bits = bits_for(D.sentinel);
    if (D.bits > planned_bits) D.flags |= VG_FLAG_REPLAN;
  }
  return D;
}
__device__ __forceinline__ unsigned int vg_key(const VgDims& D, float inv_leaf, float px, float py, float pz) {
  if (D.flags != 0u) return D.sentinel;
  return leaf_key<int>(px, py, pz, inv_leaf, D.mb[0], D.mb[1], D.mb[2], D.dv[0], D.dv[0] * D.dv[1], D.sentinel);
}

__global__ __launch_bounds__(256) void leaf_key_dims_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, int n, float inv_leaf,
                                                            const unsigned long long* __restrict__ parts, int nparts, int planned_bits,
                                                            unsigned int* __restrict__ key, unsigned int* __restrict__ dims) {
  const int tid = threadIdx.x;
  // the point first: its loads are in flight while the records are folded
  const int i = blockIdx.x * 256 + tid;
  const float px = (i < n) ? x[i] : NAN, py = (i < n) ? y[i] : NAN, pz = (i < n) ? z[i] : NAN;
  const VgDims D = vg_fold_dims(parts, nparts, inv_leaf, planned_bits);
  if (blockIdx.x == 0 && tid == 0) { dims[0] = D.sentinel; dims[1] = D.n_finite; dims[2] = D.flags; dims[3] = (unsigned int)D.bits; }
  if (i < n) key[i] = vg_key(D, inv_leaf, px, py, pz);
}

// The same on the sort's 2048-key workgroups, counting the keys' FIRST digit on the way (lsd_first_hist_plan: the table the first pass
// of sort_pairs_u32_lsd reads) — the sort then starts with its scatter: one launch less, and the records are folded by an eighth of
// the workgroups.
__global__ __launch_bounds__(256) void leaf_key_dims_hist_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                 const float* __restrict__ z, int n, float inv_leaf,
                                                                 const unsigned long long* __restrict__ parts, int nparts, int planned_bits,
                                                                 unsigned int* __restrict__ key, unsigned int* __restrict__ dims,
                                                                 unsigned int mask, int C, unsigned short* __restrict__ hist, int row_pitch) {
  extern __shared__ unsigned int s_hist[];  // [C]
  const int tid = threadIdx.x;
  for (int k = tid; k < C; k += 256) s_hist[k] = 0u;
  const int base = blockIdx.x * 2048;
  float px[8], py[8], pz[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256 + tid;
    const bool in = i < n;
    px[j] = in ? x[i] : NAN; py[j] = in ? y[i] : NAN; pz[j] = in ? z[i] : NAN;
  }
  const VgDims D = vg_fold_dims(parts, nparts, inv_leaf, planned_bits);   // its barrier also orders the zeroing above before the counts below
  if (blockIdx.x == 0 && tid == 0) { dims[0] = D.sentinel; dims[1] = D.n_finite; dims[2] = D.flags; dims[3] = (unsigned int)D.bits; }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int i = base + j * 256 + tid;
    if (i < n) {
      const unsigned int k = vg_key(D, inv_leaf, px[j], py[j], pz[j]);
      key[i] = k;
      atomicAdd(&s_hist[k & mask], 1u);
    }
  }
  __syncthreads();
  for (int k = tid; k < C; k += 256) hist[(size_t)k * row_pitch + blockIdx.x] = (unsigned short)s_hist[k];
}

__global__ __launch_bounds__(256) void deinterleave_kernel(const unsigned char* __restrict__ aos, size_t stride, int n,
                                                           float* __restrict__ x, float* __restrict__ y, float* __restrict__ z) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (((stride & 15) == 0) && ((reinterpret_cast<size_t>(aos) & 15) == 0)) {   // one 16-byte load per record (pcl::PointXYZI: 32-byte stride)
    const float4 q = *reinterpret_cast<const float4*>(aos + (size_t)i * stride);
    x[i] = q.x; y[i] = q.y; z[i] = q.z;
    return;
  }
  const float* p = (const float*)(aos + (size_t)i * stride);
  x[i] = p[0]; y[i] = p[1]; z[i] = p[2];
}

struct DeintMember { const unsigned char* aos; size_t stride; int n; float *x, *y, *z; };
struct DeintGroup { DeintMember m[LSR_GROUP]; };
__global__ __launch_bounds__(256) void deinterleave_group_kernel(const DeintGroup g) {
  const DeintMember& M = g.m[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M.n) return;
  if (((M.stride & 15) == 0) && ((reinterpret_cast<size_t>(M.aos) & 15) == 0)) {   // one 16-byte load per record
    const float4 q = *reinterpret_cast<const float4*>(M.aos + (size_t)i * M.stride);
    M.x[i] = q.x; M.y[i] = q.y; M.z[i] = q.z;
    return;
  }
  const float* p = (const float*)(M.aos + (size_t)i * M.stride);
  M.x[i] = p[0]; M.y[i] = p[1]; M.z[i] = p[2];
}

__global__ __launch_bounds__(256) void transform_strided_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                const float* __restrict__ z, int n, const float* __restrict__ Tdev,
                                                                unsigned char* __restrict__ out, size_t stride) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float px = x[i], py = y[i], pz = z[i];
  float* o = (float*)(out + (size_t)i * stride);
  o[0] = fmaf(Tdev[0], px, fmaf(Tdev[4], py, fmaf(Tdev[8], pz, Tdev[12])));
  o[1] = fmaf(Tdev[1], px, fmaf(Tdev[5], py, fmaf(Tdev[9], pz, Tdev[13])));
  o[2] = fmaf(Tdev[2], px, fmaf(Tdev[6], py, fmaf(Tdev[10], pz, Tdev[14])));
}

}  // namespace

int deinterleave(const void* d_aos, size_t stride_bytes, size_t n, DeviceCloud& out, hipStream_t stream) {
  int st = out.resize(n);
  if (st) return st;
  if (n == 0) return LSR_OK;
  hipLaunchKernelGGL(deinterleave_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     (const unsigned char*)d_aos, stride_bytes, (int)n, out.x(), out.y(), out.z());
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int deinterleave_group(const DeinterleaveJob* jobs, int count, hipStream_t stream) {
  int st;
  for (int g0 = 0; g0 < count; g0 += LSR_GROUP) {
    DeintGroup grp;
    std::memset(&grp, 0, sizeof(grp));
    const int ng = std::min(LSR_GROUP, count - g0);
    size_t nmax = 0;
    for (int k = 0; k < ng; k++) {
      const DeinterleaveJob& J = jobs[g0 + k];
      if ((st = J.out->resize(J.n))) return st;
      grp.m[k] = DeintMember{static_cast<const unsigned char*>(J.d_aos), J.stride, (int)J.n, J.out->x(), J.out->y(), J.out->z()};
      nmax = std::max(nmax, J.n);
    }
    if (nmax > 0) hipLaunchKernelGGL(deinterleave_group_kernel, dim3((unsigned)((nmax + 255) / 256), ng), dim3(256), 0, stream, grp);
  }
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

int transform_to_strided(const DeviceCloud& src, const float* d_T16, void* d_out, size_t stride_bytes, hipStream_t stream) {
  if (src.n == 0) return LSR_OK;
  hipLaunchKernelGGL(transform_strided_kernel, dim3((unsigned)((src.n + 255) / 256)), dim3(256), 0, stream, src.x(), src.y(),
                     src.z(), (int)src.n, d_T16, (unsigned char*)d_out, stride_bytes);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

// ---- N1: pcl::VoxelGrid::filter (centroid per occupied leaf, output ordered by leaf index) -------------
// scanmatcher/src/scanmatcher_component.cpp:324-328 (every scan, vg_size_for_input), :266-269, :443-447
// (map side, vg_size_for_map), graph_based_slam/src/graph_based_slam_component.cpp:224-226.
// Same key/sort machinery as K1; one thread per leaf (sorted_runs_centroids, lsd_sort.hip) sums its (few) points in ascending point order in FLOAT, as
// pcl::CentroidPoint does (PCL's own order inside a leaf is whatever std::sort leaves: unspecified; ascending index is
// the oracle's choice and this kernel's) — all fields, intensity included (downsample_all_data_).
int voxel_grid_filter(const DeviceCloud& cloud, float leaf, DeviceCloud& out, BuildScratch& sc, hipStream_t stream) {
  const int n = (int)cloud.n;
  out.n = 0;
  if (n == 0) return out.resize(0, cloud.has_i);
  int st;
  // A/B switch, read once: LSR_VG_DEVICE_DIMS=0 — always work out the grid dimensions on the host
  static const bool device_dims = [] { const char* e = getenv("LSR_VG_DEVICE_DIMS"); return !(e && e[0] == '0'); }();
  const float inv_leaf = 1.0f / leaf;
  SortScratch s;
  if ((st = sort_scratch_carve(sc, (size_t)n, false, &s))) return st;
  unsigned int* dims_dev = sc.words.p + 16;   // {sentinel, finite points, flags, key bits} of the device-side form, in front of the ladder
  const unsigned int* ks;
  const int* vs;

  // ---- device-side dimensions: the pass that wrote `cloud` left its bounding-box records in device memory (pc2_ingest) and an earlier
  // call on this scratch says how many key bits such a cloud needs -> key (folds the records itself), sort, run heads and centroids are
  // enqueued back to back; the host waits ONCE, for {runs, finite points, flags}.  A cloud that needs more bits than planned (or whose
  // index space overflows) comes back flagged and takes the host-side form below, which also renews the hint.
  if (device_dims && cloud.bbox_enqueued && !cloud.bbox_valid && sc.bbox_parts > 0 && sc.bbox_dev.p && sc.vg_bits_hint > 0 &&
      sc.vg_hint_leaf == leaf) {   // (an object that filters at two leaf sizes in turn — scans and keyframes — stays on the host form)
    const int planned_bits = sc.vg_bits_hint;
    LsdFirstHist fh;
    if ((st = lsd_first_hist_plan((size_t)n, planned_bits, sc.temp, &fh))) return st;
    if (fh.usable)   // the key kernel counts the first digit on the sort's own workgroups: the sort starts with its scatter
      hipLaunchKernelGGL(leaf_key_dims_hist_kernel, dim3(fh.nblk), dim3(256), (size_t)fh.C * 4, stream, cloud.x(), cloud.y(), cloud.z(), n,
                         inv_leaf, sc.bbox_dev.p, sc.bbox_parts, planned_bits, s.key_in, dims_dev, fh.mask, fh.C, fh.hist, fh.row_pitch);
    else
      hipLaunchKernelGGL(leaf_key_dims_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud.x(), cloud.y(), cloud.z(), n, inv_leaf,
                         sc.bbox_dev.p, sc.bbox_parts, planned_bits, s.key_in, dims_dev);
    if ((st = sort_scratch_run(s, (size_t)n, planned_bits, sc.temp, stream, &ks, &vs, fh.usable))) return st;
    unsigned int token = 0;
    if ((st = sorted_runs_begin(ks, (size_t)n, s.block_heads, s.block_base, sc, stream, &token, dims_dev))) return st;
    // the centroids do not wait for the count: the planes are laid out for n runs, the cloud shrinks to what was found
    if ((st = out.resize((size_t)n, cloud.has_i))) return st;
    if ((st = sorted_runs_centroids(ks, vs, (size_t)n, s.block_base, 0u, cloud.x(), cloud.y(), cloud.z(), cloud.i(), out.x(), out.y(), out.z(),
                                    out.i(), stream, dims_dev))) return st;
    int n_runs = 0;
    if ((st = sorted_runs_count(sc, stream, token, &n_runs))) return st;
    const unsigned int flags = sc.mb.p->vg_flags, n_finite = sc.mb.p->vg_finite;
    if (flags == 0u) {
      sc.vg_form = 2;
      sc.bbox_parts = 0;            // the records are spent
      cloud.bbox_enqueued = false;
      // the plan follows the clouds: up at once (the host form does that), down only when a cloud needs clearly fewer bits — a stream
      // whose index space hovers around a power of two would otherwise be flagged every other scan; an empty cloud says nothing
      const int needed = (int)sc.mb.p->vg_bits;
      if (n_finite > 0u && needed > 0 && needed <= sc.vg_bits_hint - 3) sc.vg_bits_hint = needed;
      return out.shrink((size_t)(n_runs - ((n_finite < (unsigned int)n) ? 1 : 0)));   // minus the sentinel run
    }
    // flagged: the centroid launch may still be writing `out` — the host-side form below runs behind it on the same stream
    out.n = 0;
    sc.vg_form = 3;
  } else {
    sc.vg_form = 1;
  }

  float mn[3], mx[3];
  unsigned int n_finite = 0;
  st = cloud_bbox(cloud, mn, mx, &n_finite, sc, stream);
  if (st) return st;
  if (n_finite == 0) return out.resize(0, cloud.has_i);
  const GridDims G = grid_dims(mn, mx, inv_leaf);
  if (G.volume > (long long)INT32_MAX) {  // PCL: "Leaf size is too small for the input dataset"
    set_last_error("voxel index space exceeds int32: leaf size too small for the cloud extent");
    return LSR_ERR_INDEX_OVERFLOW;
  }
  const int *min_b = G.min_b, *div_b = G.div_b;
  const unsigned int sentinel = (unsigned int)((int64_t)div_b[0] * div_b[1] * div_b[2]);  // one past the last leaf index
  sc.vg_bits_hint = bits_for(sentinel);
  sc.vg_hint_leaf = leaf;
  hipLaunchKernelGGL(leaf_key_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, cloud.x(), cloud.y(), cloud.z(), n, inv_leaf,
                     min_b[0], min_b[1], min_b[2], div_b[0], div_b[0] * div_b[1], sentinel, s.key_in, (uint4*)nullptr, (size_t)0,
                     (int*)nullptr, (size_t)0, (int*)nullptr);
  // hand-written stable LSD sort (three passes for a 27-bit leaf index) + run heads + centroids: lsd_sort.hip
  if ((st = sort_scratch_run(s, (size_t)n, bits_for(sentinel), sc.temp, stream, &ks, &vs))) return st;
  unsigned int token = 0;
  if ((st = sorted_runs_begin(ks, (size_t)n, s.block_heads, s.block_base, sc, stream, &token))) return st;
  // the centroids do not wait for the count either (planes laid out for n runs; shrunk below)
  if ((st = out.resize((size_t)n, cloud.has_i))) return st;
  if ((st = sorted_runs_centroids(ks, vs, (size_t)n, s.block_base, sentinel, cloud.x(), cloud.y(), cloud.z(), cloud.i(), out.x(), out.y(), out.z(),
                                  out.i(), stream))) return st;
  int n_runs = 0;
  if ((st = sorted_runs_count(sc, stream, token, &n_runs))) return st;   // host mailbox: no D2H copy, no stream sync
  return out.shrink((size_t)(n_runs - ((n_finite < (unsigned int)n) ? 1 : 0)));     // minus the sentinel run
}

// SoA planes -> strided xyz records (device to device)
namespace {
__global__ __launch_bounds__(256) void interleave_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ z, int n, unsigned char* __restrict__ out,
                                                         size_t stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float* o = (float*)(out + (size_t)i * stride);
  o[0] = x[i]; o[1] = y[i]; o[2] = z[i];
}
}  // namespace

int interleave(const DeviceCloud& in, void* d_out, size_t stride_bytes, hipStream_t stream) {
  if (in.n == 0) return LSR_OK;
  hipLaunchKernelGGL(interleave_kernel, dim3((unsigned)((in.n + 255) / 256)), dim3(256), 0, stream, in.x(), in.y(), in.z(),
                     (int)in.n, (unsigned char*)d_out, stride_bytes);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

// ---- N4: sensor_msgs/PointCloud2 <-> SoA planes with arbitrary float32 field offsets --------------------------------
// pcl::fromROSMsg (scanmatcher_component.cpp:201-202) reads x / y / z / intensity wherever the message's fields put them;
// pcl::toROSMsg (:279,284; SubMap.msg:4) writes pcl::PointXYZI's layout.  Offsets are in bytes inside a point_step record.
namespace {
__global__ __launch_bounds__(256) void pc2_write_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                                        const float* __restrict__ w, int n, unsigned char* __restrict__ data, int step,
                                                        int ox, int oy, int oz, int oi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned char* rec = data + (size_t)i * step;
  *reinterpret_cast<float*>(rec + ox) = x[i];
  *reinterpret_cast<float*>(rec + oy) = y[i];
  *reinterpret_cast<float*>(rec + oz) = z[i];
  if (oi >= 0) *reinterpret_cast<float*>(rec + oi) = w ? w[i] : 0.f;
}
}  // namespace

namespace {
// payload -> planes, the frontend's range filter and the bounding box of what is left in ONE pass (until round 5 three launches —
// read, range mask, bounding box — and two more trips over the planes).
//   range filter (N4, scanmatcher_component.cpp:210-218): keep p iff scan_min_range < sqrt(x^2 + y^2) < scan_max_range (double
//   arithmetic, as pow(p.x, 2.0) promotes); a rejected point gets a NaN x in the handle's private copy, so the voxel filter that
//   follows drops it exactly like non-finite input.
//   bounding box: the workgroup records go to the host mailbox (cloud_bbox_end folds them as it folds bbox_kernel's) and, the same
//   words, to device memory for voxel_grid_filter's device-side dimensions.
//   TF (lsr_set_input_source_pc2_tf): the scan arrives in the sensor frame and is moved into the robot frame as it is read
//   (tf2::doTransform, scanmatcher_component.cpp:195) — before the range test, the NaN marking and the box, which are all defined on
//   robot-frame coordinates.  The twelve floats travel in the kernel arguments; the untransformed instantiation never reads them.
template <bool TF>
__global__ __launch_bounds__(256) void pc2_ingest_kernel(const unsigned char* __restrict__ data, int step, int ox, int oy, int oz, int oi,
                                                         int n, float* __restrict__ x, float* __restrict__ y, float* __restrict__ z,
                                                         float* __restrict__ w, int do_range, double rmin, double rmax,
                                                         unsigned long long* __restrict__ parts_dev, BuildMailbox* __restrict__ mb,
                                                         unsigned int token, const SensorTf12 tf) {
  BoxAcc box;
  const int step_pts = gridDim.x * blockDim.x;
  for (int i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += 4 * step_pts) {  // four records per trip in flight
    float p[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + u * step_pts;
      if (i < n) {
        const unsigned char* rec = data + (size_t)i * step;
        p[u][0] = *reinterpret_cast<const float*>(rec + ox);
        p[u][1] = *reinterpret_cast<const float*>(rec + oy);
        p[u][2] = *reinterpret_cast<const float*>(rec + oz);
        p[u][3] = (w && oi >= 0) ? *reinterpret_cast<const float*>(rec + oi) : 0.f;
      } else {
        p[u][0] = p[u][1] = p[u][2] = NAN; p[u][3] = 0.f;
      }
    }
    if (TF) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const float sx = p[u][0], sy = p[u][1], sz = p[u][2];
        p[u][0] = xform_ref(tf.m[0], tf.m[1], tf.m[2], tf.m[3], sx, sy, sz);
        p[u][1] = xform_ref(tf.m[4], tf.m[5], tf.m[6], tf.m[7], sx, sy, sz);
        p[u][2] = xform_ref(tf.m[8], tf.m[9], tf.m[10], tf.m[11], sx, sy, sz);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int i = i0 + u * step_pts;
      if (i >= n) continue;
      if (do_range) {
        const double px = (double)p[u][0], py = (double)p[u][1];
        const double r = sqrt(px * px + py * py);
        if (!(rmin < r && r < rmax)) p[u][0] = __int_as_float(0x7FC00000);
      }
      x[i] = p[u][0]; y[i] = p[u][1]; z[i] = p[u][2];
      if (w) w[i] = p[u][3];
      box.add(p[u][0], p[u][1], p[u][2]);
    }
  }
  box_publish(box_fold_block(box), &mb->part[blockIdx.x], token, parts_dev + (size_t)blockIdx.x * 8, nullptr);
}
}  // namespace

namespace {
// tf2::doTransform(*msg, transformed_msg, transform) on a payload (scanmatcher_component.cpp:195), one record per thread: x / y / z moved by
// xform_ref, every other byte of the record copied.  in == out (in place) or disjoint.  The records of a workgroup are contiguous: for a
// disjoint output they are copied as words by the whole workgroup first, the coordinates are stored over the copy.  A thread reads no
// record of `in` but its own, and in place nothing else is written.
__global__ __launch_bounds__(256) void pc2_transform_kernel(const unsigned char* in, unsigned char* out, int step, int ox, int oy, int oz,
                                                            int n, const SensorTf12 tf) {
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  if (i < n) {
    const unsigned char* rec = in + (size_t)i * step;
    sx = *reinterpret_cast<const float*>(rec + ox);
    sy = *reinterpret_cast<const float*>(rec + oy);
    sz = *reinterpret_cast<const float*>(rec + oz);
  }
  if (out != in) {   // uniform over the launch
    const size_t first = (size_t)blockIdx.x * 256;
    const size_t count = min((size_t)256, (size_t)n - first);
    const unsigned int* src = reinterpret_cast<const unsigned int*>(in + first * step);
    unsigned int* dst = reinterpret_cast<unsigned int*>(out + first * step);
    const size_t words = count * (size_t)(step / 4);
    for (size_t k = tid; k < words; k += 256) dst[k] = src[k];
    __syncthreads();   // the copy precedes the coordinate stores below (other threads wrote this thread's record)
  }
  if (i < n) {
    unsigned char* o = out + (size_t)i * step;
    *reinterpret_cast<float*>(o + ox) = xform_ref(tf.m[0], tf.m[1], tf.m[2], tf.m[3], sx, sy, sz);
    *reinterpret_cast<float*>(o + oy) = xform_ref(tf.m[4], tf.m[5], tf.m[6], tf.m[7], sx, sy, sz);
    *reinterpret_cast<float*>(o + oz) = xform_ref(tf.m[8], tf.m[9], tf.m[10], tf.m[11], sx, sy, sz);
  }
}

// the completion word of pc2_transform: one system-scope store behind the transform launch, which has ended when this one starts
__global__ void pc2_transform_publish_kernel(BuildMailbox* __restrict__ mb, unsigned int token) {
  __hip_atomic_store(&mb->tf_token, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace

int pc2_transform(const void* d_in, void* d_out, int step, int ox, int oy, int oz, size_t n, const SensorTf12& tf, BuildScratch& sc,
                  hipStream_t stream, bool wait) {
  if (n == 0) return LSR_OK;
  int st;
  if (wait && (st = sc.ensure_mailbox())) return st;
  const unsigned int nb = (unsigned int)((n + 255) / 256);
  hipLaunchKernelGGL(pc2_transform_kernel, dim3(nb), dim3(256), 0, stream, (const unsigned char*)d_in, (unsigned char*)d_out, step, ox, oy, oz,
                     (int)n, tf);
  LSR_HIP(hipGetLastError());
  if (!wait) return LSR_OK;
  unsigned int token = ++sc.token;
  if (token == 0) token = ++sc.token;
  hipLaunchKernelGGL(pc2_transform_publish_kernel, dim3(1), dim3(1), 0, stream, sc.d_mb, token);
  LSR_HIP(hipGetLastError());
  return wait_mailbox_word(&sc.mb.p->tf_token, token, stream, sc.wait_mode, "sensor-frame transform");
}

int pc2_ingest(const void* d_data, int step, int ox, int oy, int oz, int oi, size_t n, bool do_range, double rmin, double rmax,
               DeviceCloud& out, BuildScratch& sc, hipStream_t stream, const SensorTf12* tf) {
  int st = out.resize(n, oi >= 0);
  if (st) return st;
  if (n == 0) return LSR_OK;
  if ((st = sc.ensure_mailbox())) return st;
  if ((st = sc.bbox_dev.reserve((size_t)BBOX_MAX_PARTS * 8))) return st;
  unsigned int token = ++sc.token;
  if (token == 0) token = ++sc.token;
  const int nb = std::max(1, std::min((int)((n + 1023) / 1024), BBOX_MAX_PARTS));
  if (tf)
    hipLaunchKernelGGL(pc2_ingest_kernel<true>, dim3(nb), dim3(256), 0, stream, (const unsigned char*)d_data, step, ox, oy, oz, oi, (int)n, out.x(),
                       out.y(), out.z(), out.i(), do_range ? 1 : 0, rmin, rmax, sc.bbox_dev.p, sc.d_mb, token, *tf);
  else
    hipLaunchKernelGGL(pc2_ingest_kernel<false>, dim3(nb), dim3(256), 0, stream, (const unsigned char*)d_data, step, ox, oy, oz, oi, (int)n, out.x(),
                       out.y(), out.z(), out.i(), do_range ? 1 : 0, rmin, rmax, sc.bbox_dev.p, sc.d_mb, token, SensorTf12{});
  LSR_HIP(hipGetLastError());
  sc.bbox_parts = nb;
  sc.bbox_token = token;
  out.bbox_enqueued = true;
  return LSR_OK;
}

int pc2_write(const DeviceCloud& in, void* d_data, int step, int ox, int oy, int oz, int oi, hipStream_t stream) {
  if (in.n == 0) return LSR_OK;
  hipLaunchKernelGGL(pc2_write_kernel, dim3((unsigned)((in.n + 255) / 256)), dim3(256), 0, stream, in.x(), in.y(), in.z(), in.i(), (int)in.n,
                     (unsigned char*)d_data, step, ox, oy, oz, oi);
  LSR_HIP(hipGetLastError());
  return LSR_OK;
}

}  // namespace lsr

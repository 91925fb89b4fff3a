// IMU de-skew of the raw scan on the device: LidarUndistortion::adjustDistortion (scanmatcher/include/scanmatcher/
// lidar_undistortion.hpp:110-226; scanmatcher_component.cpp:204-208, before the range filter) as a records -> records step, and the
// C ABI of the IMU queue behind it (lidar_undistortion.hpp:53-106; scanmatcher_component.cpp:501-527).
//
// The reference walks the points in order with two carried states; deskew_point.hpp shows why both are order-free.  Launches, all on
// the handle's stream, one point per thread, DESKEW_WG points per workgroup:
//   deskew_half_kernel      h_i, flag_i, H = min{i : flag_i} (one atomicMin per wave that has a flag); start / end / diff of the scan
//   deskew_front_kernel     t_i, f_i, f'_i; the maximum of f' per workgroup; the pose of point 0 (or start_missing)
//   deskew_apply_kernel     carry = max of the workgroup maxima in front of this workgroup (the scan of the maxima: every workgroup
//                           folds the <= n / 256 words it needs itself, no launch of its own), prefix maximum inside the workgroup,
//                           pointer, skip, interpolation, transform, record out — the only writer of the records, and it reads no
//                           record but its own, so in place is allowed
//   deskew_publish_kernel   c_{n-1}, the skip count, start_missing and H into the host mailbox, token last
// The IMU table (<= 201 entries of 48 bytes) and the control block travel in ONE copy from pinned memory; the kernels keep the table in LDS.
#include "deskew.hpp"

#include <algorithm>

#include "api_internal.hpp"

namespace lsr {

namespace {

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}

__global__ __launch_bounds__(DESKEW_WG) void deskew_half_kernel(const unsigned char* __restrict__ data, int step, int ox, int oy, int n,
                                                               DeskewCtl* __restrict__ ctl) {
  const int i = blockIdx.x * DESKEW_WG + threadIdx.x;
  const float start = deskew_ori(*reinterpret_cast<const float*>(data + ox), *reinterpret_cast<const float*>(data + oy));
  unsigned int mine = 0xFFFFFFFFu;
  if (i < n) {
    const unsigned char* rec = data + (size_t)i * step;
    bool flag;
    (void)deskew_first_branch(deskew_ori(*reinterpret_cast<const float*>(rec + ox), *reinterpret_cast<const float*>(rec + oy)), start, &flag);
    if (flag) mine = (unsigned int)i;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mine = min(mine, (unsigned int)__shfl_xor((int)mine, m, 64));
  if ((threadIdx.x & 63) == 0 && mine != 0xFFFFFFFFu) atomicMin(&ctl->half_index, mine);
  if (i == 0) {
    const unsigned char* last = data + (size_t)(n - 1) * step;
    const float end = deskew_end(start, deskew_ori(*reinterpret_cast<const float*>(last + ox), *reinterpret_cast<const float*>(last + oy)));
    ctl->start = start;
    ctl->end = end;
    ctl->diff = end - start;
  }
}

__global__ __launch_bounds__(DESKEW_WG) void deskew_front_kernel(const unsigned char* __restrict__ data, int step, int ox, int oy, int n,
                                                                DeskewCtl* __restrict__ ctl, const ImuEntry* __restrict__ table,
                                                                double scan_time, double scan_period, float* __restrict__ rel_out,
                                                                int* __restrict__ code_out, int* __restrict__ block_max) {
  __shared__ ImuEntry s_table[IMU_TABLE_MAX];
  __shared__ int s_max[DESKEW_WG / 64];
  const int tid = threadIdx.x;
  const int m = ctl->m;
  {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(table);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(s_table);
    const int words = (m + 1) * (int)(sizeof(ImuEntry) / 8);
    for (int k = tid; k < words; k += DESKEW_WG) dst[k] = src[k];
  }
  const unsigned int H = min(ctl->half_index, (unsigned int)n);
  const float start = ctl->start, end = ctl->end, diff = ctl->diff;
  __syncthreads();
  const ImuEntry* entry = s_table + 1;
  const int i = blockIdx.x * DESKEW_WG + tid;
  int fv = 0;
  if (i < n) {
    const unsigned char* rec = data + (size_t)i * step;
    const float ori = deskew_ori(*reinterpret_cast<const float*>(rec + ox), *reinterpret_cast<const float*>(rec + oy));
    bool flag;
    const float ori_h = ((unsigned int)i <= H) ? deskew_first_branch(ori, start, &flag) : deskew_second_branch(ori, end);
    const float rel = deskew_rel_time(ori_h, start, diff, scan_period);
    const double t = scan_time + (double)rel;
    const int f = deskew_front(entry, m, t);
    fv = deskew_front_valid(entry, f, t, scan_period);
    rel_out[i] = rel;
    code_out[i] = (fv == f) ? f : (f | (int)0x80000000);
    if (i == 0) {   // point 0 stands on entry max(0, f_0) = f_0
      const bool missing = (fv != f) || deskew_skips(entry, f, t, scan_period);
      ctl->start_missing = missing ? 1 : 0;
      if (!missing) {
        DeskewPose P;
        deskew_pose(entry, f, t, &P);
        ctl->start_pose = P;
        float R[9];
        deskew_rotation(P.rpy, R);
        for (int k = 0; k < 9; k++) ctl->Rs[k] = R[k];
      }
    }
  }
  const int wm = wave_max(fv);
  if ((tid & 63) == 0) s_max[tid >> 6] = wm;
  __syncthreads();
  if (tid == 0) {
    int v = s_max[0];
    for (int w = 1; w < DESKEW_WG / 64; w++) v = max(v, s_max[w]);
    block_max[blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(DESKEW_WG) void deskew_apply_kernel(const unsigned char* in, unsigned char* out, int step,
                                                                int ox, int oy, int oz, int n, DeskewCtl* __restrict__ ctl,
                                                                const ImuEntry* __restrict__ table, double scan_time, double scan_period,
                                                                const float* __restrict__ rel_in, const int* __restrict__ code_in,
                                                                const int* __restrict__ block_max, int* __restrict__ entry_out,
                                                                unsigned char* __restrict__ skipped_out) {
  __shared__ ImuEntry s_table[IMU_TABLE_MAX];
  __shared__ int s_wave[DESKEW_WG / 64], s_carry[DESKEW_WG / 64];
  __shared__ unsigned int s_skipped;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m = ctl->m;
  {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(table);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(s_table);
    const int words = (m + 1) * (int)(sizeof(ImuEntry) / 8);
    for (int k = tid; k < words; k += DESKEW_WG) dst[k] = src[k];
  }
  if (tid == 0) s_skipped = 0u;
  // the scan of the workgroup maxima, folded by the workgroup that needs it: carry = max of block_max[0 .. blockIdx.x)
  int carry = 0;
  for (int j = tid; j < (int)blockIdx.x; j += DESKEW_WG) carry = max(carry, block_max[j]);
  carry = wave_max(carry);
  if (lane == 0) s_carry[wv] = carry;
  const int i = blockIdx.x * DESKEW_WG + tid;
  const int code = (i < n) ? code_in[i] : 0;
  const int f = code & 0x7FFFFFFF;
  const int fv = (code < 0) ? 0 : f;
  // inclusive prefix maximum inside the wave, then across the waves
  int incl = fv;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d, 64);
    if (lane >= d) incl = max(incl, o);
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  carry = s_carry[0];
  for (int w = 1; w < DESKEW_WG / 64; w++) carry = max(carry, s_carry[w]);
  int before = carry;   // c_{i-1}
  for (int w = 0; w < wv; w++) before = max(before, s_wave[w]);
  const int up = __shfl_up(incl, 1, 64);
  if (lane > 0) before = max(before, up);

  // the records of this workgroup are contiguous: copy them as words, then overwrite the coordinates
  if (out != in) {
    const size_t first = (size_t)blockIdx.x * DESKEW_WG;
    const size_t count = min((size_t)DESKEW_WG, (size_t)n - first);
    const unsigned int* src = reinterpret_cast<const unsigned int*>(in + first * step);
    unsigned int* dst = reinterpret_cast<unsigned int*>(out + first * step);
    const size_t words = count * (size_t)(step / 4);
    for (size_t k = tid; k < words; k += DESKEW_WG) dst[k] = src[k];
  }
  __syncthreads();   // the copy above precedes the coordinate stores below (other threads wrote this thread's record)

  const ImuEntry* entry = s_table + 1;
  bool skip = false;
  if (i < n) {
    const float rel = rel_in[i];
    const double t = scan_time + (double)rel;
    const int p = max(before, f);
    skip = deskew_skips(entry, p, t, scan_period);
    entry_out[i] = p;
    skipped_out[i] = skip ? 1 : 0;
    if (i == n - 1) ctl->cursor = skip ? before : p;
    if (!skip && i > 0 && ctl->start_missing == 0) {
      const unsigned char* rec = in + (size_t)i * step;
      const float x = *reinterpret_cast<const float*>(rec + ox), y = *reinterpret_cast<const float*>(rec + oy),
                  z = *reinterpret_cast<const float*>(rec + oz);
      DeskewPose cur;
      deskew_pose(entry, p, t, &cur);
      float q[3];
      deskew_transform(ctl->Rs, ctl->start_pose, cur, rel, x, y, z, q);
      unsigned char* o = out + (size_t)i * step;
      *reinterpret_cast<float*>(o + ox) = q[0];
      *reinterpret_cast<float*>(o + oy) = q[1];
      *reinterpret_cast<float*>(o + oz) = q[2];
    }
  }
  const unsigned long long b = __ballot(skip);
  if (lane == 0 && b != 0ull) atomicAdd(&s_skipped, (unsigned int)__popcll(b));
  __syncthreads();
  if (tid == 0 && s_skipped != 0u) atomicAdd(&ctl->n_skipped, s_skipped);
}

__global__ void deskew_publish_kernel(const DeskewCtl* __restrict__ ctl, int n, DeskewMailbox* __restrict__ mb, unsigned int token) {
  mb->cursor = ctl->cursor;
  mb->n_skipped = (int)ctl->n_skipped;
  mb->start_missing = ctl->start_missing;
  mb->half_index = (int)min(ctl->half_index, (unsigned int)n);
  __threadfence_system();
  __hip_atomic_store(&mb->token, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

int deskew_run(DeskewState& S, const void* d_in, void* d_out, size_t n, int step, int ox, int oy, int oz, double scan_time, int wait_mode,
               hipStream_t stream) {
  int st;
  if (!S.d_mb) {   // keyed on the device view: a call that failed half way through here starts over
    if ((st = S.mb.reserve(1, hipHostMallocMapped | hipHostMallocCoherent))) return st;
    std::memset(S.mb.p, 0, sizeof(DeskewMailbox));
    DeskewMailbox* d = nullptr;
    LSR_HIP(hipHostGetDevicePointer((void**)&d, S.mb.p, 0));
    if (!d) { set_last_error("de-skew mailbox has no device address"); return LSR_ERR_HIP; }
    S.d_mb = d;
  }
  const int nb = (int)((n + DESKEW_WG - 1) / DESKEW_WG);
  if ((st = S.d_up.reserve(1)) || (st = S.rel.reserve(n)) || (st = S.code.reserve(n)) || (st = S.entry.reserve(n)) ||
      (st = S.skipped.reserve(n)) || (st = S.block_max.reserve((size_t)nb)))
    return st;
  const int m = S.h_up.p->ctl.m;
  LSR_HIP(hipMemcpyAsync(S.d_up.p, S.h_up.p, sizeof(DeskewCtl) + (size_t)(m + 1) * sizeof(ImuEntry), hipMemcpyHostToDevice, stream));
  DeskewCtl* ctl = &S.d_up.p->ctl;
  const ImuEntry* table = S.d_up.p->table;
  const double period = S.imu.scan_period;
  unsigned int token = ++S.token;
  if (token == 0) token = ++S.token;
  const unsigned char* in = static_cast<const unsigned char*>(d_in);
  unsigned char* out = static_cast<unsigned char*>(d_out);
  hipLaunchKernelGGL(deskew_half_kernel, dim3(nb), dim3(DESKEW_WG), 0, stream, in, step, ox, oy, (int)n, ctl);
  hipLaunchKernelGGL(deskew_front_kernel, dim3(nb), dim3(DESKEW_WG), 0, stream, in, step, ox, oy, (int)n, ctl, table, scan_time, period, S.rel.p,
                     S.code.p, S.block_max.p);
  hipLaunchKernelGGL(deskew_apply_kernel, dim3(nb), dim3(DESKEW_WG), 0, stream, in, out, step, ox, oy, oz, (int)n, ctl, table, scan_time, period,
                     S.rel.p, S.code.p, S.block_max.p, S.entry.p, S.skipped.p);
  hipLaunchKernelGGL(deskew_publish_kernel, dim3(1), dim3(1), 0, stream, ctl, (int)n, S.d_mb, token);
  LSR_HIP(hipGetLastError());
  return wait_mailbox_word(&S.mb.p->token, token, stream, wait_mode, "de-skew");
}

}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_imu_reset(lsr_handle h, double scan_period) {
  LSR_CHECK_HANDLE_NOT_NULL(h);   // the IMU entries touch no device: no DeviceGuard, no stream
  if (!(scan_period > 0.0)) { set_last_error("scan_period must be > 0"); return LSR_ERR_INVALID_ARGUMENT; }
  h->deskew.imu.reset(scan_period);
  h->deskew.trace_n = 0;
  return LSR_OK;
}

int lsr_imu_push(lsr_handle h, const float* ang_vel3, const float* acc3, const float* quat_wxyz4, double stamp) {
  LSR_CHECK_HANDLE_NOT_NULL(h);
  if (!ang_vel3 || !acc3 || !quat_wxyz4) { set_last_error("null IMU sample"); return LSR_ERR_INVALID_ARGUMENT; }
  if (h->deskew.imu.push(ang_vel3, acc3, quat_wxyz4, stamp) != IMU_PUSH_OK) {
    set_last_error("IMU sample refused: its stamp is smaller than the previous sample's");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  return LSR_OK;
}

int lsr_imu_receive(lsr_handle h, const double* orientation_xyzw4, const double* angular_velocity3, const double* linear_acceleration3,
                    double stamp) {
  LSR_CHECK_HANDLE_NOT_NULL(h);
  if (!orientation_xyzw4 || !angular_velocity3 || !linear_acceleration3) { set_last_error("null IMU message field"); return LSR_ERR_INVALID_ARGUMENT; }
  float ang[3], acc[3], quat[4];
  ImuQueue::sample_from_msg(orientation_xyzw4, angular_velocity3, linear_acceleration3, ang, acc, quat);
  return lsr_imu_push(h, ang, acc, quat, stamp);
}

int lsr_imu_info(lsr_handle h, int32_t* info4) {
  LSR_CHECK_HANDLE_NOT_NULL(h);
  if (!info4) { set_last_error("null output"); return LSR_ERR_INVALID_ARGUMENT; }
  const ImuQueue& Q = h->deskew.imu;
  info4[0] = (int32_t)std::min<long long>(Q.count, INT32_MAX);
  info4[1] = Q.last;
  info4[2] = Q.last_iter;
  info4[3] = 0;
  return LSR_OK;
}

int lsr_deskew_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, double scan_time, int on_device,
                   void* out_data, lsr_deskew_info* info) {
  LSR_CHECK_HANDLE(h);
  // the intensity field is not looked at: every byte outside x / y / z is copied as it is, whatever the layout says about it
  int st = arg_error(check_layout_xyz(layout));
  if (st) return st;
  if ((st = arg_error(check_records_in_out(data, out_data, n_points, layout->point_step)))) return st;
  const size_t bytes = n_points * (size_t)layout->point_step;
  DeskewState& S = h->deskew;
  lsr_deskew_info I = {0, 0, -1, S.imu.last_iter};
  S.trace_n = 0;
  if (n_points == 0 || S.imu.last <= 0) {   // the reference moves nothing (a queue whose newest slot is 0 included)
    if (n_points > 0 && out_data != data) {
      if (on_device) {
        // no kernel, so no mailbox to wait for: this rare path (a cloud before the second IMU sample) synchronises the stream, so that
        // the records are complete when the call returns, for a reader on any stream, like on the path below
        LSR_HIP(hipMemcpyAsync(out_data, data, bytes, hipMemcpyDeviceToDevice, h->stream));
        LSR_HIP(hipStreamSynchronize(h->stream));
      } else {
        std::memcpy(out_data, data, bytes);
      }
    }
    if (info) *info = I;
    return LSR_OK;
  }
  if ((st = S.h_up.reserve(1))) return st;
  DeskewUpload& U = *S.h_up.p;
  std::memset(&U.ctl, 0, sizeof(DeskewCtl));
  U.ctl.half_index = 0xFFFFFFFFu;
  U.ctl.m = S.imu.linearise(U.table);
  // device records: deskew_run has waited for the mailbox, the records are complete; host records: the copy down comes behind it
  if ((st = records_in_records_out(h, data, out_data, bytes, on_device != 0, [&](const void* d_in, void* d_out) {
        return deskew_run(S, d_in, d_out, n_points, (int)layout->point_step, (int)layout->offset_x, (int)layout->offset_y,
                          (int)layout->offset_z, scan_time, h->scratch.wait_mode, h->stream);
      })))
    return st;
  const DeskewMailbox& M = *S.mb.p;
  S.trace_n = n_points;
  S.trace_base = S.imu.last_iter;
  S.imu.advance(M.cursor);
  I.n_skipped = M.n_skipped;
  I.start_missing = M.start_missing;
  I.half_index = M.half_index;
  I.cursor = S.imu.last_iter;
  if (info) *info = I;
  return LSR_OK;
}

int lsr_deskew_trace(lsr_handle h, float* rel_time, int32_t* slot, uint8_t* skipped) {
  LSR_CHECK_HANDLE(h);
  DeskewState& S = h->deskew;
  const size_t n = S.trace_n;
  if (n == 0) return LSR_OK;
  if (rel_time) LSR_HIP(hipMemcpyAsync(rel_time, S.rel.p, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (slot) LSR_HIP(hipMemcpyAsync(slot, S.entry.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (skipped) LSR_HIP(hipMemcpyAsync(skipped, S.skipped.p, n, hipMemcpyDeviceToHost, h->stream));
  LSR_HIP(hipStreamSynchronize(h->stream));
  if (slot)
    for (size_t i = 0; i < n; i++) slot[i] = (slot[i] + S.trace_base) % IMU_QUEUE_LENGTH;
  return LSR_OK;
}

}  // extern "C"

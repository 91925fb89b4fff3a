// TEST INFRASTRUCTURE.  csrc/imu_queue.hpp and csrc/deskew_point.hpp compiled for the CPU and driven the way csrc/deskew.hip drives
// them — H as a minimum index, the IMU pointer as an inclusive prefix maximum of f', then one independent step per point — so that
// the claim the device formulation rests on (it equals the reference's sequential walk, tests/deskew_numpy.py) is checked without a
// GPU (tests/test_deskew_cpu.py).
//   g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off harness.cpp -o libdeskewemu.so
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define LSR_HOST_EMU 1
#include "../../lidarslam_ros2_amd/csrc/deskew_point.hpp"

using namespace lsr;

extern "C" {

void* emu_queue_new() { return new ImuQueue(); }
void emu_queue_free(void* q) { delete static_cast<ImuQueue*>(q); }
void emu_queue_reset(void* q, double scan_period) { static_cast<ImuQueue*>(q)->reset(scan_period); }
int emu_queue_push(void* q, const float* ang_vel3, const float* acc3, const float* quat_wxyz, double stamp) {
  return static_cast<ImuQueue*>(q)->push(ang_vel3, acc3, quat_wxyz, stamp);
}
// lsr_imu_receive without a handle: the message fields through ImuQueue::sample_from_msg, then push
int emu_queue_receive(void* q, const double* q_xyzw, const double* ang_vel, const double* lin_acc, double stamp, float* sample10) {
  ImuQueue::sample_from_msg(q_xyzw, ang_vel, lin_acc, sample10, sample10 + 3, sample10 + 6);
  return static_cast<ImuQueue*>(q)->push(sample10, sample10 + 3, sample10 + 6, stamp);
}
void emu_queue_info(void* q, int32_t* info4) {
  const ImuQueue& Q = *static_cast<ImuQueue*>(q);
  info4[0] = (int32_t)Q.count; info4[1] = Q.last; info4[2] = Q.last_iter; info4[3] = 0;
}
// the whole ring: stamp[200], fields[200][18] = rpy, acc, ang_vel, shift, velo, ang_rot
void emu_queue_dump(void* q, double* stamp, float* fields) {
  const ImuQueue& Q = *static_cast<ImuQueue*>(q);
  for (int s = 0; s < IMU_QUEUE_LENGTH; s++) {
    stamp[s] = Q.stamp[s];
    float* F = fields + 18 * s;
    for (int k = 0; k < 3; k++) {
      F[k] = Q.rpy[s][k]; F[3 + k] = Q.acc[s][k]; F[6 + k] = Q.ang_vel[s][k];
      F[9 + k] = Q.shift[s][k]; F[12 + k] = Q.velo[s][k]; F[15 + k] = Q.ang_rot[s][k];
    }
  }
}
// the linearised table: stamp[201], fields[201][9] = rpy, shift, velo; row 0 is entry -1; returns m
int emu_queue_table(void* q, double* stamp, float* fields) {
  ImuEntry T[IMU_TABLE_MAX];
  std::memset(T, 0, sizeof(T));
  const int m = static_cast<ImuQueue*>(q)->linearise(T);
  for (int r = 0; r < m + 1; r++) {
    stamp[r] = T[r].stamp;
    for (int k = 0; k < 3; k++) { fields[9 * r + k] = T[r].rpy[k]; fields[9 * r + 3 + k] = T[r].shift[k]; fields[9 * r + 6 + k] = T[r].velo[k]; }
  }
  return m;
}

// xyz: n x 3 floats in, out: n x 3 floats; info4 = {n_skipped, start_missing, half_index, last_iter after the call}
void emu_deskew(void* q, const float* xyz, int n, double scan_time, float* out, float* rel_time, int32_t* slot, uint8_t* skipped,
                int32_t* info4) {
  ImuQueue& Q = *static_cast<ImuQueue*>(q);
  std::memcpy(out, xyz, sizeof(float) * 3 * (size_t)n);
  info4[0] = 0; info4[1] = 0; info4[2] = -1; info4[3] = Q.last_iter;
  if (n == 0 || Q.last <= 0) return;
  ImuEntry T[IMU_TABLE_MAX];
  const int m = Q.linearise(T);
  const ImuEntry* entry = T + 1;
  const double period = Q.scan_period;
  // K1
  const float start = deskew_ori(xyz[0], xyz[1]);
  const float end = deskew_end(start, deskew_ori(xyz[3 * (n - 1)], xyz[3 * (n - 1) + 1]));
  const float diff = end - start;
  int H = n;
  for (int i = n - 1; i >= 0; i--) {   // any order: a minimum
    bool flag;
    (void)deskew_first_branch(deskew_ori(xyz[3 * i], xyz[3 * i + 1]), start, &flag);
    if (flag && i < H) H = i;
  }
  // K2
  std::vector<int> f(n), fv(n);
  std::vector<double> t(n);
  for (int i = 0; i < n; i++) {
    const float ori = deskew_ori(xyz[3 * i], xyz[3 * i + 1]);
    bool flag;
    const float ori_h = (i <= H) ? deskew_first_branch(ori, start, &flag) : deskew_second_branch(ori, end);
    rel_time[i] = deskew_rel_time(ori_h, start, diff, period);
    t[i] = scan_time + (double)rel_time[i];
    f[i] = deskew_front(entry, m, t[i]);
    fv[i] = deskew_front_valid(entry, f[i], t[i], period);
  }
  // K3: inclusive prefix maximum
  std::vector<int> c(n);
  for (int i = 0, run = 0; i < n; i++) { run = fv[i] > run ? fv[i] : run; c[i] = run; }
  // K4
  const int p0 = f[0];
  const bool missing = deskew_skips(entry, p0, t[0], period);
  DeskewPose S;
  float Rs[9];
  if (!missing) { deskew_pose(entry, p0, t[0], &S); deskew_rotation(S.rpy, Rs); }
  int n_skipped = 0;
  for (int i = 0; i < n; i++) {
    const int before = i ? c[i - 1] : 0;
    const int p = before > f[i] ? before : f[i];
    const bool skip = deskew_skips(entry, p, t[i], period);
    slot[i] = (Q.last_iter + p) % IMU_QUEUE_LENGTH;
    skipped[i] = skip ? 1 : 0;
    n_skipped += skip ? 1 : 0;
    if (!skip && i > 0 && !missing) {
      DeskewPose cur;
      deskew_pose(entry, p, t[i], &cur);
      deskew_transform(Rs, S, cur, rel_time[i], xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], out + 3 * i);
    }
  }
  Q.advance(c[n - 1]);
  info4[0] = n_skipped; info4[1] = missing ? 1 : 0; info4[2] = H; info4[3] = Q.last_iter;
}

}  // extern "C"

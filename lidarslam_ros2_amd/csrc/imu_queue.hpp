// The IMU queue of the frontend's de-skew: LidarUndistortion::getImu (scanmatcher/include/scanmatcher/lidar_undistortion.hpp:53-106,
// fed by ScanMatcherComponent::receiveImu, scanmatcher_component.cpp:501-527) restated as a host-side ring of 200 slots plus the
// LINEARISATION of that ring into the table the de-skew kernels read (csrc/deskew.hip never sees the ring).  Plain C++, no HIP
// types: tests/test_deskew_cpu.py compiles this file for the host and compares it bit for bit with tests/deskew_numpy.py.
//
// Number formats.  Stamps are f64, everything else is stored as f32.  An expression that mixes an f32 operand with the f64 `dt` is
// evaluated in f64 and rounded to f32 when it is stored (C's usual arithmetic conversions); roll / pitch / yaw and the rotation of
// the acceleration are pure f32.  The file is meant to be compiled without FMA contraction (-ffp-contract=off).
//
// Two definitions the reference leaves open: every slot starts out as zeros (the reference's arrays are indeterminate), and a push
// whose stamp is smaller than the previous push's is refused (IMU_PUSH_OUT_OF_ORDER) and stored nowhere — the table handed to the
// device then has non-decreasing stamps, which is what turns the reference's walking pointer into a prefix maximum (deskew_point.hpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace lsr {

constexpr int IMU_QUEUE_LENGTH = 200;          // imu_que_length_
constexpr int IMU_TABLE_MAX = IMU_QUEUE_LENGTH + 1;   // entry -1 and up to 200 entries
constexpr int IMU_PUSH_OK = 0, IMU_PUSH_OUT_OF_ORDER = 1;

// One entry of the linearised table: 48 bytes, what a point needs of one IMU sample.
struct ImuEntry {
  double stamp;
  float rpy[3];
  float shift[3];
  float velo[3];
  float pad;
};

struct ImuQueue {
  double scan_period = 0.1;
  int last = -1;          // imu_ptr_last_
  int last_iter = 0;      // imu_ptr_last_iter_
  long long count = 0;    // accepted pushes since the last reset
  double stamp[IMU_QUEUE_LENGTH];
  float rpy[IMU_QUEUE_LENGTH][3];
  float acc[IMU_QUEUE_LENGTH][3];
  float ang_vel[IMU_QUEUE_LENGTH][3];
  float shift[IMU_QUEUE_LENGTH][3];
  float velo[IMU_QUEUE_LENGTH][3];
  float ang_rot[IMU_QUEUE_LENGTH][3];

  ImuQueue() { reset(0.1); }

  void reset(double period) {
    scan_period = period;
    last = -1;
    last_iter = 0;
    count = 0;
    std::memset(stamp, 0, sizeof(stamp));
    std::memset(rpy, 0, sizeof(rpy));
    std::memset(acc, 0, sizeof(acc));
    std::memset(ang_vel, 0, sizeof(ang_vel));
    std::memset(shift, 0, sizeof(shift));
    std::memset(velo, 0, sizeof(velo));
    std::memset(ang_rot, 0, sizeof(ang_rot));
  }

  // rotation matrix of a (unit) quaternion w x y z, f32, row-major
  static void quat_to_matrix(const float* q, float* m) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
    const float twx = tx * w, twy = ty * w, twz = tz * w;
    const float txx = tx * x, txy = ty * x, txz = tz * x;
    const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
    m[0] = 1.0f - (tyy + tzz); m[1] = txy - twz; m[2] = txz + twy;
    m[3] = txy + twz; m[4] = 1.0f - (txx + tzz); m[5] = tyz - twx;
    m[6] = txz - twy; m[7] = tyz + twx; m[8] = 1.0f - (txx + tyy);
  }

  // sensor_msgs/Imu fields -> the sample push() takes, as ScanMatcherComponent::receiveImu forms it (scanmatcher_component.cpp:
  // 505-522): roll / pitch of the orientation's rotation matrix in double (tf2::Matrix3x3::getRPY away from the gimbal lock),
  // acc = float(a) + {sin(pitch), -cos(pitch) sin(roll), -cos(pitch) cos(roll)} * 9.81 in double, rounded to float.  The ONE copy of
  // this arithmetic: lsr_imu_receive, and through it every language surface, calls it.
  static void sample_from_msg(const double* q_xyzw, const double* angular_velocity, const double* linear_acceleration, float* ang_vel3,
                              float* acc3, float* quat_wxyz) {
    const double x = q_xyzw[0], y = q_xyzw[1], z = q_xyzw[2], w = q_xyzw[3];
    const double s = 2.0 / (x * x + y * y + z * z + w * w);
    double m20 = s * (x * z - w * y);
    const double m21 = s * (y * z + w * x), m22 = 1.0 - s * (x * x + y * y);
    m20 = m20 < -1.0 ? -1.0 : (m20 > 1.0 ? 1.0 : m20);
    const double pitch = -std::asin(m20), roll = std::atan2(m21, m22);
    acc3[0] = (float)((double)(float)linear_acceleration[0] + std::sin(pitch) * 9.81);
    acc3[1] = (float)((double)(float)linear_acceleration[1] - std::cos(pitch) * std::sin(roll) * 9.81);
    acc3[2] = (float)((double)(float)linear_acceleration[2] - std::cos(pitch) * std::cos(roll) * 9.81);
    for (int k = 0; k < 3; k++) ang_vel3[k] = (float)angular_velocity[k];
    quat_wxyz[0] = (float)w; quat_wxyz[1] = (float)x; quat_wxyz[2] = (float)y; quat_wxyz[3] = (float)z;
  }

  int push(const float* ang_vel3, const float* acc3, const float* quat_wxyz, double t) {
    if (last >= 0 && t < stamp[last]) return IMU_PUSH_OUT_OF_ORDER;
    float m[9];
    quat_to_matrix(quat_wxyz, m);
    const float roll = atan2f(m[7], m[8]);
    const float pitch = asinf(-m[6]);
    const float yaw = atan2f(m[3], m[0]);
    last = (last + 1) % IMU_QUEUE_LENGTH;
    count++;
    stamp[last] = t;
    rpy[last][0] = roll; rpy[last][1] = pitch; rpy[last][2] = yaw;
    for (int k = 0; k < 3; k++) { acc[last][k] = acc3[k]; ang_vel[last][k] = ang_vel3[k]; }
    float aw[3];   // acceleration in the world frame
    for (int r = 0; r < 3; r++) aw[r] = (m[3 * r] * acc3[0] + m[3 * r + 1] * acc3[1]) + m[3 * r + 2] * acc3[2];
    const int back = (last + IMU_QUEUE_LENGTH - 1) % IMU_QUEUE_LENGTH;
    const double dt = stamp[last] - stamp[back];
    if (dt < scan_period) {
      for (int k = 0; k < 3; k++) {
        shift[last][k] = (float)((double)shift[back][k] + (double)velo[back][k] * dt + (double)aw[k] * dt * dt * 0.5);
        velo[last][k] = (float)((double)velo[back][k] + (double)aw[k] * dt);
        ang_rot[last][k] = (float)((double)ang_rot[back][k] + (double)ang_vel3[k] * dt);
      }
    }   // else: the slot keeps what it held (a gap in the IMU stream restarts nothing)
    return IMU_PUSH_OK;
  }

  void entry_of_slot(int slot, ImuEntry* e) const {
    e->stamp = stamp[slot];
    for (int k = 0; k < 3; k++) { e->rpy[k] = rpy[slot][k]; e->shift[k] = shift[slot][k]; e->velo[k] = velo[slot][k]; }
    e->pad = 0.f;
  }

  // Entries of the table a scan sees: ring slots last_iter .. last in ring order (0 when last < 0).
  int table_size() const {
    if (last < 0) return 0;
    return ((last - last_iter) % IMU_QUEUE_LENGTH + IMU_QUEUE_LENGTH) % IMU_QUEUE_LENGTH + 1;
  }

  // table[0] = entry -1 (the slot in front of last_iter: what an interpolation at entry 0 reads), table[1 + k] = entry k.
  // `table` holds IMU_TABLE_MAX entries; returns m.
  int linearise(ImuEntry* table) const {
    const int m = table_size();
    entry_of_slot((last_iter + IMU_QUEUE_LENGTH - 1) % IMU_QUEUE_LENGTH, &table[0]);
    for (int k = 0; k < m; k++) entry_of_slot((last_iter + k) % IMU_QUEUE_LENGTH, &table[1 + k]);
    return m;
  }

  // the cursor a scan ended on (table entry) becomes the ring slot the next scan starts from
  void advance(int cursor_entry) { last_iter = (last_iter + cursor_entry) % IMU_QUEUE_LENGTH; }
};

}  // namespace lsr

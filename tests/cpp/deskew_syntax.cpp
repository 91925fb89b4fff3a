// The use_imu members of the C++ surface against the mock PCL / pclomp headers: compiled with -fsyntax-only by
// tests/test_deskew_cpu.py, which also checks that the block between the markers below is, verbatim, the block INTEGRATION.md shows.
#include <cstdint>
#include <vector>

#include <lidarslam_reg/gfx950_registration.hpp>
#include <lidarslam_reg/registration.hpp>

struct ImuMsg { double orientation[4], angular_velocity[3], linear_acceleration[3], stamp; };   // sensor_msgs/Imu, the fields used
struct CloudMsg { std::vector<uint8_t> data; uint32_t width, height, point_step; double stamp; };

// [deskew-snippet begin]
// scanmatcher_component.cpp:80 — once, where the node calls lidar_undistortion_.setScanPeriod(scan_period_)
void on_configure(Gfx950Registration<pcl::PointXYZI, pcl::PointXYZI>& reg, double scan_period) { reg.imuReset(scan_period); }

// scanmatcher_component.cpp:501-527 — the imu subscription's callback
void on_imu(Gfx950Registration<pcl::PointXYZI, pcl::PointXYZI>& reg, const ImuMsg& msg) {
  reg.receiveImu(msg.orientation, msg.angular_velocity, msg.linear_acceleration, msg.stamp);
}

// scanmatcher_component.cpp:204-218, 324-329 — the cloud callback with use_imu: the raw payload is de-skewed in place of
// adjustDistortion, and the de-skewed payload goes through range filter + VoxelGrid + setInputSource on the device
bool on_cloud(Gfx950Registration<pcl::PointXYZI, pcl::PointXYZI>& reg, CloudMsg& msg, double scan_min_range, double scan_max_range,
              float vg_size_for_input) {
  const lsr_pc2_layout layout = {msg.point_step, 0u, 4u, 8u, 16};              // from msg.fields
  const std::size_t n = (std::size_t)msg.width * msg.height;
  lsr_deskew_info info;
  if (!reg.deskewPointCloud2(msg.data.data(), n, layout, msg.stamp, msg.data.data(), /*on_device=*/false, &info)) return false;
  std::size_t kept = 0;
  return lsr_set_input_source_pc2(reg.handle(), msg.data.data(), n, &layout, scan_min_range, scan_max_range, vg_size_for_input, 0, &kept) == LSR_OK;
}
// [deskew-snippet end]

using Cloud = pcl::PointCloud<pcl::PointXYZI>;
bool host_api(lidarslam_reg::NormalDistributionsTransform<pcl::PointXYZI, pcl::PointXYZI, Cloud, Cloud>& ndt, CloudMsg& msg, const ImuMsg& imu) {
  ndt.imuReset();
  const bool ok = ndt.receiveImu(imu.orientation, imu.angular_velocity, imu.linear_acceleration, imu.stamp);
  const lsr_pc2_layout layout = {msg.point_step, 0u, 4u, 8u, -1};
  return ok && ndt.deskewPointCloud2(msg.data.data(), (std::size_t)msg.width * msg.height, layout, msg.stamp, msg.data.data());
}

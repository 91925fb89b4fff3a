// The sensor-mount and use_odom members of the C++ surface against the mock PCL / pclomp headers: compiled with -fsyntax-only by
// tests/test_sensor_transform_cpu.py, which also checks that the block between the markers below is, verbatim, the block INTEGRATION.md shows.
#include <cstdint>
#include <vector>

#include <lidarslam_reg/gfx950_registration.hpp>
#include <lidarslam_reg/registration.hpp>

struct TransformMsg { double translation[3], rotation[4]; };   // geometry_msgs/Transform: translation x y z, rotation x y z w
struct CloudMsg { std::vector<uint8_t> data; uint32_t width, height, point_step; double stamp; };

// [sensor-transform-snippet begin]
// scanmatcher_component.cpp:188-199 — the head of the cloud callback: what lookupTransform(robot_frame_id_, msg->header.frame_id)
// returned goes to the object instead of into tf2::doTransform; a static mount is set once
void on_sensor_transform(Gfx950Registration<pcl::PointXYZI, pcl::PointXYZI>& reg, const TransformMsg& t) {
  const lsr_sensor_transform tf = {{t.translation[0], t.translation[1], t.translation[2]}, {t.rotation[0], t.rotation[1], t.rotation[2], t.rotation[3]}};
  reg.setSensorTransform(tf);
}

// :195-218, 324-329 without IMU — the raw payload, still in the sensor frame, goes straight in: doTransform, fromROSMsg, the range
// filter, VoxelGrid and setInputSource are one call, and the transform costs no pass of its own
bool on_cloud(Gfx950Registration<pcl::PointXYZI, pcl::PointXYZI>& reg, const CloudMsg& msg, double scan_min_range, double scan_max_range,
              float vg_size_for_input) {
  const lsr_pc2_layout layout = {msg.point_step, 0u, 4u, 8u, 16};              // from msg.fields
  return reg.setInputSourcePointCloud2(msg.data.data(), (std::size_t)msg.width * msg.height, layout, scan_min_range, scan_max_range,
                                       vg_size_for_input);
}

// :195-208 with use_imu — adjustDistortion reads the TRANSFORMED cloud, so the payload is moved first, records -> records (in place
// here), then de-skewed, and the robot-frame payload goes in through the untransformed entry
bool on_cloud_imu(Gfx950Registration<pcl::PointXYZI, pcl::PointXYZI>& reg, CloudMsg& msg, const lsr_sensor_transform& tf,
                  double scan_min_range, double scan_max_range, float vg_size_for_input) {
  const lsr_pc2_layout layout = {msg.point_step, 0u, 4u, 8u, 16};
  const std::size_t n = (std::size_t)msg.width * msg.height;
  if (!reg.transformPointCloud2(msg.data.data(), n, layout, tf, msg.data.data())) return false;
  if (!reg.deskewPointCloud2(msg.data.data(), n, layout, msg.stamp, msg.data.data())) return false;
  std::size_t kept = 0;
  return lsr_set_input_source_pc2(reg.handle(), msg.data.data(), n, &layout, scan_min_range, scan_max_range, vg_size_for_input, 0, &kept) == LSR_OK;
}

// :333-348 — use_odom: odom_mat is tf2::transformToEigen(lookupTransform(odom_frame_id_, robot_frame_id_, stamp)).matrix().cast<float>()
Eigen::Matrix4f guess_with_odom(const Eigen::Matrix4f& sim_trans, Eigen::Matrix4f& previous_odom_mat, const Eigen::Matrix4f& odom_mat) {
  const Eigen::Matrix4f guess = Gfx950Registration<pcl::PointXYZI, pcl::PointXYZI>::odomGuess(sim_trans, previous_odom_mat, odom_mat);
  previous_odom_mat = odom_mat;                                                // :347
  return guess;                                                                // registration_->align(*output_cloud, guess), :353
}
// [sensor-transform-snippet end]

using Cloud = pcl::PointCloud<pcl::PointXYZI>;
using HostNdt = lidarslam_reg::NormalDistributionsTransform<pcl::PointXYZI, pcl::PointXYZI, Cloud, Cloud>;
bool host_api(HostNdt& ndt, CloudMsg& msg, const lsr_sensor_transform& tf) {
  const lsr_pc2_layout layout = {msg.point_step, 0u, 4u, 8u, -1};
  const std::size_t n = (std::size_t)msg.width * msg.height;
  ndt.setSensorTransform(tf);
  std::size_t kept = 0;
  bool ok = ndt.setInputSourcePointCloud2(msg.data.data(), n, layout, 0.1, 100.0, 0.2f, false, &kept);
  ndt.clearSensorTransform();
  ok = ok && ndt.transformPointCloud2(msg.data.data(), n, layout, tf, msg.data.data());
  const lidarslam_reg::Matrix4f I = lidarslam_reg::Matrix4f::Identity();
  const lidarslam_reg::Matrix4f g = HostNdt::odomGuess(I, I, I);
  return ok && g(0, 0) == 1.f;
}

// TEST INFRASTRUCTURE: the call site INTEGRATION.md §3g shows replaced — `if (do_save_map) {pcl::io::savePCDFileASCII("map.pcd",
// *map_ptr);}` at the end of doPoseAdjustment (graph_based_slam_component.cpp:369) — compiled against include/lidarslam_reg/pcd_io.hpp
// and linked against the library by tests/test_pcd_ascii_cpu.py, which also checks that the block between the markers below is,
// verbatim, the block INTEGRATION.md shows.  The mock message and Eigen types carry only the members the snippet touches; toSubmaps
// is the helper of §3e (tests/cpp/map_snippets.cpp).
#include <lidarslam_reg/pcd_io.hpp>

#include <cstdint>
#include <string>
#include <vector>

namespace mock {
struct Point { double x, y, z; };
struct Quat { double x, y, z, w; };
struct Pose { Point position; Quat orientation; };
struct PointCloud2 {
  uint32_t height = 1, width = 0;
  std::vector<uint8_t> data;
};
struct SubMap { double distance = 0; Pose pose; PointCloud2 cloud; };
struct MapArray { std::vector<SubMap> submaps; };
struct Matrix4d { double m[16]; const double* data() const { return m; } };
struct Isometry3d { Matrix4d mat; Matrix4d matrix() const { return mat; } };   // Eigen::Isometry3d: matrix().data()
}  // namespace mock
namespace Eigen { using mock::Isometry3d; }
namespace lidarslam_msgs { namespace msg { using mock::MapArray; } }

static std::vector<lsr_submap> toSubmaps(const lidarslam_msgs::msg::MapArray & map_array_msg) {
  std::vector<lsr_submap> sm(map_array_msg.submaps.size());
  for (size_t i = 0; i < sm.size(); i++) {
    const auto & m = map_array_msg.submaps[i];
    sm[i] = {{m.pose.position.x, m.pose.position.y, m.pose.position.z},
             {m.pose.orientation.x, m.pose.orientation.y, m.pose.orientation.z, m.pose.orientation.w},
             m.distance, m.cloud.data.data(), (size_t)m.cloud.width * m.cloud.height};
  }
  return sm;
}

struct Backend {
  lsr_handle handle_;
  void saveMap(const lidarslam_msgs::msg::MapArray & map_array_msg, const std::vector<Eigen::Isometry3d> & estimates, bool do_save_map);
};

void Backend::saveMap(const lidarslam_msgs::msg::MapArray & map_array_msg, const std::vector<Eigen::Isometry3d> & estimates, bool do_save_map)
{
  // [pcd-snippet begin: save_map]
  // graph_based_slam_component.cpp:369 — if (do_save_map) {pcl::io::savePCDFileASCII("map.pcd", *map_ptr);} // too heavy
  // the submaps are moved by the optimiser's estimates into a map that stays on the device, its text is formatted there,
  // and this thread writes one piece to the file while the next one is formatted: the same bytes, no PCL writer
  if (do_save_map) {
    if (!lidarslam_reg::saveMapPCD(handle_, "map.pcd", toSubmaps(map_array_msg), estimates.data())) {return;}
  }
  // [pcd-snippet end: save_map]
}

int main() {
  // without a handle the call is refused by the argument check, before any device or file is touched: the helper reports and returns false
  lidarslam_msgs::msg::MapArray map_array_msg;
  map_array_msg.submaps.resize(1);
  std::vector<Eigen::Isometry3d> estimates(1);
  Backend backend{nullptr};
  backend.saveMap(map_array_msg, estimates, true);
  const bool ok = lidarslam_reg::saveMapPCD(nullptr, "map.pcd", toSubmaps(map_array_msg), estimates.data());
  const float one = 1.0f;
  const bool ok2 = lidarslam_reg::savePCDFileASCII(nullptr, "never_written.pcd", &one, 0);
  std::FILE* f = std::fopen("never_written.pcd", "rb");
  std::printf("PCD_SNIPPETS refused=%d refused_payload=%d file=%d\n", ok ? 0 : 1, ok2 ? 0 : 1, f ? 1 : 0);
  if (f) std::fclose(f);
  return (ok || ok2 || f) ? 1 : 0;
}

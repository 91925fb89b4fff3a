// TEST INFRASTRUCTURE: the publishMap and `do_save_map` call sites of INTEGRATION.md §3i with a leaf size — compiled against
// include/lidarslam_reg/map_assembly.hpp and pcd_io.hpp and linked against the library by tests/test_map_filter_cpu.py, which also
// checks that the blocks between the markers below are, verbatim, the blocks INTEGRATION.md shows.  The mock types are those of
// tests/cpp/pcd_write_snippets.cpp.
#include <lidarslam_reg/map_assembly.hpp>
#include <lidarslam_reg/pcd_io.hpp>

#include <cstdint>
#include <string>
#include <vector>

namespace mock {
struct Point { double x, y, z; };
struct Quat { double x, y, z, w; };
struct Pose { Point position; Quat orientation; };
struct PointCloud2 {
  uint32_t height = 1, width = 0, point_step = 0, row_step = 0;
  std::vector<uint8_t> data;
};
struct SubMap { double distance = 0; Pose pose; PointCloud2 cloud; };
struct MapArray { std::vector<SubMap> submaps; };
struct Matrix4d { double m[16]; const double* data() const { return m; } };
struct Isometry3d { Matrix4d mat; Matrix4d matrix() const { return mat; } };   // Eigen::Isometry3d: matrix().data()
}  // namespace mock
namespace Eigen { using mock::Isometry3d; }
namespace lidarslam_msgs { namespace msg { using mock::MapArray; } }
namespace sensor_msgs { namespace msg { using mock::PointCloud2; } }

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

struct Node {
  lsr_handle handle_;
  float map_leaf_size_ = 0.1f;
  bool publishMap(const lidarslam_msgs::msg::MapArray & map_array_msg, sensor_msgs::msg::PointCloud2 & map_msg);
  bool saveMap(const lidarslam_msgs::msg::MapArray & map_array_msg, const std::vector<Eigen::Isometry3d> & estimates, bool do_save_map);
};

bool Node::publishMap(const lidarslam_msgs::msg::MapArray & map_array_msg, sensor_msgs::msg::PointCloud2 & map_msg)
{
  // [map-filter-snippet begin: publish_map]
  // publishMap (scanmatcher_component.cpp:529-552) with the map thinned before it leaves the device: every submap moved by its
  // pose, pcl::VoxelGrid(map_leaf_size_) over the whole map with a 64-bit leaf index, one PointXYZI record per occupied leaf
  if (!lidarslam_reg::assembleMapFiltered(handle_, toSubmaps(map_array_msg), static_cast<const double *>(nullptr), map_leaf_size_,
                                          map_msg.data)) {return false;}
  map_msg.point_step = 32;
  map_msg.height = 1;
  map_msg.width = (uint32_t)(map_msg.data.size() / 32);
  map_msg.row_step = 32 * map_msg.width;
  // [map-filter-snippet end: publish_map]
  return true;
}

bool Node::saveMap(const lidarslam_msgs::msg::MapArray & map_array_msg, const std::vector<Eigen::Isometry3d> & estimates, bool do_save_map)
{
  // [map-filter-snippet begin: save_map]
  // the map half of doPoseAdjustment (graph_based_slam_component.cpp:321-369): the submaps moved by the optimiser's estimates,
  // thinned on the device, written as DATA binary_compressed
  if (do_save_map) {
    if (!lidarslam_reg::saveMapPCDFiltered(handle_, "map.pcd", toSubmaps(map_array_msg), estimates.data(), map_leaf_size_,
                                           LSR_PCD_BINARY_COMPRESSED)) {return false;}
  }
  // [map-filter-snippet end: save_map]
  return true;
}

int main() {
  // without a handle every call is refused by the argument check, before any device or file is touched
  lidarslam_msgs::msg::MapArray map_array_msg;
  map_array_msg.submaps.resize(1);
  std::vector<Eigen::Isometry3d> estimates(1);
  sensor_msgs::msg::PointCloud2 map_msg;
  map_msg.data.assign(7, 1);
  Node node{nullptr};
  int refused = 0;
  refused += node.publishMap(map_array_msg, map_msg) ? 0 : 1;
  const int emptied = map_msg.data.empty() ? 1 : 0;
  refused += node.saveMap(map_array_msg, estimates, true) ? 0 : 1;
  const float one[8] = {1.0f, 1.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  std::vector<uint8_t> payload(3, 1);
  refused += lidarslam_reg::voxelGridFilterMap(nullptr, one, 1, 0.1f, payload) ? 0 : 1;
  size_t n = 0;
  refused += lidarslam_reg::assembleMapFilteredDevice(nullptr, toSubmaps(map_array_msg), nullptr, 0.1f, nullptr, 0, &n) ? 0 : 1;
  refused += lidarslam_reg::assembleMapFiltered(nullptr, toSubmaps(map_array_msg), estimates.data(), 0.1f, payload) ? 0 : 1;
  refused += lidarslam_reg::saveMapPCDFiltered(nullptr, "map.pcd", toSubmaps(map_array_msg), static_cast<const double*>(nullptr), 0.1f) ? 0 : 1;
  std::FILE* f = std::fopen("map.pcd", "rb");
  std::printf("MAP_FILTER_SNIPPETS refused=%d emptied=%d payload=%d file=%d\n", refused, emptied, (int)payload.size(), f ? 1 : 0);
  if (f) std::fclose(f);
  return (refused != 6 || !emptied || !payload.empty() || f) ? 1 : 0;
}

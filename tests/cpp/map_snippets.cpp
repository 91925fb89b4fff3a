// TEST INFRASTRUCTURE: the two call sites INTEGRATION.md §3e shows replaced — ScanMatcherComponent::publishMap
// (scanmatcher_component.cpp:529-552) and the map half of doPoseAdjustment (graph_based_slam_component.cpp:321-368) — compiled against
// include/lidarslam_reg/map_assembly.hpp and linked against the library by tests/test_map_assembly_cpu.py, which also checks that the
// blocks between the markers below are, verbatim, the blocks INTEGRATION.md shows.  The mock message, g2o and Eigen types carry only
// the members the snippets touch.
#include <lidarslam_reg/map_assembly.hpp>

#include <array>
#include <cstdint>
#include <string>
#include <vector>

namespace mock {
struct Header { std::string frame_id; };
struct Point { double x, y, z; };
struct Quat { double x, y, z, w; };
struct Pose { Point position; Quat orientation; };
struct PoseStamped { Header header; Pose pose; };
struct Path { Header header; std::vector<PoseStamped> poses; };
struct PointField { std::string name; uint32_t offset; uint8_t datatype; uint32_t count; };
struct PointCloud2 {
  Header header;
  uint32_t height = 1, width = 0, point_step = 32, row_step = 0;
  std::vector<PointField> fields;
  bool is_bigendian = false, is_dense = true;
  std::vector<uint8_t> data;
};
struct SubMap { Header header; double distance = 0; Pose pose; PointCloud2 cloud; };
struct MapArray { Header header; std::vector<SubMap> submaps; };
template <typename T> struct Publisher { void publish(const T&) {} };
struct Matrix4d { double m[16]; const double* data() const { return m; } };
struct Affine3d { Matrix4d mat; Matrix4d matrix() const { return mat; } };                 // Eigen::Affine3d: matrix().data()
struct VertexSE3 { Affine3d est; Affine3d estimate() const { return est; } };                // g2o::VertexSE3
struct Optimizer { std::vector<VertexSE3> v; VertexSE3* vertex(int i) { return &v[i]; } };   // g2o::SparseOptimizer
inline Pose toMsg(const Affine3d& a) { return Pose{{a.mat.m[12], a.mat.m[13], a.mat.m[14]}, {0, 0, 0, 1}}; }   // tf2::toMsg
}  // namespace mock
namespace tf2 { using mock::toMsg; }
namespace Eigen { using mock::Affine3d; }
namespace g2o { using mock::VertexSE3; }
namespace lidarslam_msgs { namespace msg { using mock::MapArray; using mock::SubMap; } }
namespace nav_msgs { namespace msg { using mock::Path; } }
namespace geometry_msgs { namespace msg { using mock::Pose; using mock::PoseStamped; } }
namespace sensor_msgs { namespace msg { using mock::PointCloud2; } }
#define RCLCPP_ERROR(logger, fmt, ...) std::fprintf(stderr, fmt "\n", __VA_ARGS__)
#define RCLCPP_INFO(logger, fmt, ...) std::fprintf(stderr, fmt "\n", __VA_ARGS__)

// [map-snippet begin: helpers]
// the submaps of a MapArray as the C ABI takes them (the same records lsr_search_loop takes)
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
// what pcl::toROSMsg fills in around the data of a pcl::PointXYZI cloud
static void describeXYZI(sensor_msgs::msg::PointCloud2 & msg, size_t n_points) {
  msg.height = 1; msg.width = (uint32_t)n_points; msg.point_step = 32; msg.row_step = 32 * msg.width;
  msg.is_bigendian = false; msg.is_dense = true;
  msg.fields = {{"x", 0, 7, 1}, {"y", 4, 7, 1}, {"z", 8, 7, 1}, {"intensity", 16, 7, 1}};   // 7 = FLOAT32
}
// [map-snippet end: helpers]

struct Frontend {
  lsr_handle handle_;
  mock::Publisher<sensor_msgs::msg::PointCloud2> * map_pub_;
  int get_logger() { return 0; }
  void publishMap(const lidarslam_msgs::msg::MapArray & map_array_msg, const std::string & map_frame_id);
};

// [map-snippet begin: publish_map]
void Frontend::publishMap(const lidarslam_msgs::msg::MapArray & map_array_msg, const std::string & map_frame_id)
{
  // scanmatcher_component.cpp:529-552 — every submap moved by its own pose, the records concatenated: one call, on the device
  sensor_msgs::msg::PointCloud2 map_msg;
  if (!lidarslam_reg::assembleMap(handle_, toSubmaps(map_array_msg), static_cast<const double *>(nullptr), map_msg.data)) {return;}
  describeXYZI(map_msg, map_msg.data.size() / 32);
  RCLCPP_INFO(get_logger(), "publish a map, number of points in the map : %ld", (long)map_msg.width);
  map_msg.header.frame_id = map_frame_id;
  map_pub_->publish(map_msg);
}
// [map-snippet end: publish_map]

struct Backend {
  lsr_handle handle_;
  mock::Publisher<lidarslam_msgs::msg::MapArray> * modified_map_array_pub_;
  mock::Publisher<nav_msgs::msg::Path> * modified_path_pub_;
  mock::Publisher<sensor_msgs::msg::PointCloud2> * modified_map_pub_;
  void publishModifiedMap(const lidarslam_msgs::msg::MapArray & map_array_msg, mock::Optimizer & optimizer);
};

void Backend::publishModifiedMap(const lidarslam_msgs::msg::MapArray & map_array_msg, mock::Optimizer & optimizer)
{
  const int submaps_size = (int)map_array_msg.submaps.size();
  // [map-snippet begin: pose_adjustment]
  /* modified_map publish (graph_based_slam_component.cpp:321-368; g2o above this line is unchanged) */
  lidarslam_msgs::msg::MapArray modified_map_array_msg;
  modified_map_array_msg.header = map_array_msg.header;
  nav_msgs::msg::Path path;
  path.header.frame_id = "map";
  std::vector<Eigen::Affine3d> estimates(submaps_size);
  for (int i = 0; i < submaps_size; i++) {
    estimates[i] = static_cast<g2o::VertexSE3 *>(optimizer.vertex(i))->estimate();
  }
  // every submap moved by the optimiser's estimate, all of them in one launch; first_record says where each one lies in the map
  sensor_msgs::msg::PointCloud2 map_msg;
  std::vector<size_t> first_record;
  if (!lidarslam_reg::assembleMap(handle_, toSubmaps(map_array_msg), estimates.data(), map_msg.data, &first_record)) {return;}
  for (int i = 0; i < submaps_size; i++) {
    lidarslam_msgs::msg::SubMap submap;
    submap.header = map_array_msg.submaps[i].header;
    submap.pose = tf2::toMsg(estimates[i]);
    submap.cloud.data.assign(map_msg.data.begin() + 32 * first_record[i], map_msg.data.begin() + 32 * first_record[i + 1]);
    describeXYZI(submap.cloud, first_record[i + 1] - first_record[i]);
    modified_map_array_msg.submaps.push_back(submap);
    geometry_msgs::msg::PoseStamped pose_stamped;
    pose_stamped.header = submap.header;
    pose_stamped.pose = submap.pose;
    path.poses.push_back(pose_stamped);
  }
  modified_map_array_pub_->publish(modified_map_array_msg);
  modified_path_pub_->publish(path);
  describeXYZI(map_msg, first_record[submaps_size]);
  map_msg.header.frame_id = "map";
  modified_map_pub_->publish(map_msg);
  // [map-snippet end: pose_adjustment]
}

// a frontend that keeps its published map resident: the new keyframes only, behind the records the buffer already holds
bool extendResidentMap(lsr_handle h, const std::vector<lsr_submap>& new_submaps_on_device, unsigned char* d_map, size_t capacity_points,
                       size_t& held_points) {
  size_t added = 0;
  if (!lidarslam_reg::assembleMapDevice(h, new_submaps_on_device, nullptr, d_map + 32 * held_points, capacity_points - held_points, &added)) return false;
  held_points += added;
  return true;
}

int main() {
  // without a handle the call is refused by the argument check, before any device is touched: the adapter reports and returns false
  std::vector<uint8_t> payload(3, 1);
  std::vector<lsr_submap> none(1);
  std::memset(none.data(), 0, sizeof(lsr_submap));
  const bool ok = lidarslam_reg::assembleMap(nullptr, none, static_cast<const double*>(nullptr), payload);
  std::printf("MAP_SNIPPETS refused=%d payload=%zu\n", ok ? 0 : 1, payload.size());
  return ok ? 1 : 0;
}

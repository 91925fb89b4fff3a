// TEST INFRASTRUCTURE: the call site INTEGRATION.md §3f shows — GraphBasedSlamComponent::doPoseAdjustment
// (graph_based_slam_component.cpp:262-371) with g2o removed — compiled against include/lidarslam_reg/pose_graph.hpp and
// include/lidarslam_reg/map_assembly.hpp and linked against the library by tests/test_pose_graph_cpu.py, which also checks that the block
// between the markers below is, verbatim, the block INTEGRATION.md shows.  The mock message and Eigen types carry only the members the
// snippet touches.
#include <lidarslam_reg/map_assembly.hpp>
#include <lidarslam_reg/pose_graph.hpp>

#include <cstdint>
#include <string>
#include <utility>
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
struct Matrix4d {
  double m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double* data() const { return m; }
  double* data() { return m; }
};
// Eigen::Affine3d / Eigen::Isometry3d: matrix().data(), const and mutable; constructible from a 4x4
struct Transform3d {
  Matrix4d mat;
  Transform3d() = default;
  explicit Transform3d(const Matrix4d& M) : mat(M) {}
  const Matrix4d& matrix() const { return mat; }
  Matrix4d& matrix() { return mat; }
};
// Eigen::fromMsg(geometry_msgs::Pose, Affine3d): the translation is enough for a compile-and-link check
inline void fromMsg(const Pose& p, Transform3d& a) { a = Transform3d(); a.mat.m[12] = p.position.x; a.mat.m[13] = p.position.y; a.mat.m[14] = p.position.z; }
inline Pose toMsg(const Transform3d& a) { return Pose{{a.mat.m[12], a.mat.m[13], a.mat.m[14]}, {0, 0, 0, 1}}; }   // tf2::toMsg
}  // namespace mock
namespace tf2 { using mock::toMsg; }
namespace Eigen { using Affine3d = mock::Transform3d; using Isometry3d = mock::Transform3d; using mock::fromMsg; }
namespace lidarslam_msgs { namespace msg { using mock::MapArray; using mock::SubMap; } }
namespace nav_msgs { namespace msg { using mock::Path; } }
namespace geometry_msgs { namespace msg { using mock::Pose; using mock::PoseStamped; } }
namespace sensor_msgs { namespace msg { using mock::PointCloud2; } }
#define RCLCPP_INFO(logger, fmt, ...) std::fprintf(stderr, fmt "\n", __VA_ARGS__)

// the two helpers of INTEGRATION.md §3e (tests/cpp/map_snippets.cpp)
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
static void describeXYZI(sensor_msgs::msg::PointCloud2 & msg, size_t n_points) {
  msg.height = 1; msg.width = (uint32_t)n_points; msg.point_step = 32; msg.row_step = 32 * msg.width;
  msg.is_bigendian = false; msg.is_dense = true;
  msg.fields = {{"x", 0, 7, 1}, {"y", 4, 7, 1}, {"z", 8, 7, 1}, {"intensity", 16, 7, 1}};   // 7 = FLOAT32
}

struct LoopEdge { std::pair<int, int> pair_id; Eigen::Isometry3d relative_pose; };   // graph_based_slam_component.h

struct Backend {
  lsr_handle handle_;
  int num_adjacent_pose_cnstraints_ = 5;
  std::vector<LoopEdge> loop_edges_;
  mock::Publisher<lidarslam_msgs::msg::MapArray> * modified_map_array_pub_;
  mock::Publisher<nav_msgs::msg::Path> * modified_path_pub_;
  mock::Publisher<sensor_msgs::msg::PointCloud2> * modified_map_pub_;
  int get_logger() { return 0; }
  void doPoseAdjustment(lidarslam_msgs::msg::MapArray map_array_msg, bool do_save_map);
};

// [pose-graph-snippet begin: do_pose_adjustment]
void Backend::doPoseAdjustment(lidarslam_msgs::msg::MapArray map_array_msg, bool do_save_map)
{
  // graph_based_slam_component.cpp:267-319 without g2o: the vertices are the stored poses (vertex 0 fixed), ...
  int submaps_size = map_array_msg.submaps.size();
  std::vector<Eigen::Isometry3d> poses(submaps_size);
  for (int i = 0; i < submaps_size; i++) {
    Eigen::Affine3d affine;
    Eigen::fromMsg(map_array_msg.submaps[i].pose, affine);
    poses[i] = Eigen::Isometry3d(affine.matrix());
  }
  // ... the edges are num_adjacent_pose_cnstraints_ odometry edges into every vertex i > num_adjacent_pose_cnstraints_ (:289-303) ...
  std::vector<lsr_pose_edge> edges;
  if (!lidarslam_reg::adjacentPoseEdges(poses, num_adjacent_pose_cnstraints_, edges)) {return;}
  /* loop edge */
  for (auto loop_edge : loop_edges_) {
    edges.push_back(lidarslam_reg::poseEdge(loop_edge.pair_id.first, loop_edge.pair_id.second, loop_edge.relative_pose));
  }
  // ... and optimizer.optimize(10) runs on the device (identity information, Levenberg-Marquardt as g2o runs it)
  std::vector<Eigen::Isometry3d> estimates;
  lsr_pose_graph_result result;
  if (!lidarslam_reg::optimizePoseGraph(handle_, poses, edges, estimates, &result)) {return;}
  RCLCPP_INFO(get_logger(), "pose graph: %d iterations, chi2 %g -> %g", result.iterations, result.chi2_before, result.chi2_after);
  // optimizer.save("pose_graph.g2o") (:319) stays the caller's: VERTEX_SE3:QUAT / EDGE_SE3:QUAT lines from `estimates` and `edges`

  /* modified_map publish (:321-368, INTEGRATION.md 3e with `estimates` straight from the call above) */
  lidarslam_msgs::msg::MapArray modified_map_array_msg;
  modified_map_array_msg.header = map_array_msg.header;
  nav_msgs::msg::Path path;
  path.header.frame_id = "map";
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
  (void)do_save_map;   // pcl::io::savePCDFileASCII("map.pcd", ...) (:369) stays as it is
}
// [pose-graph-snippet end: do_pose_adjustment]

int main() {
  // the odometry edges need no device: 8 poses one metre apart, k = 5 -> vertices 6 and 7 get five edges each
  std::vector<Eigen::Isometry3d> poses(8);
  for (int i = 0; i < 8; i++) poses[i].matrix().data()[12] = (double)i;
  std::vector<lsr_pose_edge> edges;
  const bool made = lidarslam_reg::adjacentPoseEdges(poses, 5, edges);
  const bool shape = made && edges.size() == 10 && edges[0].from == 1 && edges[0].to == 6 && edges[0].measurement[12] == 5.0 &&
                     edges[9].from == 6 && edges[9].to == 7 && edges[9].measurement[12] == 1.0;
  // without a handle the optimiser is refused by the argument check, before any device is touched: the adapter reports and returns
  // false, and the output vector stays as it was
  std::vector<Eigen::Isometry3d> estimates(3);
  const bool ok = lidarslam_reg::optimizePoseGraph(nullptr, poses, edges, estimates);
  std::printf("POSE_GRAPH_SNIPPETS edges=%zu shape=%d refused=%d kept=%zu\n", edges.size(), shape ? 1 : 0, ok ? 0 : 1, estimates.size());
  return (shape && !ok) ? 0 : 1;
}

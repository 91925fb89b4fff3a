// TEST INFRASTRUCTURE: the `do_save_map` call site of INTEGRATION.md §3g with a body kind — compiled against
// include/lidarslam_reg/pcd_io.hpp and linked against the library by tests/test_pcd_write_cpu.py, which also checks that the block
// between the markers below is, verbatim, the block INTEGRATION.md shows.  The mock types are those of tests/cpp/pcd_snippets.cpp.
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
  // [pcd-snippet begin: save_map_compressed]
  // DATA binary_compressed: the map's field-major image is compressed in HBM chunk by chunk (LZF), then written piece by piece;
  // LSR_PCD_BINARY writes packed 16-byte records instead.  pcl::io::loadPCDFile and lsr_load_pcd read both.
  if (do_save_map) {
    if (!lidarslam_reg::saveMapPCD(handle_, "map.pcd", toSubmaps(map_array_msg), estimates.data(), false,
                                   LSR_PCD_BINARY_COMPRESSED)) {return;}
  }
  // [pcd-snippet end: save_map_compressed]
}

int main() {
  // without a handle every call is refused by the argument check, before any device or file is touched
  lidarslam_msgs::msg::MapArray map_array_msg;
  map_array_msg.submaps.resize(1);
  std::vector<Eigen::Isometry3d> estimates(1);
  Backend backend{nullptr};
  backend.saveMap(map_array_msg, estimates, true);
  int refused = 0;
  for (int kind : {(int)LSR_PCD_ASCII, (int)LSR_PCD_BINARY, (int)LSR_PCD_BINARY_COMPRESSED, 3})
    refused += lidarslam_reg::saveMapPCD(nullptr, "map.pcd", toSubmaps(map_array_msg), estimates.data(), false, kind) ? 0 : 1;
  const float one[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  const lsr_pc2_layout packed{16u, 0u, 4u, 8u, 12};
  refused += lidarslam_reg::savePCDFileBinary(nullptr, "never_written.pcd", one, 1, packed) ? 0 : 1;
  refused += lidarslam_reg::savePCDFileBinaryCompressed(nullptr, "never_written.pcd", one, 1, packed) ? 0 : 1;
  std::FILE* f = std::fopen("never_written.pcd", "rb");
  std::printf("PCD_WRITE_SNIPPETS refused=%d file=%d\n", refused, f ? 1 : 0);
  if (f) std::fclose(f);
  return (refused != 6 || f) ? 1 : 0;
}

// TEST INFRASTRUCTURE: the localisation-side call site INTEGRATION.md §3h shows — a node that registers scans against a map saved by
// an earlier session (`map.pcd`, graph_based_slam_component.cpp:369) — compiled against include/lidarslam_reg/pcd_io.hpp and linked
// against the library by tests/test_pcd_read_cpu.py, which also checks that the block between the markers below is, verbatim, the block
// INTEGRATION.md shows.
#include <lidarslam_reg/pcd_io.hpp>

#include <cstdint>
#include <string>
#include <vector>

struct Localizer {
  lsr_handle handle_;
  std::vector<uint8_t> map_payload_;   // sensor_msgs::msg::PointCloud2::data of the map, for a publisher
  size_t map_points_ = 0;
  bool loadMap(const std::string & map_path, bool publish_map);
};

bool Localizer::loadMap(const std::string & map_path, bool publish_map)
{
  // [pcd-snippet begin: load_map]
  // the map an earlier session saved (pcl::io::savePCDFileASCII, or lsr_save_map_pcd_ascii) becomes the registration target:
  // this thread reads the file piece by piece while the device cuts the piece before into lines and parses them; the records
  // stay in HBM and go straight into setInputTarget — no pcl::io::loadPCDFile, no strtof on the host
  if (!lidarslam_reg::setInputTargetPCD(handle_, map_path, &map_points_)) {return false;}
  // a publisher that wants the map on the host reads it the same way, as a PointCloud2 payload of pcl::PointXYZI records
  if (publish_map) {
    if (!lidarslam_reg::loadPCDFile(handle_, map_path, map_payload_)) {return false;}
  }
  // [pcd-snippet end: load_map]
  return true;
}

int main() {
  // without a handle both calls are refused by the argument check, before any device or file is touched: the helpers report and
  // return false, and the payload stays as it was
  Localizer loc{nullptr};
  loc.map_payload_.assign(3, 7);
  const bool ok = loc.loadMap("no_such_map.pcd", true);
  std::vector<uint8_t> payload(2, 9);
  const bool ok2 = lidarslam_reg::loadPCDFile(nullptr, "no_such_map.pcd", payload);
  // the header parser needs no handle
  const char head[] = "VERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nWIDTH 5\nDATA ascii\n1 2 3\n";
  lsr_pcd_info info;
  const int st = lsr_parse_pcd_header(head, sizeof(head) - 1, &info);
  std::printf("PCD_READ_SNIPPETS refused=%d refused_payload=%d kept=%d header=%d points=%d offset=%d\n", ok ? 0 : 1, ok2 ? 0 : 1,
              (loc.map_payload_.size() == 3 && payload.size() == 2) ? 1 : 0, st, (int)info.n_points, (int)info.data_offset);
  return (ok || ok2 || st != LSR_OK) ? 1 : 0;
}

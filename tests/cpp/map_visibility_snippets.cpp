// TEST INFRASTRUCTURE: the map half of doPoseAdjustment without what moved, INTEGRATION.md §3m — compiled against
// include/lidarslam_reg/map_visibility.hpp and linked against the library; main() runs what needs no device: the pair table and the
// refusals.
#include <lidarslam_reg/map_visibility.hpp>

#include <cmath>
#include <cstdio>

namespace {
struct Backend {
  lsr_handle registration = nullptr;
  std::vector<lsr_submap> submaps;              // the MapArray so far, pose-local pcl::PointXYZI records
  lidarslam_reg::DepthImageTable depth_images;  // one eroded depth image per submap, extended as submaps arrive
  std::vector<unsigned char> map_records;       // *map_ptr, pcl::PointXYZI records
  size_t n_removed = 0;

  // [map-visibility-snippet begin: static_map]
  bool modifiedMap(const std::vector<double>& optimised_poses16) {
    if (!depth_images.update(registration, submaps)) return false;       // the new keyframes' images, one launch and one erosion
    std::vector<size_t> first_record;                                     // submap i's cloud: records first_record[i] .. [i + 1]
    return lidarslam_reg::assembleStaticMap(registration, submaps, depth_images, map_records, optimised_poses16.data(), &first_record,
                                            &n_removed);
  }
  // [map-visibility-snippet end: static_map]
};
}  // namespace

int main() {
  int ok = 0, refused = 0;
  const lsr_visibility_params p = lidarslam_reg::visibilityDefaults();
  lsr_submap s[3] = {};
  for (int i = 0; i < 3; i++) s[i].orientation[3] = 1.0;
  s[1].position[0] = 3.0;
  s[2].position[0] = 100.0;   // out of keyframe_range of both
  int32_t first[4], other[6];
  float rel[72];
  size_t n_pairs = 0;
  if (lsr_visibility_pairs(s, 3, nullptr, &p, first, other, rel, 6, &n_pairs) == LSR_OK && n_pairs == 2 && first[1] == 1 && first[2] == 2 &&
      first[3] == 2 && other[0] == 1 && other[1] == 0 && std::fabs(rel[3] + 3.0f) < 1e-6f && std::fabs(rel[12 + 3] - 3.0f) < 1e-6f)
    ok++;
  lsr_visibility_params bad = p;
  bad.face_width = 9;
  if (lsr_visibility_pairs(s, 3, nullptr, &bad, first, other, rel, 6, &n_pairs) == LSR_ERR_INVALID_ARGUMENT) refused++;
  if (lsr_visibility_pairs(s, 3, nullptr, &p, first, other, rel, 1, &n_pairs) == LSR_ERR_INVALID_ARGUMENT && n_pairs == 2) refused++;
  Backend backend;                                  // no object: the build refuses, the table stays empty
  backend.submaps.push_back(s[0]);
  std::vector<double> poses(16, 0.0);
  poses[0] = poses[5] = poses[10] = poses[15] = 1.0;
  if (!backend.modifiedMap(poses) && backend.depth_images.count == 0 && backend.map_records.empty()) refused++;
  std::printf("MAP_VISIBILITY_SNIPPETS ok=%d refused=%d\n", ok, refused);
  return (ok == 1 && refused == 3) ? 0 : 1;
}

// TEST INFRASTRUCTURE: the relocalisation of INTEGRATION.md §3k — compiled against include/lidarslam_reg.h and registration.hpp and
// linked against the library by tests/test_pose_search_cpu.py, which also checks that the block between the markers below is,
// verbatim, the block INTEGRATION.md shows.
#include <lidarslam_reg/registration.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace mock {
struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };
struct Cloud { std::vector<PointXYZI> points; };
}  // namespace mock
using Ndt = lidarslam_reg::NormalDistributionsTransform<mock::PointXYZI, mock::PointXYZI, mock::Cloud, mock::Cloud>;

// the C ABI: `h` holds the window of the map around center16 as target and the scan as source
static int relocalise(lsr_handle h, const float * center16, float * pose16)
{
  // [pose-search-snippet begin: relocalise]
  // the parking position is known to +-10 m, the heading not at all: 21 x 21 positions at 1 m, 72 headings at 5 degrees; the 16
  // distinct best (0.9 m or 7.5 degrees apart) are refined by the object's own NDT schedule as one candidate set
  lsr_pose_search_params prm = {};
  prm.lattice.n[0] = 21; prm.lattice.n[1] = 21; prm.lattice.n[2] = 1;
  prm.lattice.step[0] = prm.lattice.step[1] = prm.lattice.step[2] = 1.0;
  prm.lattice.n_yaw = 72;
  prm.lattice.yaw_step = 5.0 * M_PI / 180.0;
  prm.top_k = 16;
  prm.min_sep_m = 0.9;
  prm.min_sep_rad = 7.5 * M_PI / 180.0;
  lsr_result result;
  lsr_pose_search_report report;
  int st = lsr_ndt_search_pose(h, center16, &prm, pose16, &result, &report);
  if (st != LSR_OK) {return st;}                      // lsr_last_error() says why
  if (report.n_kept == 0) {return LSR_ERR_NO_TARGET;}  // no pose of the lattice puts a scan point into a map voxel: pose16 is untouched
  // pose16 = the winner (the largest trans_probability of the refined candidates), also the object's getFinalTransformation()
  // [pose-search-snippet end: relocalise]
  return result.converged ? LSR_OK : LSR_ERR_INVALID_ARGUMENT;
}

// the C++ surface: the same through the registration object
static bool relocalise(Ndt & ndt, const lidarslam_reg::Matrix4f & center, lidarslam_reg::Matrix4f * pose)
{
  lsr_pose_search_params prm = {};
  prm.lattice.n[0] = prm.lattice.n[1] = 9; prm.lattice.n[2] = 1;
  prm.lattice.step[0] = prm.lattice.step[1] = prm.lattice.step[2] = 1.0;
  prm.lattice.n_yaw = 13;
  prm.lattice.yaw_step = 5.0 * M_PI / 180.0;
  prm.top_k = 16; prm.min_sep_m = 0.9; prm.min_sep_rad = 7.5 * M_PI / 180.0;
  std::vector<double> score(4), pairs(4);
  std::vector<float> four(64, 0.f);
  if (!ndt.scorePoses(four.data(), 4, score.data(), pairs.data())) {return false;}
  if (!ndt.searchPose(center, prm)) {return false;}
  *pose = ndt.getFinalTransformation();
  return true;
}

int main() {
  // host only: the lattice, the selection, and the refusals that need no device
  const lidarslam_reg::Matrix4f I = lidarslam_reg::Matrix4f::Identity();
  lsr_pose_lattice L = {{3, 3, 1}, {1.0, 1.0, 1.0}, 4, 0.5};
  size_t count = 0;
  int ok = 0, refused = 0;
  ok += (lsr_pose_lattice_poses(I.data(), &L, nullptr, 0, &count) == LSR_OK && count == 36) ? 1 : 0;
  std::vector<float> poses(16 * count);
  ok += (lsr_pose_lattice_poses(I.data(), &L, poses.data(), count, &count) == LSR_OK && poses[12] == -1.0f && poses[13] == -1.0f) ? 1 : 0;
  std::vector<double> score(count, 1.0);
  score[7] = 3.0; score[8] = 2.5; score[30] = 2.0;       // 7 and 8 are 1 m apart at one heading; 30 is another heading
  int32_t kept[LSR_POSE_SEARCH_MAX_KEPT];
  int n_kept = 0;
  ok += (lsr_select_poses(score.data(), poses.data(), count, 2, 1.5, 0.3, kept, &n_kept) == LSR_OK && n_kept == 2 && kept[0] == 7 && kept[1] == 30) ? 1 : 0;
  refused += lsr_select_poses(score.data(), poses.data(), count, 17, 1.5, 0.3, kept, &n_kept) == LSR_ERR_INVALID_ARGUMENT ? 1 : 0;
  L.n[1] = 0;
  refused += lsr_pose_lattice_poses(I.data(), &L, nullptr, 0, &count) == LSR_ERR_INVALID_ARGUMENT ? 1 : 0;
  float pose16[16] = {0};
  refused += relocalise(nullptr, I.data(), pose16) == LSR_ERR_INVALID_ARGUMENT ? 1 : 0;    // no handle
  bool (*cpp_surface)(Ndt &, const lidarslam_reg::Matrix4f &, lidarslam_reg::Matrix4f *) = &relocalise;   // instantiated, not run: it needs a device
  std::printf("POSE_SEARCH_SNIPPETS ok=%d refused=%d surface=%d\n", ok, refused, cpp_surface != nullptr ? 1 : 0);
  return (ok != 3 || refused != 3) ? 1 : 0;
}

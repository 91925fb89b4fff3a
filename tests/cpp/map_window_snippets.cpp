// TEST INFRASTRUCTURE: the localiser's callback of INTEGRATION.md §3j — compiled against include/lidarslam_reg/map_window.hpp and
// registration.hpp and linked against the library by tests/test_map_window_cpu.py, which also checks that the block between the
// markers below is, verbatim, the block INTEGRATION.md shows.
#include <lidarslam_reg/map_window.hpp>
#include <lidarslam_reg/registration.hpp>

#include <cstdint>
#include <memory>
#include <vector>

namespace mock {
struct PointXYZI { float x, y, z, pad, intensity, pad2[3]; };
struct Cloud { std::vector<PointXYZI> points; };
}  // namespace mock
using Ndt = lidarslam_reg::NormalDistributionsTransform<mock::PointXYZI, mock::PointXYZI, mock::Cloud, mock::Cloud>;

struct Localizer {
  std::unique_ptr<Ndt> registration_;
  lidarslam_reg::MapWindowTracker tracker_;
  const void * map_records_ = nullptr;   // the saved map, resident in HBM: pcl::PointXYZI records (lidarslam_reg::loadPCDFile...)
  size_t map_points_ = 0;
  lidarslam_reg::Matrix4f pose_ = lidarslam_reg::Matrix4f::Identity();
  bool receiveCloud(const void * payload, size_t n_points);
};

bool Localizer::receiveCloud(const void * payload, size_t n_points)
{
  const lsr_pc2_layout layout = {32u, 0u, 4u, 8u, 16};
  mock::Cloud output;
  // [map-window-snippet begin: receive_cloud]
  // the target is the window of the saved map around the pose, cut out of the resident map on the device; it is cut again once
  // the pose has left the centre of the cut by more than slack / 2 (and at once, reported, when the pose is outside the window)
  const double t[3] = {pose_.m[12], pose_.m[13], pose_.m[14]};
  if (tracker_.needsCut(t)) {
    if (!tracker_.cutAround(t)) {return false;}
    if (!registration_->setInputTargetWindow(map_records_, map_points_, layout, tracker_.window)) {return false;}
  }
  if (!registration_->setInputSourcePointCloud2(payload, n_points, layout, 0.1, 100.0, 0.2f)) {return false;}
  registration_->align(output, pose_);
  pose_ = registration_->getFinalTransformation();
  // [map-window-snippet end: receive_cloud]
  return !tracker_.lost;
}

int main() {
  // host only: the window of a pose, the re-cut rule, and the refusals that need no device
  lidarslam_reg::MapWindowTracker tr;
  tr.reach[0] = tr.reach[1] = 50.0; tr.reach[2] = 10.0;
  tr.slack[0] = tr.slack[1] = 6.0; tr.slack[2] = 4.0;
  tr.leaf = 1.0f;
  double t[3] = {10.5, -3.25, 0.0};
  int ok = 0;
  ok += tr.needsCut(t) && tr.cutAround(t) ? 1 : 0;                       // no window yet
  ok += (tr.window.lo[0] == -46 && tr.window.hi[0] == 66 && tr.window.lo[2] == -14 && tr.window.hi[2] == 14) ? 1 : 0;
  t[0] += 2.9;
  ok += !tr.needsCut(t) ? 1 : 0;                                         // within slack / 2
  t[0] += 0.2;
  ok += (tr.needsCut(t) && !tr.lost && tr.cutAround(t) && tr.n_recuts == 1) ? 1 : 0;
  t[1] += 500.0;
  ok += (tr.needsCut(t) && tr.lost) ? 1 : 0;                             // outside the window: lost, and said so
  lsr_map_window w;
  const double far[3] = {3.0e6, 0, 0}, half[3] = {1, 1, 1};
  int refused = 0;
  refused += lidarslam_reg::mapWindowAround(far, half, 0.1f, &w) ? 0 : 1;     // a cell beyond 2^24
  refused += lidarslam_reg::mapWindowAround(t, half, 0.0f, &w) ? 0 : 1;
  std::vector<uint8_t> payload(3, 1);
  const float one[8] = {1.0f, 1.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  refused += lidarslam_reg::cropMap(nullptr, one, 1, tr.window, payload) ? 0 : 1;   // no handle
  size_t n = 0;
  refused += lidarslam_reg::cropMapDevice(nullptr, one, 1, tr.window, nullptr, 0, &n) ? 0 : 1;
  std::printf("MAP_WINDOW_SNIPPETS ok=%d refused=%d payload=%d\n", ok, refused, (int)payload.size());
  return (ok != 5 || refused != 4 || !payload.empty()) ? 1 : 0;
}

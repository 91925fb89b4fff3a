// TEST INFRASTRUCTURE: searchLoop by appearance of INTEGRATION.md §3l — compiled against include/lidarslam_reg/scan_context.hpp and
// linked against the library; main() runs what needs no device: the tables, the guess and the refusals.
#include <lidarslam_reg/scan_context.hpp>

#include <cmath>
#include <cstdio>

namespace {
struct Backend {
  lsr_handle registration = nullptr;
  std::vector<lsr_submap> submaps;              // the MapArray so far, pose-local pcl::PointXYZI records
  lidarslam_reg::ScanContextTable contexts;     // one descriptor per submap, extended as submaps arrive
  lsr_loop_params loop{1.0, 20.0, 20.0, 3, 0.2f, 1, 0};
  std::vector<lsr_loop_edge> loop_edges;

  // [scan-context-snippet begin: search_loop]
  bool searchLoop() {
    if (!contexts.update(registration, submaps)) return false;            // the new keyframes' descriptors, one launch
    const lsr_appearance_loop_params params = lidarslam_reg::appearanceLoopDefaults(loop);
    std::vector<lsr_loop_edge> edges;
    if (!lidarslam_reg::searchLoopAppearance(registration, submaps, 32, contexts, params, edges)) return false;
    for (const lsr_loop_edge& e : edges)
      if (e.accepted) loop_edges.push_back(e);                            // pair_id and relative_pose as searchLoop fills them
    return true;
  }
  // [scan-context-snippet end: search_loop]
};
}  // namespace

int main() {
  int ok = 0, refused = 0;
  const lsr_scan_context_params p = lidarslam_reg::scanContextDefaults();
  float edge2[LSR_SCAN_CONTEXT_MAX_RINGS], b[LSR_SCAN_CONTEXT_MAX_SECTORS];
  if (lsr_scan_context_tables(&p, edge2, b) == LSR_OK && edge2[0] == 16.0f && edge2[19] == 6400.0f && std::fabs(b[29] - 1.0f) < 1e-6f) ok++;
  lsr_scan_context_params bad = p;
  bad.num_sectors = 61;
  if (lsr_scan_context_tables(&bad, edge2, b) == LSR_ERR_INVALID_ARGUMENT) refused++;
  lsr_submap a{}, c{};
  a.orientation[3] = c.orientation[3] = 1.0;
  a.position[0] = 3.0;
  float g[16];
  if (lsr_scan_context_guess(&a, &c, 15, 60, g) == LSR_OK && std::fabs(g[1] - 1.0f) < 1e-6f && std::fabs(g[12] - 3.0f) < 1e-6f) ok++;
  if (lsr_scan_context_guess(&a, &c, 60, 60, g) == LSR_ERR_INVALID_ARGUMENT) refused++;
  Backend backend;                                  // no object: the gate refuses, the table stays empty
  backend.submaps.push_back(a);
  if (!backend.searchLoop() && backend.contexts.count == 0 && backend.loop_edges.empty()) refused++;
  std::printf("SCAN_CONTEXT_SNIPPETS ok=%d refused=%d\n", ok, refused);
  return (ok == 2 && refused == 3) ? 0 : 1;
}

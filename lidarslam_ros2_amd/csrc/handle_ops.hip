// Mechanics of the registration object that every host unit behind the C ABI uses (api_internal.hpp): the deferred stream
// dependencies of a candidate set's members and the life of a target object.  Host-side orchestration only.
#include "api_internal.hpp"

namespace lsr {

// the object is about to be used on its own: its stream now waits for the group work it was part of (lsr::StreamDep, handle.hpp)
int settle_dep(lsr_handle h) {
  if (!h->dep) return LSR_OK;
  if (h->dep_stream != h->stream && hipStreamWaitEvent(h->stream, h->dep->ev, 0) != hipSuccess) {
    set_last_error("hipStreamWaitEvent failed (deferred dependency on a group launch)");
    return LSR_ERR_HIP;
  }
  h->dep.reset();
  h->dep_stream = nullptr;
  return LSR_OK;
}
// after group work for `members` has been enqueued on the lead's stream: one event record, the members remember it
int defer_members_behind(lsr_handle lead, lsr_handle* members, int count) {
  if (!lead->lead_dep) {
    auto d = std::make_shared<lsr::StreamDep>();
    if (hipEventCreateWithFlags(&d->ev, hipEventDisableTiming) != hipSuccess) { set_last_error("hipEventCreate failed"); return LSR_ERR_HIP; }
    lead->lead_dep = d;
  }
  bool any = false;
  for (int b = 0; b < count; b++) any = any || (members[b] != lead && members[b]->stream != lead->stream);
  if (!any) return LSR_OK;
  if (hipEventRecord(lead->lead_dep->ev, lead->stream) != hipSuccess) { set_last_error("hipEventRecord failed"); return LSR_ERR_HIP; }
  for (int b = 0; b < count; b++)
    if (members[b] != lead && members[b]->stream != lead->stream) { members[b]->dep = lead->lead_dep; members[b]->dep_stream = lead->stream; }
  return LSR_OK;
}

// Make everything `h` still has in flight on its own stream precede what is enqueued on `lead` next (group launches of a
// candidate set run on the first member's stream).  An idle stream — the usual case — costs one query and no event.
int order_lead_after(hipStream_t lead, lsr_handle h) {
  if (h->dep) {
    // everything this member has had enqueued since its last own use went to dep_stream (a group call ordered that stream behind the
    // member's own one before it started): on the same lead stream there is nothing to order, on another one the event is the order —
    // also when the member is the lead of THIS call (its own stream is `lead`: the dependency is then settled for good)
    if (h->dep_stream != lead) LSR_HIP(hipStreamWaitEvent(lead, h->dep->ev, 0));
    if (h->stream == lead) { h->dep.reset(); h->dep_stream = nullptr; }
    return LSR_OK;
  }
  if (h->stream == lead) return LSR_OK;
  if (hipStreamQuery(h->stream) == hipSuccess) return LSR_OK;
  LSR_HIP(hipEventRecord(h->ev1, h->stream));
  LSR_HIP(hipStreamWaitEvent(lead, h->ev1, 0));
  return LSR_OK;
}

// A fresh target object — or the handle's current one recycled when nobody else holds it (lsr_share_target): its device
// buffers only ever grow, so the frontend's "new target every few scans" costs no hipMalloc / hipFree (those were 250 us
// of a 350 us setInputTarget).
std::shared_ptr<TargetData> fresh_target(lsr_handle h) {
  std::shared_ptr<TargetData> t;
  auto only_mine = [&](const std::shared_ptr<TargetData>& c) {
    return c && c.use_count() == (long)((h->target == c) + (h->spare_target == c));
  };
  if (only_mine(h->target)) t = h->target;
  else if (only_mine(h->spare_target)) t = h->spare_target;
  else t = std::make_shared<TargetData>();
  h->spare_target = t;  // survives a failed setInputTarget (which resets h->target)
  t->n = 0;
  t->has_grid = t->has_hash = t->has_cov = t->has_centroids = false;
  t->grid_leaf = 0.f;
  return t;
}

bool target_is_shared(lsr_handle h) {
  return h->target && h->target.use_count() > (long)(1 + (h->spare_target == h->target));
}

int ensure_ndt_grid(lsr_handle h) {
  TargetData& t = *h->target;
  std::lock_guard<std::mutex> lock(t.build_mutex);
  float leaf = (float)h->ndt.resolution;
  // the KDTREE neighbourhood reads the leaves' float centroids: built on first use, for the grid in place
  auto centroids = [&]() -> int {
    if (h->ndt.neighborhood != LSR_KDTREE || t.has_centroids || t.grid.ncells == 0) return LSR_OK;
    const int cst = ndt_build_centroids(t.cloud, t.grid, h->scratch, h->stream);
    if (!cst) t.has_centroids = true;
    return cst;
  };
  if (t.has_grid && t.grid_leaf == leaf) return centroids();
  if (t.has_grid && target_is_shared(h)) {
    // rebuilding in place would pull the grid from under the other handles (their d1/d2 and leaf size belong to the old one)
    set_last_error("the shared target's voxel grid was built at another resolution: sharers must use one ndt_resolution");
    return LSR_ERR_INVALID_ARGUMENT;
  }
  t.has_centroids = false;
  int st = ndt_build_grid(t.cloud, leaf, t.grid, h->scratch, h->stream);
  if (st) return st;
  t.has_grid = true;
  t.grid_leaf = leaf;
  return centroids();
}

// An NDT target whose voxel grid was built by the counting-sort builder keeps its points in voxel order: the neighbour grid is
// a refinement of that order (one launch, nn_build_hash_from_grids) instead of a second sort of the cloud.
bool hash_from_grid_possible(lsr_handle h) {
  const TargetData& t = *h->target;
  return h->method == LSR_METHOD_NDT && t.has_grid && t.grid.has_sorted && t.grid.ncells > 0 && t.grid.sorted_n == t.cloud.n;
}

int ensure_target_hash(lsr_handle h) {
  TargetData& t = *h->target;
  std::lock_guard<std::mutex> lock(t.build_mutex);
  if (t.has_hash) return LSR_OK;
  int st;
  if (hash_from_grid_possible(h)) {
    const VoxelGridDev* vg[1] = {&t.grid};
    HashGridDev* hg[1] = {&t.hash};
    st = nn_build_hash_from_grids(vg, hg, 1, h->stream);
  } else {
    st = nn_build_hash(t.cloud, nn_pick_cell(t.cloud.n, h), t.hash, h->scratch, h->stream);
  }
  if (st) return st;
  t.has_hash = true;
  return LSR_OK;
}

}  // namespace lsr

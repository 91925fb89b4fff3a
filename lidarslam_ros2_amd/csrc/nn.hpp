// Kd-tree-free exact nearest-neighbour search on a two-level hashed voxel grid
// (replaces pcl::KdTreeFLANN behind getFitnessScore and GICP).
#pragma once
#include "common.hpp"

struct lsr_handle_s;

namespace lsr {
// N2: transform one keyframe (strided xyz, device) by a column-major 4x4 and write it at `offset` of `out`.
int transform_append(const void* d_aos, size_t stride_bytes, size_t n, const float* d_T16, DeviceCloud& out, size_t offset,
                     hipStream_t stream);
// The same for a whole window in one launch (lsr_set_input_target_frames_filtered): one table entry per frame, device resident.
// The launch also leaves the bounding-box records of the assembled cloud where pc2_ingest leaves a scan's (sc.bbox_dev, the host
// mailbox; out.bbox_enqueued), so the voxel_grid_filter behind it needs no bounding-box pass and can take its device-side form.
struct FrameSlot {
  const unsigned char* records;   // strided xyz records (device)
  int count;                      // points of the frame
  int first_out;                  // index of its first point in the assembled cloud
  int first_slice;                // index of its first slice (frames_slice_count)
  int pad;
  float T16[16];                  // column-major pose
};
int frames_slice_count(const size_t* counts, int n_frames, int* first_slice);
int assemble_frames_bbox(const FrameSlot* d_frames, int n_frames, int n_slices, size_t stride_bytes, size_t total, DeviceCloud& out,
                         BuildScratch& sc, hipStream_t stream);
// N5: the whole map from its submaps in one launch, records in, records out (lsr_assemble_map).  One table entry per submap (or
// per piece of one), device resident; the output index is 64-bit, so the table has a slot type of its own.
struct MapSlot {
  const unsigned char* records;   // the submap's records in the input layout (device)
  long long first_out;            // index of its first record in the output buffer
  int count;                      // records of the slot (> 0: empty submaps get no slot)
  int first_slice;                // index of its first slice of MAP_SLICE records
  float T16[16];                  // column-major pose
};
struct MapLayouts {               // byte offsets; intensity < 0: the input has none / the output gets none
  unsigned int in_step, in_x, in_y, in_z;
  int in_intensity;
  unsigned int out_step, out_x, out_y, out_z;
  int out_intensity;
};
constexpr int MAP_SLICE = 1024;
// wide: both layouts are pcl::PointXYZI's {32; 0,4,8,16} and every base pointer is 16-byte aligned (two 16-byte loads and two 16-byte
// stores per record); otherwise the general form, any 4-byte-aligned layout.  Both write every byte of an output record.
int assemble_map(const MapSlot* d_slots, int n_slots, int n_slices, bool wide, const MapLayouts& L, void* d_out, hipStream_t stream);
float nn_pick_cell(size_t n, const lsr_handle_s* h);
int nn_build_hash(const DeviceCloud& cloud, float cell, HashGridDev& grid, BuildScratch& sc, hipStream_t stream);
// the same structure for NDT targets whose voxel grid was built by the counting-sort builder: a refinement of the voxel order
// (fine cell = leaf / 8), one launch for up to LSR_GROUP targets, no host round trip
int nn_build_hash_from_grids(const VoxelGridDev* const* vgrids, HashGridDev* const* grids, int count, hipStream_t stream);
// mean squared 1-NN distance of T*source in the target, over pairs with d2 <= max_range.
int nn_fitness_score(const DeviceCloud& source, const float* T16_host, const HashGridDev& grid, double max_range, double* out,
                     BuildScratch& sc, DevBuf<float>& d_T16, hipStream_t stream);
int nn_fitness_begin(const DeviceCloud& source, const float* T16_host, const HashGridDev& grid, double max_range, BuildScratch& sc,
                     DevBuf<float>& d_T16, hipStream_t stream);
int nn_fitness_end(BuildScratch& sc, hipStream_t stream, double* out);
// the search + reduction of a set of candidates in group launches on one stream (each member: its own scratch and mailbox)
struct FitJob { const DeviceCloud* source; const float* T16; const HashGridDev* grid; double max_range; BuildScratch* sc; };
int nn_fitness_begin_group(const FitJob* jobs, int count, hipStream_t stream);
// Device-side entry point (results stay in HBM): 1-NN of T*q (T nullable).
int nn_search_device(const DeviceCloud& q, const float* d_T16, const HashGridDev& grid, int fine_rings, float max_d2,
                     int* d_idx, float* d_d2, hipStream_t stream, int* d_work = nullptr);  // d_work: n + 1 ints => two-stage search
int nn_search_host(const DeviceCloud& source, const float* T16_host, const HashGridDev& grid, int32_t* idx, float* d2,
                   BuildScratch& sc, DevBuf<float>& d_T16, hipStream_t stream);
}  // namespace lsr

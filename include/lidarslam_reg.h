/*
 * lidarslam_reg.h — C ABI of the MI355X-native scan-matching registration core.
 *
 * This is the drop-in boundary for the ONE hot path of rsasaki0109/lidarslam_ros2: the
 * pcl::Registration<pcl::PointXYZI,pcl::PointXYZI> object that ScanMatcherComponent
 * (scanmatcher/include/scanmatcher/scanmatcher_component.h:93) and GraphBasedSlamComponent
 * (graph_based_slam/include/graph_based_slam/graph_based_slam_component.h:106) hold and call.
 * Every entry point below names the reference call it replaces (file:line under
 * /root/reference).  The arithmetic the reference reaches through those calls lives in the
 * un-vendored submodule Thirdparty/ndt_omp_ros2 (.gitmodules:1-4) + PCL; SURVEY.md §9 is its
 * restatement.
 *
 * Conventions
 *  - plain C, no exceptions cross this boundary; every function returns an lsr_status
 *    (0 = ok, < 0 = error) and leaves outputs untouched on error;
 *  - clouds are "strided xyz": 3 consecutive fp32 at byte offset 0 of every `stride_bytes`
 *    record (pcl::PointXYZI: stride 32; packed xyz: stride 12; xyzw: stride 16);
 *  - 4x4 transforms are COLUMN-MAJOR fp32 (Eigen::Matrix4f memory order);
 *  - a handle is thread-compatible (one caller at a time), distinct handles are re-entrant —
 *    the reference's threading contract (lidarslam/src/lidarslam.cpp:12-17);
 *  - there is NO CPU fallback: without a usable gfx950 device lsr_create fails.
 */
#ifndef LIDARSLAM_REG_H
#define LIDARSLAM_REG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lsr_handle_s* lsr_handle;

typedef enum lsr_status {
  LSR_OK = 0,
  LSR_ERR_INVALID_ARGUMENT = -1,
  LSR_ERR_NO_DEVICE = -2,       /* no gfx950 device / HIP runtime unusable */
  LSR_ERR_HIP = -3,             /* a HIP call failed; see lsr_last_error() */
  LSR_ERR_NO_TARGET = -4,       /* align/getFitnessScore before setInputTarget */
  LSR_ERR_NO_SOURCE = -5,       /* align/getFitnessScore before setInputSource */
  LSR_ERR_NOT_IMPLEMENTED = -6, /* a .pcd file the readers do not take: DATA binary_compressed (without LSR_PCD_READ_COMPRESSED), coordinates that are not 4-byte floats
                                   (lsr_parse_pcd_header, lsr_decode_pcd, lsr_load_pcd; until round 6 the NDT neighbourhood KDTREE too) */
  LSR_ERR_INDEX_OVERFLOW = -7,  /* voxel index space exceeds int32 (PCL: "Leaf size is too small") */
  LSR_ERR_TOO_FEW_POINTS = -8,  /* GICP: cloud smaller than k_correspondences */
  LSR_ERR_IO = -9               /* a file could not be opened or written (lsr_save_pcd_ascii), opened or read (lsr_load_pcd,
                                   lsr_set_input_target_pcd); errno's text in lsr_last_error() */
} lsr_status;

/* registration_method: scanmatcher_component.cpp:103-124, graph_based_slam_component.cpp:63-86 */
typedef enum lsr_method { LSR_METHOD_NDT = 0, LSR_METHOD_GICP = 1 } lsr_method;

/* pclomp::NeighborSearchMethod, selected at scanmatcher_component.cpp:110 (the reference only ever selects DIRECT7).
 * KDTREE (round 6): ndt_omp's radiusSearch(x', resolution) over the kd-tree of the leaves' float centroids, restated as the 27 cells
 * around the point's cell filtered by the kd-tree's own test (FLANN L2_Simple<float> strictly below (float)(resolution^2)) — a
 * centroid lies inside its own cell, so no leaf outside those cells can pass.  The kd-tree holds every leaf with >= 6 points, those
 * the eigen check invalidated (npts = -1) included: pclomp pushes the centroid before that check and neither radiusSearch() nor
 * computeDerivatives() tests nr_points, so such a leaf is a neighbour with its constructor icov of 0 — it adds -d1 to the score and
 * nothing to the gradient or Hessian (the DIRECT lookups skip it).  The centroids are built on first use. */
typedef enum lsr_neighborhood { LSR_KDTREE = 0, LSR_DIRECT26 = 1, LSR_DIRECT7 = 2, LSR_DIRECT1 = 3 } lsr_neighborhood;

typedef enum lsr_key {
  /* double-valued (lsr_set_f64 / lsr_get_f64) */
  LSR_RESOLUTION = 0,                 /* ndt->setResolution                 scanmatcher_component.cpp:107 */
  LSR_TRANSFORMATION_EPSILON = 1,     /* setTransformationEpsilon           scanmatcher_component.cpp:108,119 */
  LSR_STEP_SIZE = 2,                  /* NDT step_size_ (ctor default 0.1; never set by the reference) */
  LSR_OUTLIER_RATIO = 3,              /* NDT outlier_ratio_ (0.55) */
  LSR_MAX_CORRESPONDENCE_DISTANCE = 4,/* setMaxCorrespondenceDistance      scanmatcher_component.cpp:118 */
  LSR_ROTATION_EPSILON = 5,           /* GICP rotation_epsilon_ (2e-3) */
  LSR_EUCLIDEAN_FITNESS_EPSILON = 6,  /* setEuclideanFitnessEpsilon         graph_based_slam_component.cpp:80 (no effect) */
  LSR_GICP_EPSILON = 7,               /* GICP gicp_epsilon_ (1e-3) */
  LSR_MAP_ASSEMBLY_MS = 8,            /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the launches of the last
                                         lsr_assemble_map on this object (the kernel alone: staging copies are outside the bracket); else 0 */
  LSR_POSE_GRAPH_BAND_SOLVE_MS = 9,   /* read-only (lsr_get_f64), the next two likewise: with LSR_PROFILE = 1, three stages of the last
                                         lsr_optimize_pose_graph / _long on this object, each between hipEvents and summed over its trials
                                         [ms]: the right-hand sides and the 1 + 6L band solves; */
  LSR_POSE_GRAPH_DENSE_MS = 10,       /* the dense part (C = I + U B^-1 U^T formed, factored and solved); */
  LSR_POSE_GRAPH_COMBINE_MS = 11,     /* the row combine x = B^-1 b - B^-1 U^T z.  Else 0 */
  LSR_PCD_FORMAT_MS = 12,             /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the formatting launches
                                         (length pass, scan, write pass; copies outside the brackets) of the last lsr_format_pcd_ascii /
                                         lsr_save_pcd_ascii / lsr_save_map_pcd_ascii on this object, summed over its pieces; else 0 */
  LSR_PCD_PARSE_MS = 13,              /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the four launches (line
                                         pass, scan, index pass, parse pass; copies outside the brackets) of the last lsr_decode_pcd /
                                         lsr_load_pcd / lsr_set_input_target_pcd of an ASCII file on this object, summed over its
                                         pieces; else 0 */
  LSR_PCD_INFLATE_MS = 14,            /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the inflate launches (block
                                         maps, scan, source words, doubling passes, record gather; copies outside the brackets) of the
                                         last lsr_decode_pcd / lsr_load_pcd / lsr_set_input_target_pcd of a DATA binary_compressed file
                                         on this object; else 0 (0 after a file of another kind) */
  LSR_PCD_DEFLATE_MS = 15,            /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the deflate launches
                                         (field-major gather, chunk compressor, scan, and the compaction where the stream is written;
                                         copies outside the brackets) of the last lsr_format_pcd / lsr_save_pcd / lsr_save_map_pcd with
                                         LSR_PCD_BINARY_COMPRESSED on this object; else 0 (0 after a call of these with another kind) */
  LSR_MAP_FILTER_BBOX_MS = 16,        /* read-only (lsr_get_f64), the next five likewise: with LSR_PROFILE = 1, the hipEvent time [ms] of
                                         the launches of the last lsr_voxel_grid_filter_map / lsr_assemble_map_filtered /
                                         lsr_save_map_pcd_filtered on this object (copies outside the brackets): the bounding-box pass; */
  LSR_MAP_FILTER_KEY_MS = 17,         /* the key pass; */
  LSR_MAP_FILTER_SORT_MS = 18,        /* the sort (both words and the two gathers of a wide index); */
  LSR_MAP_FILTER_RUNS_MS = 19,        /* the run finder and its scan; */
  LSR_MAP_FILTER_CENTROID_MS = 20,    /* the centroids; */
  LSR_MAP_FILTER_WRITE_MS = 21,       /* the write of the output records.  Else 0 (the last two also after a call that only counted) */
  LSR_MAP_WINDOW_MS = 22,             /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the three launches (count,
                                         scan, write; copies outside the brackets) of the last lsr_crop_map /
                                         lsr_set_input_target_window on this object; else 0 (the write is absent after a call that only
                                         counted or kept nothing) */
  LSR_POSE_SEARCH_MS = 23,            /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the scoring launch (the
                                         pose upload and the copy of the scores outside the brackets) of the last lsr_ndt_score_poses /
                                         lsr_ndt_search_pose on this object; else 0 */
  LSR_SCAN_CONTEXT_BUILD_MS = 24,     /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the descriptor launches
                                         (staging copies outside the brackets) of the last lsr_scan_context_build on this object; */
  LSR_SCAN_CONTEXT_MATCH_MS = 25,     /* of the comparison launch of the last lsr_scan_context_match / lsr_search_loop_appearance.  Else 0 */
  LSR_DEPTH_IMAGES_MS = 26,           /* read-only (lsr_get_f64): with LSR_PROFILE = 1, the hipEvent time [ms] of the image launches (build
                                         and erosion; the fill and the staging copies outside the brackets) of the last
                                         lsr_depth_images_build on this object; */
  LSR_VISIBILITY_MS = 27,             /* of the votes launch of the last lsr_visibility_votes, or of the votes and the three launches of
                                         the compaction (count, scan, write) of the last lsr_assemble_map_static.  Else 0 */
  /* int-valued (lsr_set_i32 / lsr_get_i32) */
  LSR_MAX_ITERATIONS = 32,           /* setMaximumIterations               graph_based_slam_component.cpp:66,77 */
  LSR_NEIGHBORHOOD = 33,              /* setNeighborhoodSearchMethod        scanmatcher_component.cpp:110 */
  LSR_NUM_THREADS = 34,               /* setNumThreads (accepted, ignored)  scanmatcher_component.cpp:111 */
  LSR_K_CORRESPONDENCES = 35,         /* GICP k_correspondences_ (20) */
  LSR_MAX_INNER_ITERATIONS = 36,      /* GICP max_inner_iterations_ (20) */
  LSR_RANSAC_ITERATIONS = 37,         /* setRANSACIterations (accepted, ignored) graph_based_slam_component.cpp:81 */
  LSR_HESSIAN_D1_SIGN = 38,           /* +1 = upstream "+sy" quirk in h_ang d1 (default), -1 = analytic */
  LSR_PROFILE = 39,                   /* 1 = bracket the derivative launch chains with hipEvents (lsr_get_profile) */
  /* tuning (NO effect on results: every NDT derivative kernel returns the same bits — the sum of a pass is defined on the
     input, csrc/ndt.hip: canon): */
  LSR_NDT_WORKGROUP = 40,             /* lane kernel: threads per workgroup (512, 1024); quad kernel: source points per
                                         workgroup (64, 128; four lanes each); 0 = automatic (512 / 128).  256 (the default of
                                         the rounds 1-3 kernel) is accepted and means automatic; as an environment preset an
                                         unknown value is reported on stderr and ignored */
  LSR_NDT_TABLE_MODE = 41,            /* where the pass reads leaf records: -1 = automatic, 0 = dense global table,
                                         1 = compact global table, 2 = whole table staged in LDS (when it fits) */
  LSR_GRID_BUILDER = 42,              /* 0 = automatic (counting sort for <= 16383 grid cells, radix sort beyond), 1 = always
                                         the radix-sort builder */
  LSR_WAIT_MODE = 43,                 /* how the calling thread waits for the device inside align() / setInputTarget():
                                         0 = spin (lowest latency, pins one core per running call), 1 = sched_yield between
                                         polls, 2 = sleep 20 us between polls (a ROS2 MultiThreadedExecutor runs two
                                         registration objects side by side, lidarslam/src/lidarslam.cpp:12-17).
                                         Environment preset: LSR_WAIT_MODE=spin|yield|sleep (or 0|1|2) */
  LSR_NDT_QUAD = 44,                  /* single NDT registrations: 1 = quad kernel (four lanes per source point on every CU:
                                         lowest latency for a 30k-point scan), 0 = lane kernel (one lane per point: what candidate
                                         sets use), -1 = automatic (quad below 65 536 source points, lane from there on) */
  /* 45 is unassigned (formerly LSR_NDT_SORT): the other keys keep their numbers */
  LSR_VOXEL_FILTER_FORM = 46,         /* read-only (lsr_get_i32): which form the last VoxelGrid filter on this object took:
                                         0 = none yet, 1 = grid dimensions worked out on the host (one wait for the bounding box,
                                         one for the leaf count), 2 = on the device (one wait: from the second
                                         lsr_set_input_source_pc2 / _frontend of an object on), 3 = the device form came back
                                         flagged (more key bits than planned, or an index overflow) and the host form ran */
  LSR_NDT_SPLIT = 47,                 /* single NDT registrations on the 512-thread lane kernel: 1 = two waves per 64-point chunk (each
                                         forms one half of the per-point neighbour tree; half the serial chain per wave, twice the waves),
                                         0 = one wave per chunk, -1 = automatic (= 0: measured on BASELINE cfg 5, the split form is not
                                         faster — the pass is bound by its fixed latency chain).  Environment preset LSR_NDT_SPLIT */
  LSR_TARGET_PREPARED = 48,           /* read-only (lsr_get_i32): 1 = an align with this object's parameters finds nothing left to build on
                                         the current target (GICP: neighbour grid and k-NN covariances computed with this object's
                                         k_correspondences / gicp_epsilon; NDT: voxel grid at this object's resolution), 0 = the next
                                         align builds something first, or there is no target */
  LSR_MAP_ASSEMBLY_FORM = 49,         /* read-only (lsr_get_i32): which form the last lsr_assemble_map on this object took: 0 = none yet,
                                         1 = wide (both layouts {32; 0,4,8,16}, every base pointer 16-byte aligned: two 16-byte loads
                                         and two 16-byte stores per record), 2 = general (any layout).  The bytes are the same */
  LSR_PCD_PIECE_RECORDS = 50,         /* records per piece of lsr_save_pcd_ascii / lsr_save_map_pcd_ascii (64 .. 1 << 22, default 1 << 20): a
                                         piece is formatted and copied while the calling thread writes the one before it.  The file's
                                         bytes do not depend on it.  lsr_save_pcd / lsr_save_map_pcd: the same for a binary body; a
                                         compressed stream is copied and written in pieces of as many bytes as that many packed records */
  LSR_PCD_READ_PIECE_BYTES = 52,      /* bytes per piece of lsr_load_pcd / lsr_set_input_target_pcd (2048 .. 1 << 28, default 1 << 26): a piece
                                         is read from the file while the one before it is parsed.  The records do not depend on it */
  LSR_PCD_UNRESOLVED_TOKENS = 53,     /* read-only (lsr_get_i32): how many values of the last lsr_decode_pcd / lsr_load_pcd /
                                         lsr_set_input_target_pcd on this object the device left to the C library's strtof (0 for every
                                         text whose values have at most 19 significant digits) */
  LSR_PCD_READ_COMPRESSED = 54,       /* 1 = lsr_decode_pcd / lsr_load_pcd / lsr_set_input_target_pcd on this object read DATA
                                         binary_compressed files, the LZF stream inflated on the device; 0 (default) = they refuse such a
                                         file with LSR_ERR_NOT_IMPLEMENTED.  Any other value is LSR_ERR_INVALID_ARGUMENT.  Per object, no
                                         environment preset */
  LSR_MAP_FILTER_KEY_BITS = 55,       /* read-only (lsr_get_i32): the bits of the largest leaf index of the last lsr_voxel_grid_filter_map /
                                         lsr_assemble_map_filtered / lsr_save_map_pcd_filtered on this object (0 before the first, and
                                         after a cloud without a finite point); above 32 the index was sorted as two words */
  LSR_VISIBILITY_PIECE_BYTES = 56,    /* bytes per staging piece of HOST clouds in lsr_depth_images_build / lsr_visibility_votes /
                                         lsr_assemble_map_static's votes (256 .. 1 << 30, default 1 << 26): the table of submaps is walked
                                         one launch per piece, a long submap cut.  The images and the votes do not depend on it */
  LSR_GICP_SOLVER = 51                /* GICP inner optimiser (lsr_gicp_solver): LSR_GICP_GAUSS_NEWTON (default) or LSR_GICP_BFGS, the
                                         reference's own schedule (PCL's port of GSL vector_bfgs2: Fletcher line search, memoryless
                                         direction update, |g| < 1e-2 / max_inner_iterations / no progress).  Per object, no environment
                                         preset; every entry that aligns a GICP object follows it (lsr_align, the batches, lsr_search_loop,
                                         the frontend paths), and a batch may mix objects with different solvers.  Any other value:
                                         LSR_ERR_INVALID_ARGUMENT */
} lsr_key;
typedef enum lsr_gicp_solver { LSR_GICP_GAUSS_NEWTON = 0 /* default */, LSR_GICP_BFGS = 1 } lsr_gicp_solver;
/* Environment presets read when an object is created: LSR_NDT_WORKGROUP, LSR_NDT_TABLE_MODE, LSR_NDT_QUAD, LSR_GRID_BUILDER,
 * LSR_WAIT_MODE (the keys above); LSR_NDT_CHAINS=1|2|3 fixes the number of independent launch chains a candidate set runs as (default: two
 * from six members on, each on a stream verified to run concurrently with the object's own; LSR_DEBUG_STREAMS=1 prints what the
 * verification found).  Diagnostic A/B switch read once per process, with bit-identical results: LSR_VG_DEVICE_DIMS=0 (the
 * VoxelGrid filter always works out its grid dimensions on the host). */

typedef struct lsr_result {
  int32_t converged;            /* hasConverged()                             scanmatcher_component.cpp:375 */
  int32_t iterations;           /* nr_iterations_ */
  double score;                 /* NDT: trans_probability_ (= score / N); GICP: final mean Mahalanobis cost (either solver) */
  int32_t n_evaluations;        /* NDT: derivative evaluations as the reference counts them (computeDerivatives calls + the
                                   computeHessian after a line search that took trial steps).  The tenth trial of a search
                                   and the computeHessian behind it are ONE launch here and count as two.
                                   GICP: Gauss-Newton inner steps; under LSR_GICP_BFGS the cost/gradient passes of the align (every
                                   pass yields f and g: fewer than the functor calls the reference's wrapper would count) */
  int32_t n_correspondences;    /* GICP: pairs in the last outer iteration; NDT: valid (point, voxel) pairs of the last derivative pass */
  double gpu_ms;                /* HOST wall-clock time of the align call that produced this result, from the first
                                   enqueue to the result in host memory; for lsr_align_batch every member carries the
                                   time of the whole batch.  (Device-side time per derivative pass: lsr_get_profile.) */
} lsr_result;

typedef struct lsr_profile {
  double deriv_ms_total;        /* hipEvent time of the derivative-launch chains since last reset (events bracket every
                                   chunk of launches as enqueued: launch-to-launch time, dependent-launch gap included) */
  int64_t deriv_launches;       /* launches of those chains that evaluated points: n_evaluations minus the line searches
                                   that ran to their tenth trial (for a batch: of the member with the most) */
  int64_t deriv_points;         /* source points processed by those launches */
  int64_t deriv_pairs;          /* valid (point,voxel) pairs of the LAST launch (K-bar * N) */
} lsr_profile;

const char* lsr_version(void);
const char* lsr_status_string(int status);
const char* lsr_last_error(void);                       /* thread-local, human readable */
int lsr_device_count(int* count);

/* new pclomp::NormalDistributionsTransform<..>() / new pclomp::GeneralizedIterativeClosestPoint<..>()
 * scanmatcher_component.cpp:105-106,116-117; graph_based_slam_component.cpp:64-65,74-75.
 * `stream` is a hipStream_t to run on (NULL = the handle creates its own). */
int lsr_create(int method, int device_id, void* stream, lsr_handle* out);
int lsr_destroy(lsr_handle h);

int lsr_set_f64(lsr_handle h, int key, double value);
int lsr_set_i32(lsr_handle h, int key, int value);
int lsr_get_f64(lsr_handle h, int key, double* value);
int lsr_get_i32(lsr_handle h, int key, int* value);

/* registration_->setInputTarget(cloud)   scanmatcher_component.cpp:275,307,315; graph_based_slam_component.cpp:227
 * NDT: builds the voxel-covariance grid on the device.  GICP: uploads and builds the neighbour-search grid; the 20-NN
 * covariances of the target are computed by the first align() that needs them, as the reference does.
 * Host-memory (`pts` readable by the CPU) and device-memory (`pts` a HIP device pointer) forms. */
int lsr_set_input_target(lsr_handle h, const void* pts, size_t stride_bytes, size_t n);
int lsr_set_input_target_device(lsr_handle h, const void* dev_pts, size_t stride_bytes, size_t n);
/* The same for a SET of candidates — one setInputTarget per candidate submap window, graph_based_slam_component.cpp:181-227
 * (BASELINE cfg 4).  handles[b] receives clouds[b] (counts[b] records of stride_bytes; all host or all device pointers).
 * Same result per object as `count` calls of lsr_set_input_target, but the builds overlap on the device: every stage of
 * every member is enqueued (on its own object's stream) before the host waits for the first — objects that were created on
 * one shared stream get the same results without the overlap.  All members on one device.  On error no member keeps a
 * target.  An object may appear only once. */
int lsr_set_input_target_batch(lsr_handle* handles, int count, const void* const* clouds, const size_t* counts,
                               size_t stride_bytes, int on_device);
/* Ordering and lifetime of DEVICE-resident inputs (every *_device entry point and every `on_device != 0` argument): the
 * core reads them with kernels on the handle's stream (lsr_create's `stream`, or the handle's own).  (1) If another
 * stream produced the buffer, call lsr_wait_stream(h, that_stream) first — it makes the handle's stream wait for
 * everything enqueued on the producer so far (event record + hipStreamWaitEvent, no host wait); buffers produced on the
 * handle's own stream or already complete need nothing.  (2) setInputTarget-type calls return after the read has
 * completed; lsr_set_input_source_device returns with the read ENQUEUED: keep the buffer alive and unmodified until the
 * next lsr_align / lsr_align_batch / lsr_get_fitness_score on this handle has returned (or synchronise its stream).
 * (3) lsr_set_input_source_filtered / _frontend / _pc2 return when the caller's buffer (host or device) has been read and the
 * number of points kept is known; the last kernel of the filter may still be running on the handle's stream, where every later
 * call on the handle is enqueued behind it (a lsr_align right after it starts under it).  LSR_SOURCE_SYNC=1 makes them wait. */
int lsr_wait_stream(lsr_handle h, void* producer_stream);
/* Submap assembly fused with setInputTarget: frame f (strided xyz, counts[f] points) is moved by poses16[16*f ..]
 * (column-major 4x4, pcl::transformPointCloud's fp32 arithmetic) and the frames are concatenated in order — what
 * updateMap() does on the host before setInputTarget (scanmatcher_component.cpp:449-464,307) and searchLoop() for a
 * loop candidate window (graph_based_slam_component.cpp:208-227).  on_device != 0: frame pointers are HIP device
 * pointers (keyframes kept resident in HBM); the assembled target never visits the host. */
int lsr_set_input_target_frames(lsr_handle h, int n_frames, const void* const* frames, const size_t* counts, size_t stride_bytes,
                                const float* poses16, int on_device);
/* The same followed by pcl::VoxelGrid(leaf) of the assembled cloud and setInputTarget of the FILTERED cloud, all in HBM: the
 * GICP branch of a map update (scanmatcher_component.cpp:308-316: `targeted_cloud_`, assembled newest keyframe first by
 * :448-464, goes through VoxelGrid(vg_size_for_input) before setInputTarget).  The filtered cloud is, bit for bit, what
 * lsr_voxel_grid_filter returns for the same assembled points (centroid per leaf, float sums in cloud order, output in
 * leaf-index order) — so the order of the frames matters for the bits.  Any method: a GICP object gets its neighbour grid,
 * an NDT object its voxel grid over the filtered cloud.  n_out (nullable) receives the number of target points.
 * leaf <= 0 is LSR_ERR_INVALID_ARGUMENT; on error the object keeps no target.  The window is assembled by one launch that also
 * leaves the bounding box of the assembled cloud on the device: from the object's second call on the filter works out its grid
 * dimensions there (LSR_VOXEL_FILTER_FORM 2, one host wait). */
int lsr_set_input_target_frames_filtered(lsr_handle h, int n_frames, const void* const* frames, const size_t* counts,
                                         size_t stride_bytes, const float* poses16, int on_device, float leaf, size_t* n_out);
/* Builds now, on the object's stream, everything the first lsr_align against the current target would still have to build, and
 * returns after it has completed; needs no input source.  GICP: the neighbour grid and the k-NN covariances of the target with
 * the object's current k_correspondences / gicp_epsilon (the reference computes them lazily inside align).  NDT: nothing is
 * left as a rule (setInputTarget builds the voxel grid).  LSR_ERR_NO_TARGET without a target, LSR_ERR_TOO_FEW_POINTS when the
 * target has fewer points than k_correspondences.  Called on the object that built a target before lsr_share_target hands it
 * over, the scan that takes the target over pays for no target-side build (LSR_TARGET_PREPARED reads 1 on the taker when its
 * k_correspondences / gicp_epsilon are the builder's). */
int lsr_prepare_target(lsr_handle h);
/* registration_->setInputSource(cloud)   scanmatcher_component.cpp:329; graph_based_slam_component.cpp:181 */
int lsr_set_input_source(lsr_handle h, const void* pts, size_t stride_bytes, size_t n);
int lsr_set_input_source_device(lsr_handle h, const void* dev_pts, size_t stride_bytes, size_t n);
/* The same for a SET of candidates (graph_based_slam_component.cpp:181 inside the candidate loop): handles[b] receives clouds[b];
 * all host or all device pointers; the uploads share launches.  Device inputs follow the lifetime rule of
 * lsr_set_input_source_device. */
int lsr_set_input_source_batch(lsr_handle* handles, int count, const void* const* clouds, const size_t* counts,
                               size_t stride_bytes, int on_device);
/* pcl::VoxelGrid<PointXYZI>::filter (centroid per occupied leaf, output ordered by leaf index) fused with
 * setInputSource: the frontend's per-scan `voxel_grid.filter(*filtered); registration_->setInputSource(filtered)`
 * (scanmatcher_component.cpp:324-329) without the filtered cloud ever leaving HBM.  on_device != 0: `pts` is a
 * HIP device pointer.  n_out (nullable) receives the number of points kept. */
int lsr_set_input_source_filtered(lsr_handle h, const void* pts, size_t stride_bytes, size_t n, float leaf, int on_device,
                                  size_t* n_out);
/* The frontend's whole per-scan preprocessing on the device: min-max range filter
 * (`scan_min_range < sqrt(x^2+y^2) < scan_max_range`, scanmatcher_component.cpp:210-218) -> VoxelGrid
 * (vg_size_for_input, :324-328) -> setInputSource (:329).  A sensor_msgs/PointCloud2 payload with x@0,y@4,z@8
 * (point_step = stride_bytes, e.g. 32 for the PointXYZI layout pcl::toROSMsg writes) can be passed as is; other field
 * offsets and the intensity field: lsr_set_input_source_pc2. */
int lsr_set_input_source_frontend(lsr_handle h, const void* pts, size_t stride_bytes, size_t n, double scan_min_range,
                                  double scan_max_range, float vg_size_for_input, int on_device, size_t* n_out);
/* ---- sensor_msgs/PointCloud2 codec ---------------------------------------------
 * A PointCloud2 `data` buffer is `width*height` records of `point_step` bytes with FLOAT32 fields at the byte offsets its
 * `fields` array names; pcl::fromROSMsg (scanmatcher_component.cpp:201-202) reads them wherever they are and
 * pcl::toROSMsg (:279,284; lidarslam_msgs/msg/SubMap.msg:4) writes pcl::PointXYZI's layout {x@0, y@4, z@8, intensity@16,
 * point_step 32}.  The binding passes the message's own offsets; offset_intensity < 0 = the message has none. */
typedef struct lsr_pc2_layout {
  uint32_t point_step;
  uint32_t offset_x, offset_y, offset_z;
  int32_t offset_intensity;
} lsr_pc2_layout;
/* fromROSMsg -> min-max range filter (:210-218) -> VoxelGrid(vg_size_for_input) (:324-328) -> setInputSource (:329) from the
 * raw message payload, on the device.  Intensity is carried the way pcl::VoxelGrid does with its default
 * downsample_all_data: the leaf mean (float accumulation, points in ascending index). */
int lsr_set_input_source_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, double scan_min_range,
                             double scan_max_range, float vg_size_for_input, int on_device, size_t* n_out);
/* toROSMsg of the handle's current input source (e.g. the filtered scan, to publish it or to store it in a SubMap):
 * n records of layout->point_step bytes, x / y / z / intensity at the layout's offsets, every other byte zero. */
int lsr_get_source_pc2(lsr_handle h, void* out_data, size_t capacity_points, const lsr_pc2_layout* layout, size_t* n_out);
/* The same into a DEVICE buffer (d_out: capacity_points records of layout->point_step bytes in HBM): the filtered scan stays resident,
 * e.g. as the newest submap of the frontend's map window — updateMap()'s VoxelGrid(vg_size_for_map) + toROSMsg
 * (scanmatcher_component.cpp:442-446, 466-470) without the 3.5 MB round trip over PCIe; lsr_set_input_target_frames(on_device = 1)
 * takes such buffers.  Returns after the records are complete (any stream may read them). */
int lsr_get_source_pc2_device(lsr_handle h, void* d_out, size_t capacity_points, const lsr_pc2_layout* layout, size_t* n_out);
/* pcl::VoxelGrid::filter, message payload in, message payload out (map side: :266-269, 443-447;
 * graph_based_slam_component.cpp:224-226), intensity averaged per leaf like the coordinates. */
int lsr_voxel_grid_filter_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout, float leaf, void* out_data,
                              size_t capacity_points, const lsr_pc2_layout* out_layout, size_t* n_out);
/* The same filter as a stand-alone operation, host in / host out (map side: scanmatcher_component.cpp:266-269,
 * 443-447; graph_based_slam_component.cpp:224-226).  Writes xyz at offset 0 of each out_stride_bytes record. */
int lsr_voxel_grid_filter(lsr_handle h, const void* pts, size_t stride_bytes, size_t n, float leaf, void* out_pts,
                          size_t out_stride_bytes, size_t out_capacity, size_t* n_out);
/* ---- IMU de-skew of the raw scan (use_imu: scanmatcher_component.cpp:204-208, 501-527) ------------
 * The reference's LidarUndistortion (scanmatcher/include/scanmatcher/lidar_undistortion.hpp) keeps a ring of 200 IMU samples and, per
 * scan, moves every point of the RAW cloud into the sensor frame of the scan's first point before the range filter sees it.  The
 * ring lives in the handle, on the host; the scan is de-skewed on the device, records in, records out, so that the existing
 * lsr_set_input_source_pc2 (and the map side) consume the result unchanged.  Two definitions the reference leaves open: a fresh ring
 * is all zeros, and a sample older than the previous one is refused. */
/* lidar_undistortion_.setScanPeriod / a fresh LidarUndistortion (lidar_undistortion.hpp:229-237): empties the ring; scan_period > 0 */
int lsr_imu_reset(lsr_handle h, double scan_period);
/* lidar_undistortion_.getImu(angular_velo, acc, quat, imu_time)   scanmatcher_component.cpp:525 (lidar_undistortion.hpp:53-106).
 * ang_vel3 / acc3: 3 floats each, acc3 with gravity already removed (:509-511); quat_wxyz4: w x y z.  A stamp smaller than the
 * previous sample's: LSR_ERR_INVALID_ARGUMENT, nothing stored.  Needs no device. */
int lsr_imu_push(lsr_handle h, const float* ang_vel3, const float* acc3, const float* quat_wxyz4, double stamp);
/* ScanMatcherComponent::receiveImu(msg)   scanmatcher_component.cpp:501-527: the same from the fields of a sensor_msgs/Imu message —
 * orientation x y z w, angular velocity, linear acceleration, all double.  Removes gravity from the acceleration with the roll / pitch
 * of the orientation (:505-511) and pushes the sample (lsr_imu_push; same refusal).  The only implementation of that arithmetic: the
 * C++ classes and the Python binding call this entry.  Needs no device. */
int lsr_imu_receive(lsr_handle h, const double* orientation_xyzw4, const double* angular_velocity3, const double* linear_acceleration3,
                    double stamp);
/* inspection: info4 = {samples accepted since the reset, imu_ptr_last_, imu_ptr_last_iter_, 0} */
int lsr_imu_info(lsr_handle h, int32_t* info4);
typedef struct lsr_deskew_info {
  int32_t n_skipped;      /* points left untouched: no IMU sample within scan_period of their time */
  int32_t start_missing;  /* 1 = the scan's first point is one of them: the whole scan is returned unchanged (the reference reads
                             uninitialised values there); the IMU pointer still advances */
  int32_t half_index;     /* first point whose azimuth has passed start + pi (n_points when none does); -1 when nothing ran */
  int32_t cursor;         /* imu_ptr_last_iter_ after the call */
} lsr_deskew_info;
/* lidar_undistortion_.adjustDistortion(tmp_ptr, scan_time)   scanmatcher_component.cpp:207 (lidar_undistortion.hpp:110-226).
 * data: n_points records of layout->point_step bytes in payload order (the order is the scan's time axis); out_data: the same
 * records with x / y / z moved and every other byte copied.  on_device != 0: both are HIP device pointers (ordering rules as for every
 * device input above), equal (in place) or disjoint (ranges that overlap otherwise: LSR_ERR_INVALID_ARGUMENT); the call returns when the
 * records are complete, for a reader on any stream, and performs no device-to-host copy and no stream synchronisation — except
 * when the ring is too short and out_data != data: that plain copy is followed by a synchronisation of the handle's stream.  on_device == 0: both are host pointers, equal or disjoint.  With fewer than two samples in
 * the ring (imu_ptr_last_ <= 0) or n_points == 0 the records are copied unchanged, as the reference leaves them.  info: nullable. */
int lsr_deskew_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, double scan_time, int on_device,
                   void* out_data, lsr_deskew_info* info);
/* inspection, in the style of lsr_ndt_grid_dump: what the last lsr_deskew_pc2 on this handle decided per point (each nullable, n_points
 * entries): rel_time (lidar_undistortion.hpp:153), the ring slot imu_ptr_front_ stood on (:157-162), skipped (:164-166).  Writes
 * nothing when that call moved nothing because the ring was too short. */
int lsr_deskew_trace(lsr_handle h, float* rel_time, int32_t* slot, uint8_t* skipped);

/* ---- raw scan into the robot frame; the use_odom guess (scanmatcher_component.cpp:188-199, 333-348) ------------
 * The cloud callback moves every scan from the sensor frame (msg->header.frame_id) into robot_frame_id_ before anything else reads
 * it: the de-skew, the range filter and the map side are all defined on robot-frame coordinates.  The arithmetic is this library's
 * definition (tf2's source is not part of the reference checkout: restated, unpinned):
 *  - the matrix: translation and quaternion (x y z w, NOT normalised), all double, become a double 4x4 in the expression order every
 *    pose message of the library goes through (Translation * Quaterniond, Eigen's toRotationMatrix); its top three rows are cast to
 *    fp32 element by element;
 *  - the point: x' = ((m00*x + m01*y) + m02*z) + m03, likewise y' and z', every product and sum rounded to fp32, no FMA — the bits
 *    lsr_assemble_map gives the same point and pose;
 *  - a record with a non-finite coordinate comes out with non-finite coordinates, as that arithmetic gives them; every byte of a
 *    record that is not x, y or z is copied. */
typedef struct lsr_sensor_transform {
  double translation[3];        /* geometry_msgs/Transform.translation x y z */
  double rotation_xyzw[4];      /* geometry_msgs/Transform.rotation x y z w */
} lsr_sensor_transform;
/* tfbuffer_.lookupTransform(robot_frame_id_, msg->header.frame_id, time_point)   scanmatcher_component.cpp:193-194: the result as the
 * kernels use it — out12 = rows 0-2 of the fp32 matrix, row-major.  Needs no device and no handle. */
int lsr_sensor_transform_matrix(const lsr_sensor_transform* tf, float* out12);
/* tf2::doTransform(*msg, transformed_msg, transform)   scanmatcher_component.cpp:195
 * data: n_points records of layout->point_step bytes; out_data: the same records with x / y / z moved.  on_device != 0: both are HIP
 * device pointers (ordering rules as for every device input above), equal (in place) or disjoint (ranges that overlap otherwise:
 * LSR_ERR_INVALID_ARGUMENT); the call returns when the records are complete, for a reader on any stream, and performs no
 * device-to-host copy and no stream synchronisation.  on_device == 0: both are host pointers, equal or disjoint (upload, kernel,
 * download).  n_points == 0: LSR_OK, nothing is touched.  This is the form in front of lsr_deskew_pc2 on the use_imu path (:204-208 read
 * the transformed cloud) and the one a host-side map path uses; without IMU the scan side needs no pass of its own:
 * lsr_set_input_source_pc2_tf. */
int lsr_transform_pc2(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, const lsr_sensor_transform* tf,
                      int on_device, void* out_data);
/* lsr_set_input_source_pc2 from a payload in the SENSOR frame: doTransform (:195) -> fromROSMsg (:201-202) -> range filter (:210-218) ->
 * VoxelGrid (:324-328) -> setInputSource (:329).  The transform is applied as the records are read, in the one launch that also filters
 * the range and takes the bounding box — both see robot-frame points; the source is, bit for bit, what lsr_transform_pc2 followed by
 * lsr_set_input_source_pc2 leaves.  tf == NULL: exactly lsr_set_input_source_pc2. */
int lsr_set_input_source_pc2_tf(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout,
                                const lsr_sensor_transform* tf, double scan_min_range, double scan_max_range, float vg_size_for_input,
                                int on_device, size_t* n_out);
/* receiveCloud's use_odom guess   scanmatcher_component.cpp:333-348
 * sim_trans16: the previous pose (getTransformation(corrent_pose_stamped_.pose), :331); odom16: odom_frame_id_ -> robot_frame_id_ at the
 * scan's stamp as a matrix (:342-343); previous_odom16: the same of the scan before, the identity before the first (previous_odom_mat_);
 * all column-major fp32.  previous_odom16 the identity — every entry == its entry of the identity, as Eigen's `previous_odom_mat_ !=
 * Identity()` (:344) compares: the identity's bits, or -0 for a 0 —: guess16 = sim_trans16, bit for bit (the first scan and, a quirk
 * that is kept, an odometry that truly reads identity).  Otherwise guess16 =
 * sim_trans * previous_odom^-1 * odom (:345), computed in double from the fp32 inputs (general 4x4 inverse) and rounded once to fp32.
 * DEVIATION: the reference multiplies in float and inverts with Eigen's Matrix4f::inverse(), a float cofactor inverse whose bits
 * cannot be restated without Eigen's source; this entry is within one rounding of the exact product instead.  The caller keeps
 * previous_odom (:347).  The only implementation: the C++ classes and the Python binding call it.  Needs no device and no handle. */
int lsr_odom_guess(const float* sim_trans16, const float* previous_odom16, const float* odom16, float* guess16);

/* Let `h` register against the target already resident in `owner` (N keyframes vs ONE submap):
 * no copy, the voxel grid / target structures are reference counted. */
int lsr_share_target(lsr_handle h, lsr_handle owner);

/* registration_->align(output, guess)    scanmatcher_component.cpp:353; graph_based_slam_component.cpp:230
 * guess: col-major 4x4 or NULL (= identity, the backend's align(output)).  final_transformation: out, 16 floats.
 * output_pts (nullable): host buffer of n_source records of out_stride_bytes.  PCL's align() copies the source into
 * `output` and then overwrites x, y, z with the transformed coordinates: here ONLY the 12 xyz bytes at offset 0 of every
 * record are written, the rest of each record is left exactly as the caller passed it (pre-fill it with the source
 * records to get PCL's result, other fields included).  Both reference callers discard `output`
 * (scanmatcher_component.cpp:350-353, graph_based_slam_component.cpp:229-230) — pass NULL to skip it. */
int lsr_align(lsr_handle h, const float* guess, float* final_transformation, lsr_result* result,
              void* output_pts, size_t out_stride_bytes);
/* B independent registrations advanced together (loop-closure candidate set / N keyframes vs submap; BASELINE.json cfg 4).
 * NDT: ONE launch chain whose grid covers all B registrations.  GICP (the stand-alone backend's configuration,
 * graph_based_slam/param/graphbasedslam.yaml:3): B launch chains side by side, each on its own object's stream, fed by one
 * host loop — objects created on one shared stream get the same results without the overlap.  All handles must live on the
 * same device and use the same method; an object may appear only once.  guesses: B*16 floats or NULL; finals: B*16 floats;
 * results: B entries. */
int lsr_align_batch(lsr_handle* handles, int batch, const float* guesses, float* finals, lsr_result* results);

/* registration_->getFinalTransformation()  scanmatcher_component.cpp:356; graph_based_slam_component.cpp:244,253 */
int lsr_get_final_transformation(lsr_handle h, float* out16);
/* registration_->hasConverged()            scanmatcher_component.cpp:375 */
int lsr_has_converged(lsr_handle h, int* out);
/* registration_->getFitnessScore(max_range = DBL_MAX)  graph_based_slam_component.cpp:231; scanmatcher_component.cpp:376 */
int lsr_get_fitness_score(lsr_handle h, double max_range, double* out);
/* align() followed by getFitnessScore(max_range) for every candidate of a set in ONE call (graph_based_slam_component.cpp:230-231
 * inside the candidate loop): finals / results as lsr_align_batch, fitness[b] as lsr_get_fitness_score_batch — with the fitness
 * search of every candidate that finishes early running under the launch chain of the ones still registering. */
int lsr_align_fitness_batch(lsr_handle* handles, int count, const float* guesses, float* finals, lsr_result* results, double max_range,
                            double* fitness);

/* registration_->getFitnessScore() of every candidate of a set (graph_based_slam_component.cpp:231 inside the candidate loop):
 * out[b] = what lsr_get_fitness_score(handles[b], max_range, ..) returns; all searches are enqueued before the first wait. */
int lsr_get_fitness_score_batch(lsr_handle* handles, int count, double max_range, double* out);

/* ---- multi-GPU sharding of a batch (BASELINE.json cfg 4) -----------------------
 * One process per GPU.  The batch of `global_count` independent registrations — the loop-closure candidate set of
 * graph_based_slam_component.cpp:188-231 generalised from the nearest candidate to all of them, or N keyframes against
 * a submap — is split by the static block partition lsr_shard_range(); every rank registers its own share with
 * lsr_align_batch (no collective on the data path) and ONE ncclAllGather of fixed 64-byte records over xGMI gives every
 * rank the whole table.  RCCL is loaded on first use; a one-rank communicator needs no RCCL. */
typedef struct lsr_comm_s* lsr_comm;
typedef struct lsr_shard_record {   /* 64 bytes */
  float T[12];                      /* final transformation, ROW-major 3x4 */
  float score;                      /* lsr_result.score */
  float iterations;
  float converged;                  /* 1 / 0 */
  float fitness;                    /* getFitnessScore() when requested, else NaN */
} lsr_shard_record;
/* first index and count of rank's share: the first (n_items % world) ranks get one extra item */
void lsr_shard_range(int n_items, int world, int rank, int* first, int* count);
/* Cost-aware plan for batches whose members differ in size (the ring gate's candidates: targets from a few thousand to
 * 661 k points): longest-processing-time-first — items by cost descending (ties: lower index), each to the least-loaded
 * rank (ties: lower rank).  cost may be NULL; without costs, or with costs the model cannot tell apart (spread within 2 % of the
 * largest), the plan is the block partition of lsr_shard_range.  owner[i] = rank of item i; order = the batch
 * regrouped rank by rank, each rank's items longest first; rank r owns order[rank_first[r] .. rank_first[r+1]).
 * Device-free and deterministic: every rank computes the same plan from the same costs. */
int lsr_shard_plan(int n_items, const double* cost, int world, int32_t* owner /* n_items */, int32_t* order /* n_items */,
                   int32_t* rank_first /* world + 1 */);
/* rank 0: 128-byte ncclUniqueId to hand to the other ranks (by whatever channel the application has) */
int lsr_comm_unique_id(void* id128);
/* every rank: ncclCommInitRank on device_id (id128 may be NULL when world == 1) */
int lsr_comm_create(const void* id128, int rank, int world, int device_id, lsr_comm* out);
int lsr_comm_destroy(lsr_comm c);
/* "N keyframes vs. one submap" across ranks: the rank `root` holds the target cloud — the submap
 * scanmatcher_component.cpp:449-464 assembles and :307 hands to registration_->setInputTarget — and every rank of the communicator
 * ends up with it as the input target of its handle `h`: a 16-byte header {points, stride} by ncclBroadcast, one ncclAllGather of a
 * ready word per rank (the records travel only if every rank can receive them), one ncclBroadcast of the records (device to device
 * over xGMI), then the same voxel grid built on every rank.  pts / stride_bytes / n / on_device are read on the root only.
 * COLLECTIVE: every rank calls it, and a rank that fails locally (bad cloud on the root, no memory, a handle on another device than
 * the communicator) still takes part in every exchange and returns its error afterwards; the other ranks return an error too
 * (LSR_ERR_NO_TARGET when the root had nothing to send) — no rank waits for one that has left.
 * ORDERING of a device-resident root cloud (on_device != 0): the records are read on the COMMUNICATOR's stream, which this call
 * orders behind the handle's stream; the caller orders the handle's stream behind the producer of the records exactly as for
 * lsr_set_input_target_device — lsr_wait_stream(h, producer_stream) or a synchronisation of its own — and keeps the buffer valid
 * until the call returns.  A one-rank communicator hands the cloud straight to lsr_set_input_target(_device).
 * Reference call it generalises: registration_->setInputTarget(targeted_cloud_ptr), one node, one object. */
int lsr_set_input_target_bcast(lsr_comm c, lsr_handle h, const void* pts, size_t stride_bytes, size_t n, int on_device, int root);
/* The pose all-gather on its own (BASELINE.json north_star: "RCCL all-gather of the 6-DoF poses"): every rank contributes `count`
 * 64-byte records — e.g. the scans of its stream, registered one after the other with lsr_align as the frontend does
 * (scanmatcher_component.cpp:353-356) — and receives all world x count of them, rank-major.  COLLECTIVE, same count on every rank. */
int lsr_comm_all_gather_records(lsr_comm c, const lsr_shard_record* local, int count, lsr_shard_record* all_records /* world x count */);
/* local_handles / local_guesses: this rank's share (local_count = lsr_shard_range count), targets and sources already
 * set; with_fitness != 0 adds getFitnessScore() per registration (graph_based_slam_component.cpp:231).
 * all_records: global_count entries, in batch order, identical on every rank. */
int lsr_align_batch_sharded(lsr_comm c, lsr_handle* local_handles, int local_count, int global_count, const float* local_guesses,
                            int with_fitness, lsr_shard_record* all_records);

/* The same with a plan from lsr_shard_plan: local_handles are order[rank_first[rank] ..] in that order (longest first).
 * all_records stays in BATCH order (record of item i at all_records[i]) on every rank. */
int lsr_align_batch_planned(lsr_comm c, lsr_handle* local_handles, int local_count, int global_count, const int32_t* order,
                            const int32_t* rank_first, const float* local_guesses, int with_fitness, lsr_shard_record* all_records);

/* ---- loop-closure gate -------------------------------------------------- */
/* One lidarslam_msgs/msg/SubMap (SubMap.msg:1-4): accumulated travel distance, geometry_msgs/Pose, and the
 * PointCloud2 payload (xyz fp32 at offset 0 of every record of stride_bytes; pose-local coordinates). */
typedef struct lsr_submap {
  double position[3];           /* pose.position x,y,z */
  double orientation[4];        /* pose.orientation x,y,z,w */
  double distance;              /* SubMap.distance */
  const void* cloud;            /* host or HIP device pointer (see on_device) */
  size_t n_points;
} lsr_submap;
/* graph_based_slam parameters used by searchLoop() (graph_based_slam_component.cpp:23-38, defaults in brackets) */
typedef struct lsr_loop_params {
  double threshold_loop_closure_score;     /* [1.0]  accept when fitness < threshold        (:233) */
  double distance_loop_closure;            /* [20.0] minimum travel since the candidate      (:195) */
  double range_of_searching_loop_closure;  /* [20.0] maximum Euclidean distance to candidate (:196) */
  int search_submap_num;                   /* [3]    half-width of the target window         (:209) */
  float voxel_leaf_size;                   /* [0.2]  voxelgrid_ leaf of the assembled target (:61,224-226) */
  int top_k;                               /* 1 = the reference (nearest candidate only); >1 = k nearest candidates */
  int reserved;
} lsr_loop_params;
typedef struct lsr_loop_edge {
  int id_from;                  /* LoopEdge.pair_id.first  = candidate submap index (:240) */
  int id_to;                    /* LoopEdge.pair_id.second = num_submaps - 1 */
  int accepted;                 /* fitness_score < threshold_loop_closure_score */
  int converged;
  int iterations;
  int n_target_points;          /* size of the filtered target window */
  double candidate_distance;    /* |latest - candidate| position distance */
  double fitness_score;         /* getFitnessScore() after align (:231) */
  double relative_pose[16];     /* from^-1 * (final * init), column-major 4x4 fp64 (:241-245) */
  float final_transformation[16];
} lsr_loop_edge;
/* GraphBasedSlamComponent::searchLoop() from `latest_submap` on (graph_based_slam_component.cpp:164-252): the latest
 * submap moved by its pose becomes the source (:171-181), candidates are gated on travelled distance and range and the
 * nearest one is picked (:188-205), its window of 2*search_submap_num+1 submaps is moved, concatenated, voxel filtered and
 * set as target (:207-227), then align() without guess (:230), getFitnessScore() (:231), the threshold (:233) and the
 * relative pose of the edge (:236-245) — clouds stay in HBM from the first transform to the fitness sum.
 * edges: up to edge_capacity entries, nearest candidate first; *n_evaluated = candidates registered (0 = no candidate).
 * Afterwards `h` answers getFinalTransformation / hasConverged for the nearest candidate and holds that candidate's window
 * as its input target — the reference's state after the loop (:227) — whatever top_k was (with top_k > 1 the k windows are
 * built on worker objects and the nearest one's is handed to `h`), so a later getFitnessScore() on `h` scores exactly the
 * pose it reports.
 * The pose-graph optimisation that follows (doPoseAdjustment, :267-319) is lsr_optimize_pose_graph below — no g2o needed —, and what the
 * caller does with the optimiser's poses right afterwards — every submap moved by its new pose, the whole map put together — is
 * lsr_assemble_map; the map.pcd the function ends with (:369) is lsr_save_map_pcd_ascii. */
int lsr_search_loop(lsr_handle h, const lsr_submap* submaps, int num_submaps, size_t stride_bytes, int on_device,
                    const lsr_loop_params* params, lsr_loop_edge* edges, int edge_capacity, int* n_evaluated);

/* ---- loop closure by appearance: Scan Context candidates ------------------ */
/* searchLoop's candidate rule rests on the drifted odometry: a submap is a candidate only when its STORED position is within range of
 * the latest one, and it is registered without a guess.  After a long featureless stretch the right keyframe is outside that range
 * and a wrong one inside it.  These entries pick the candidate and its heading by what the place looks like: a Scan Context descriptor
 * per keyframe (Kim and Kim, IROS 2018: the highest point of every ring x sector cell of a polar grid around the sensor), every stored
 * descriptor compared with the latest one at every yaw shift, both on the device.  No reference site exists: the definitions are this
 * project's (unpinned).  They use integer and single-rounded fp32 operations only — every fp32 product, sum, difference, quotient and
 * square root below is rounded once, nothing is fused —, so a numpy float32 restatement has the same bits (tests/scan_context_numpy.py).
 *
 * Parameters: num_rings R in 1 .. 40, num_sectors S even in 2 .. 120, max_radius L > 0, z_offset (the sensor's height above ground).
 * Tables, made on the host in double and rounded to float once:
 *   edge2[k] = (float)((k L / R)^2) for k = 1 .. R-1, L2 = (float)(L L);
 *   b[k] = ((float)cos(2 pi k / S), (float)sin(2 pi k / S)) for k = 1 .. S/2-1 (the C library's cos and sin).
 * The descriptor of a cloud (pose-local records, x y z at the layout's offsets), R x S floats, ring-major:
 *   1. a point with a non-finite coordinate is skipped;
 *   2. r2 = x x + y y (two products, one sum); a point with r2 >= L2 is skipped;
 *   3. ring = the number of k in 1 .. R-1 with r2 >= edge2[k];
 *   4. the point is in the upper half if y > 0 || (y == 0 && x >= 0), and then (x', y') = (x, y); else in the lower half with
 *      (x', y') = (-x, -y).  sector = (lower ? S/2 : 0) + the number of k in 1 .. S/2-1 with b[k].x y' - b[k].y x' >= 0 (two products,
 *      one difference).  No angle function is used;
 *   5. the cell's value is the maximum over its points of max(+0, z + (float)z_offset) (a sum that is not > 0 counts as +0); an empty
 *      cell is +0.
 *   The result does not depend on the order of the points: one definition, one set of bits whatever the launch form.
 * The distance of a query q to a candidate c at shift n pairs query column j with candidate column (j + n) mod S — the candidate sees
 * the query's scene turned by +n 2 pi / S about z:
 *   1. column norms nq_j = sqrtf(sum_r q q), nc_j = sqrtf(sum_r c c) and dot_j = sum_r q c: r ascending from 0.0f, product then sum;
 *   2. a column counts when both norms are > 0; term_j = 1.0f - dot_j / (nq_j nc_j);
 *   3. d(n) = (sum of the terms, j ascending from 0.0f) / (float)count; no column counts: d(n) = 1.0f;
 *   4. the distance is the minimum over n, ties to the lowest n; candidates of equal distance rank by ascending index.
 * The guess: G = M_cand Rz(shift 2 pi / S) M_latest^-1 in fp64 from the two stored poses (the matrices of lsr_search_loop), cast to
 * float element by element — lsr_align's guess for a source that is the latest cloud moved by its stored pose. */
#define LSR_SCAN_CONTEXT_MAX_RINGS 40
#define LSR_SCAN_CONTEXT_MAX_SECTORS 120
typedef struct lsr_scan_context_params { int32_t num_rings, num_sectors; double max_radius, z_offset; } lsr_scan_context_params;
/* The two tables.  Host only, no handle.  edge2: R floats — edge2[k-1] for k = 1 .. R-1, then L2; boundaries: S - 2 floats — cos, sin
 * of k = 1 .. S/2-1 (none for S = 2; the pointer is still required).  LSR_ERR_INVALID_ARGUMENT, outputs untouched: a null pointer, R or S
 * out of range, S odd, L not > 0 or not finite, z_offset not finite. */
int lsr_scan_context_tables(const lsr_scan_context_params* params, float* edge2, float* boundaries);
/* The guess G above -> guess16 (column-major float).  Host only, no handle.  0 <= shift < num_sectors, num_sectors even in 2 .. 120. */
int lsr_scan_context_guess(const lsr_submap* candidate, const lsr_submap* latest, int shift, int num_sectors, float* guess16);
/* The descriptors of num_submaps submaps in ONE launch over a device table of them (the shape of lsr_assemble_map): submaps[i].cloud =
 * n_points records of `layout` (x / y / z at its offsets; the intensity offset is not read), all host pointers (on_device == 0: staged
 * through the object's upload buffer in bounded pieces) or all HIP device pointers -> out_desc[i R S ..], host or (out_on_device != 0)
 * device.  A submap without points has an all-zero descriptor.  The cells are unsigned integer maxima on the float bits (the values
 * are >= +0, where the two orders agree), in LDS per workgroup, merged in the output where a submap is split over workgroups.
 * The call keeps no state: submaps + k with out_desc + k R S writes the bytes a call over all submaps writes there — a caller appends
 * one descriptor per new keyframe.  Ordering of device inputs: as for lsr_assemble_map; returns when the descriptors are complete.
 * LSR_ERR_INVALID_ARGUMENT, outputs untouched: null handle, submaps, layout, params or out_desc; num_submaps <= 0; a layout
 * lsr_deskew_pc2 refuses; parameters lsr_scan_context_tables refuses; a pointer that is not 4-byte aligned; n_points > 0 without a
 * cloud.  LSR_ERR_INDEX_OVERFLOW: more than INT32_MAX records in all.  LSR_SCAN_CONTEXT_BUILD_MS reports the launches' time. */
int lsr_scan_context_build(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* layout, int on_device,
                           const lsr_scan_context_params* params, float* out_desc, int out_on_device);
/* nq queries against nc candidates, every pair at every shift, in ONE launch: one workgroup per pair, the candidate in LDS with its
 * columns doubled, one lane per shift walking columns and rings in the order the definition fixes.  q, c: nq and nc descriptors of
 * R x S floats, both host or (on_device != 0) both device; dist[iq nc + ic], shift[iq nc + ic]: host.  Brute force over every stored
 * descriptor is the device's answer to a ring-key tree.  LSR_ERR_INVALID_ARGUMENT, outputs untouched: a null pointer, a count < 1,
 * refused parameters, q or c not 4-byte aligned; LSR_ERR_INDEX_OVERFLOW: more than INT32_MAX pairs.  LSR_SCAN_CONTEXT_MATCH_MS reports
 * the launch's time. */
int lsr_scan_context_match(lsr_handle h, const float* q, int nq, const float* c, int nc, int on_device,
                           const lsr_scan_context_params* params, float* dist, int32_t* shift);
/* The loop gate with candidate and heading from appearance and the translation from the pose search.
 * descriptors: num_descriptors x R x S floats, host or (desc_on_device != 0) device, descriptor i of submap i (lsr_scan_context_build);
 * the latest one is compared with all of them in one launch.  Candidates: the submaps with latest.distance - distance_i >
 * loop.distance_loop_closure AND Scan Context distance < sc_distance_threshold, ranked by that distance (ties: lower index).  The range
 * gate (range_of_searching_loop_closure) is NOT applied: it is the drifted position this entry exists to do without.  The first
 * max(loop.top_k, 1) candidates (at most edge_capacity) are evaluated one after another on `h`: source and window target exactly as
 * lsr_search_loop builds them; then, NDT: lsr_ndt_search_pose with `search` around G (a search that keeps nothing leaves G itself as the
 * final transformation, not converged); GICP: one align with guess G; then getFitnessScore, the threshold and the relative pose
 * from^-1 (final init), as lsr_search_loop fills them — candidate_distance stays the position distance.  shifts[e] and sc_dist[e] beside
 * edges[e] (both nullable).  Afterwards `h` holds the first candidate's result and window as its input target, as lsr_search_loop leaves
 * it.  No candidate: LSR_OK with *n_evaluated = 0.
 * LSR_ERR_INVALID_ARGUMENT, outputs untouched: what lsr_search_loop refuses; null descriptors or params; num_descriptors !=
 * num_submaps; Scan Context parameters lsr_scan_context_tables refuses; a threshold that is NaN; NDT with a search top_k outside 1 .. 16.
 * (Declared below, behind lsr_pose_search_params, which its parameters hold.) */

/* ---- the whole map from its submaps -------------------------------------- */
/* ScanMatcherComponent::publishMap (scanmatcher_component.cpp:529-552) and the map half of doPoseAdjustment
 * (graph_based_slam_component.cpp:321-368): every submap of a lidarslam_msgs/MapArray is moved by its pose and the records are
 * concatenated, submap after submap, record after record (`*map_ptr += ...`), in ONE launch over a device table of the submaps.
 * submaps[i].cloud: n_points records of in_layout (x / y / z / intensity at its offsets; offset_intensity < 0: intensity 0), all host
 * pointers (on_device == 0: staged through the handle's upload buffer in bounded pieces) or all HIP device pointers.
 * Poses: poses16 == NULL — each submap's own position / orientation (tf2::fromMsg -> .matrix().cast<float>(), publishMap :538-542);
 * poses16 != NULL — num_submaps column-major fp64 4x4 matrices instead (the optimiser's vertex->estimate(), :329-342), cast to float
 * element by element.  A point is moved in fp32 as ((m00*x + m01*y) + m02*z) + m03, no FMA: the bits lsr_set_input_target_frames
 * gives the same point and pose.  Non-finite coordinates are moved and written like any others; nothing is dropped.
 * Output: records of out_layout, x' y' z' intensity at its offsets (offset_intensity < 0: not written), every other byte of a record
 * zero, into out_data — a HIP device buffer (out_on_device != 0: the map stays in HBM) or a host buffer — of capacity_points records.
 * *n_out = the sum of the n_points.  first_record (nullable, num_submaps + 1 entries): index of each submap's first record, the last
 * entry the total — records [first_record[i], first_record[i+1]) are the moved cloud of submap i as it stands
 * (modified_map_array.submaps[i].cloud, :343-351), no second pass.
 * Appending: the call keeps no state.  submaps + k (and poses16 + 16 k) with out_data advanced by first_record[k] records writes
 * exactly the records a call over all submaps writes there — a frontend whose old poses never change extends a resident map by its
 * new keyframes only.
 * Ordering and lifetime of device inputs: as for every device input above (reads on the handle's stream, lsr_wait_stream for a foreign
 * producer).  Returns when the records are complete, for a reader on any stream.
 * LSR_ERR_INVALID_ARGUMENT: null handle, layout, submaps or n_out; num_submaps <= 0; a point_step that is not a multiple of 4; a field
 * that does not fit in its record; output fields that overlap; a pointer that is not 4-byte aligned; a submap with n_points > 0 and no
 * cloud; capacity_points below the total; an output range that overlaps an input cloud.  LSR_ERR_INDEX_OVERFLOW: more than INT32_MAX
 * records in all.  A total of zero is LSR_OK with *n_out = 0.  Outputs are left untouched on every error.
 * LSR_MAP_ASSEMBLY_FORM tells which of the two kernel forms ran; the bytes do not depend on it, nor on where the buffers live. */
int lsr_assemble_map(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout, int on_device,
                     const double* poses16 /* nullable */, void* out_data, size_t capacity_points,
                     const lsr_pc2_layout* out_layout, int out_on_device, size_t* first_record /* nullable */, size_t* n_out);

/* ---- moving objects out of the map: visibility votes ---------------------- */
/* lsr_assemble_map keeps every record of every keyframe: a car that drove ahead of the vehicle is in the map once per keyframe that saw
 * it, a streak along the lane, and the voxel filter thins the streak and keeps it.  A keyframe whose beam reached a surface BEHIND a
 * stored point saw through that point: the point was not there at that time.  These entries make that z-buffer test per (record,
 * neighbouring keyframe) on the device and assemble the map of the records with fewer than min_votes such votes against them.  No
 * reference site exists: the definition is this project's (unpinned).  It uses integer and single-rounded fp32 operations only — every
 * fp32 product, sum, difference, quotient and square root below is rounded once, nothing is fused —, so a numpy float32 restatement has
 * the same bits (tests/map_visibility_numpy.py).
 *
 * Parameters (defaults of the bindings in brackets): face_width W [128] even in 8 .. 1024, the columns per 90 degrees; height H [32] in
 * 4 .. 512, the rows; max_tan_elevation T [tan 30 deg] > 0; min_range [0.5] < max_range [80], both finite, max_range > 0; margin [0.5]
 * >= 0, metres; keyframe_range [30] > 0; max_neighbours [32] in 1 .. 64; min_votes [2] >= 1; sensor_origin [0, 0, 0], the lidar in the
 * keyframe's frame.  Constants, made on the host in double and rounded to float once: hw = (float)(W / 2), Tf = (float)T,
 * rs = (float)(H / (2 T)), and the floats of min_range, max_range, margin and the origin.
 *   1. The pixel of a sensor-centred point (x, y, z).  The depth image is H rows x 4 W columns: the four side faces of a cube laid side
 *      by side, with column wrap.  A point with a non-finite coordinate has no pixel.  d = max(|x|, |y|); d == 0: no pixel.
 *      |x| >= |y|: face = (x > 0 ? 0 : 2), u = y / x; else face = (y > 0 ? 1 : 3), u = -x / y — azimuth ascends with the column across
 *      all four faces.  r = sqrtf((x x + y y) + z z); r < min_range or r >= max_range: no pixel.  v = z / d,
 *      rowf = floorf((v + Tf) * rs), the row test made in float: rowf < 0, rowf >= H or a row that is not finite: no pixel.
 *      col = face W + min(W - 1, (int)floorf((u + 1.0f) * hw)).  No angle function is used.
 *   2. The depth image of a keyframe: D[row][col] = the minimum of r over the keyframe's own records, sensor_origin subtracted
 *      component-wise before step 1, that have a pixel; an empty pixel is +inf (bits 0x7f800000).  An unsigned integer minimum on the
 *      float bits (r >= +0, where the two orders agree): the image does not depend on point order or launch form.
 *   3. The eroded image: E[row][col] = the minimum of D over rows row-1 .. row+1 clamped to 0 .. H-1 and columns col-1 .. col+1 modulo
 *      4 W.  This is what is compared against: a point counts as seen through only when every beam around its direction went further.
 *   4. Neighbours and transforms (host, fp64).  The poses are poses16 when given, else the stored ones (the matrices lsr_assemble_map
 *      uses).  N(i) = the keyframes k != i with |t_k - t_i| <= keyframe_range, of which the max_neighbours nearest are kept (ties to the
 *      lower index), listed in ascending k.  T_ki = M_k^-1 M_i with the rigid inverse (R^T, -R^T t); its first three rows cast to float
 *      element by element.
 *   5. The votes of record p of keyframe i.  For each k in N(i): q = ((m00 x + m01 y) + m02 z) + m03 row by row with T_ki's floats (the
 *      expression of lsr_assemble_map), sensor_origin subtracted, the pixel by step 1; one vote when the pixel exists, E_k there is
 *      finite and r + margin < E_k[pixel] (one sum, one compare).  A record without a pixel anywhere has 0 votes and is kept.
 *   6. The static map: the records of lsr_assemble_map (same poses, same bytes per record) whose votes are below min_votes, in input
 *      order; first_record indexes the kept records. */
#define LSR_VISIBILITY_MAX_FACE_WIDTH 1024
#define LSR_VISIBILITY_MAX_HEIGHT 512
#define LSR_VISIBILITY_MAX_NEIGHBOURS 64
typedef struct lsr_visibility_params {
  int32_t face_width, height;
  double max_tan_elevation, min_range, max_range, margin, keyframe_range;
  int32_t max_neighbours, min_votes;
  double sensor_origin[3];
} lsr_visibility_params;
/* Step 4.  Host only, no handle.  The clouds of the submaps are not looked at.  first_pair: num_submaps + 1 entries — the pairs of
 * keyframe i are [first_pair[i], first_pair[i+1]); other[p] = k; rel12[12 p ..] = the first three rows of T_ki, row-major.  *n_pairs =
 * the number of pairs (at most num_submaps x min(max_neighbours, num_submaps - 1)); more than capacity_pairs of them:
 * LSR_ERR_INVALID_ARGUMENT with *n_pairs set and the tables untouched.  LSR_ERR_INVALID_ARGUMENT, outputs untouched: a null pointer
 * (poses16 may be null), num_submaps < 1, a parameter outside the ranges above. */
int lsr_visibility_pairs(const lsr_submap* submaps, int num_submaps, const double* poses16 /* nullable */,
                         const lsr_visibility_params* params, int32_t* first_pair, int32_t* other, float* rel12, size_t capacity_pairs,
                         size_t* n_pairs);
/* Steps 1 - 3: the depth image (eroded == 0: D, else E) of num_submaps submaps in ONE launch over a device table of them, the erosion in
 * one more over all images.  submaps, layout, on_device: as for lsr_scan_context_build -> out_images[i H 4W ..], host or
 * (out_on_device != 0) device.  A pixel is lowered by an unsigned minimum straight in the image: at 16 384 pixels for the few ten
 * thousand records of a keyframe a copy in LDS costs more to clear and merge than the atomics it saves, so there is one launch form.
 * The call keeps no state: submaps + k with out_images advanced by k images writes the bytes a call over all submaps writes there —
 * a caller appends one image per new keyframe.  LSR_ERR_INVALID_ARGUMENT, outputs untouched: what lsr_scan_context_build refuses, with
 * these parameters.  LSR_ERR_INDEX_OVERFLOW: more than INT32_MAX records in all.  LSR_DEPTH_IMAGES_MS reports the launches' time. */
int lsr_depth_images_build(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* layout, int on_device,
                           const lsr_visibility_params* params, int eroded, float* out_images, int out_on_device);
/* Step 5: votes[g] for every record in assembly order (g = first_record[i] + p), int32, host or (votes_on_device != 0) device; one lane
 * per record, a workgroup never straddles a submap (the pair list and the 12 floats of a pair are uniform loads, the pixel of E the one
 * gather per pair).  images: the num_submaps ERODED images, host or (images_on_device != 0) device.  first_record (nullable,
 * num_submaps + 1 entries) and *n_records as lsr_assemble_map fills them.  Refusals as lsr_depth_images_build; null images, votes or
 * n_records too.  LSR_VISIBILITY_MS reports the launch's time. */
int lsr_visibility_votes(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* layout, int on_device,
                         const double* poses16 /* nullable */, const float* images, int images_on_device,
                         const lsr_visibility_params* params, int32_t* votes, int votes_on_device, size_t* first_record /* nullable */,
                         size_t* n_records);
/* Step 6.  lsr_assemble_map's arguments and rules, plus the eroded images and the parameters: the votes, the raw map in a buffer kept on
 * the object, then flags -> scan -> write in input order (the scan and the ranking of lsr_crop_map; one host wait, for the count).
 * *n_out = the records kept, *n_removed = the records left out; first_record indexes the kept records.  out_data == NULL: only the
 * counts and first_record are set (capacity_points is ignored).  capacity_points below the count: LSR_ERR_INVALID_ARGUMENT, outputs
 * untouched.  num_submaps == 1, or a pair table that is empty, gives lsr_assemble_map's bytes.  LSR_VISIBILITY_MS reports the votes and
 * the three launches of the compaction. */
int lsr_assemble_map_static(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout, int on_device,
                            const double* poses16 /* nullable */, const float* images, int images_on_device,
                            const lsr_visibility_params* params, void* out_data, size_t capacity_points,
                            const lsr_pc2_layout* out_layout, int out_on_device, size_t* first_record /* nullable */, size_t* n_out,
                            size_t* n_removed);

/* ---- map.pcd -------------------------------------------------------- */
/* pcl::io::savePCDFileASCII("map.pcd", *map_ptr) at the end of doPoseAdjustment (graph_based_slam_component.cpp:369, "too heavy"; reached
 * by the map_save service, :96-103, and by every accepted loop closure under use_save_map_in_loop): the file's bytes are formatted on the
 * device.  The format (restated, unpinned): the v0.7 header of a cloud of width n and height 1 with default viewpoint —
 * FIELDS x y z intensity, or x y z for a layout with offset_intensity < 0 —, then one line per record in record order, the fields
 * separated by one blank, each the C library's "%.8g" of the float promoted to double (exact binary value, correctly rounded to 8
 * significant digits, ties to even; trailing zeros dropped; exponent form below 1e-4 and from 1e8; "-0"; "inf" / "-inf"), any NaN "nan". */
#define LSR_PCD_ASCII_MAX_LINE_BYTES 60    /* four fields of 14 bytes ("-1.1754944e-38"), three blanks, the newline */
#define LSR_PCD_ASCII_MAX_HEADER_BYTES 256 /* the header is shorter than this */
/* The whole file image, header and body, of n_points records of `layout` (host pointer, or HIP device pointer with on_device != 0) into
 * out_text (host, or HIP device buffer with out_on_device != 0; any alignment) of capacity_bytes; *n_bytes = the image's size.
 * out_text == NULL: only *n_bytes is set (the length pass runs; capacity_bytes is ignored).  Layout rules and the ordering rules of device
 * inputs: as for lsr_assemble_map.  Returns when the text is complete, for a reader on any stream.
 * LSR_ERR_INVALID_ARGUMENT: null handle, data, layout or n_bytes; a layout lsr_assemble_map refuses; data or a field not 4-byte aligned;
 * n_points == 0 (PCL refuses an empty cloud too); capacity_bytes below the size.  LSR_ERR_INDEX_OVERFLOW: more than INT32_MAX records.
 * No error touches out_text or *n_bytes.  What the object answers afterwards (target, source, final transformation, fitness) is unchanged,
 * as for the two entries below. */
int lsr_format_pcd_ascii(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device, void* out_text,
                         size_t capacity_bytes, int out_on_device, size_t* n_bytes);
/* The same image written to the file `path` (created or truncated), in pieces of LSR_PCD_PIECE_RECORDS records through two pinned buffers
 * kept on the object: piece k + 1 is formatted and copied on the object's stream while the calling thread fwrites piece k.  A host input
 * is staged piece by piece.  The file's bytes do not depend on the piece size or on where the input lives.  *n_bytes = the file's size.
 * Errors as above, and LSR_ERR_INVALID_ARGUMENT for a null path; LSR_ERR_IO, with errno's text in lsr_last_error(), when the file cannot
 * be opened or a write comes up short.  On any error after the file was opened it is closed and removed. */
int lsr_save_pcd_ascii(lsr_handle h, const char* path, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device,
                       size_t* n_bytes);
/* `if (do_save_map) pcl::io::savePCDFileASCII("map.pcd", *map_ptr)` (:369) in one call: lsr_assemble_map of the submaps (same arguments,
 * same launch, hence the same coordinate bits) into a device buffer of pcl::PointXYZI records {32; 0, 4, 8, 16} kept on the object, then
 * lsr_save_pcd_ascii from that buffer.  The file is byte-equal to those two calls made one after the other.  Errors: those of the two;
 * a map without any record is LSR_ERR_INVALID_ARGUMENT. */
int lsr_save_map_pcd_ascii(lsr_handle h, const char* path, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout,
                           int on_device, const double* poses16 /* nullable */, size_t* n_bytes);

/* ---- map.pcd as DATA binary and DATA binary_compressed ---------------------------------------- */
/* The same three entries with the body kind as an argument.  LSR_PCD_ASCII calls the entry above and gives its bytes; any value that is
 * not one of the three is LSR_ERR_INVALID_ARGUMENT.  The formats (restated, unpinned, like SURVEY.md 9.10):
 * Header: the text of the ASCII file — FIELDS x y z intensity, or x y z for a layout with offset_intensity < 0; SIZE 4, TYPE F, COUNT 1;
 * width n, height 1, default viewpoint — with the last line "DATA binary\n" or "DATA binary_compressed\n".
 * Binary body: n PACKED records of 12 or 16 bytes, the three or four fields copied bit for bit (NaN payloads, -0, denormals).  A stated
 * deviation: pcl::io::savePCDFileBinary of a pcl::PointXYZI cloud writes the 32-byte struct, `_` padding fields with uninitialised bytes
 * included; every PCD reader, PCL's too, loads the packed file into the same points, and it is half the size.
 * Compressed body: uint32 compressed_size, uint32 uncompressed_size, little endian, then ONE LZF stream whose inflation is the
 * field-major image — per field, in header order, a block of 4 n bytes — exactly what lsr_decode_pcd reads (above).  The stream is a
 * PURE FUNCTION OF THE IMAGE (not of the piece size, of where input or output live, of the object or the call): the image is cut into
 * chunks of LSR_PCD_LZF_CHUNK_BYTES (the last may be shorter), each compressed on its own — no reference reaches before its chunk's
 * first byte, so the chunks' streams back to back are one valid stream —, a workgroup per chunk (csrc/pcd_deflate.hip).  Inside a chunk:
 * the candidate of a position i with three bytes left in the chunk is the nearest earlier position of the chunk with the same three
 * bytes (exact comparison); its length is the common extension, at most 264 and up to the chunk's end; the parse is greedy from the
 * chunk's first byte (with a candidate a reference and on by its length, else a literal and on by one); literals go out in runs of at
 * most 32, a run ends at a reference and at the chunk's end; a reference of length <= 8 has the two-byte form, from 9 the three-byte
 * form.  uncompressed_size or a stream above 2^31 - 1 bytes is LSR_ERR_INDEX_OVERFLOW (the reader's own limit). */
#define LSR_PCD_LZF_CHUNK_BYTES 4096
typedef enum lsr_pcd_data { LSR_PCD_ASCII = 0, LSR_PCD_BINARY = 1, LSR_PCD_BINARY_COMPRESSED = 2 } lsr_pcd_data; /* = lsr_pcd_info.data_kind */
/* lsr_format_pcd_ascii with a body kind: the whole file image into out_image (host, or HIP device buffer with out_on_device != 0; any
 * alignment); out_image == NULL: only *n_bytes is set.  Same argument checks and refusals; no error touches out_image or *n_bytes.  A
 * compressed image is compressed in HBM whole: the field-major image, the chunks' streams and the stream are kept on the object. */
int lsr_format_pcd(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device, int data_kind,
                   void* out_image, size_t capacity_bytes, int out_on_device, size_t* n_bytes);
/* lsr_save_pcd_ascii with a body kind: the same image written to `path`, without seeking.  Binary: in pieces of LSR_PCD_PIECE_RECORDS
 * records through the object's two pinned buffers, piece k + 1 packed and copied while the calling thread writes piece k; no size limit
 * but INT32_MAX records.  Compressed: the size words precede the stream, so the whole cloud is compressed in HBM first, the total read
 * back, header and size words written, and the stream copied and written in pieces through the same two buffers.  Errors as for
 * lsr_save_pcd_ascii: a file that fails after it was opened is closed and removed. */
int lsr_save_pcd(lsr_handle h, const char* path, const void* data, size_t n_points, const lsr_pc2_layout* layout, int on_device, int data_kind,
                 size_t* n_bytes);
/* lsr_save_map_pcd_ascii with a body kind: lsr_assemble_map into the object's XYZI buffer, then lsr_save_pcd from it; byte-equal to
 * those two calls. */
int lsr_save_map_pcd(lsr_handle h, const char* path, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout,
                     int on_device, const double* poses16 /* nullable */, int data_kind, size_t* n_bytes);
/* The compressor alone: the LZF stream, under the rule above, of the n_image bytes (1 .. 2^31 - 1; any alignment; host, or HIP device
 * pointer with on_device != 0) at `image`, into out_stream (host, or HIP device buffer with out_on_device != 0) of capacity_bytes;
 * *n_bytes = the stream's length, at most the sum over the chunks of c + ceil(c / 32).  out_stream == NULL: only *n_bytes is set.  What a
 * compressed lsr_format_pcd puts behind its size words is this stream of the field-major image.  LSR_ERR_INVALID_ARGUMENT: null handle,
 * image or n_bytes; n_image == 0; capacity_bytes below the length.  LSR_ERR_INDEX_OVERFLOW: n_image above 2^31 - 1.  No error touches
 * out_stream or *n_bytes.  LSR_PCD_DEFLATE_MS covers it (without a gather). */
int lsr_lzf_deflate(lsr_handle h, const void* image, size_t n_image, int on_device, void* out_stream, size_t capacity_bytes,
                    int out_on_device, size_t* n_bytes);

/* ---- thinning the whole map: pcl::VoxelGrid with a 64-bit leaf index ------------------------- */
/* What publishMap (scanmatcher_component.cpp:529-552) publishes and doPoseAdjustment (graph_based_slam_component.cpp:321-369) saves is the
 * raw concatenation of the submaps: with a keyframe every metre or two and a sensor range of 100 m every spot is stored dozens of
 * times.  These entries thin a map-sized cloud with a leaf size on the device, records in and records out.  pcl::VoxelGrid itself and
 * lsr_voxel_grid_filter / _pc2 above carry the leaf index in int32 and refuse a cloud whose grid has more than INT32_MAX cells (a
 * 500 m x 500 m x 40 m map at a 0.1 m leaf has 10^10); here the index has 64 bits.  The definition (csrc/map_filter.hip), otherwise
 * that of lsr_voxel_grid_filter_pc2:
 *   Bounding box: only records with finite x, y and z take part, the others are dropped.  inv_leaf = 1.0f / leaf; mn, mx = the
 *   bounding box of the finite points.
 *   Cells: min_b[k] = (int)floorf(mn[k] * inv_leaf), max_b[k] likewise, div_b[k] = max_b[k] - min_b[k] + 1; the cell of a point p is
 *   c[k] = (int)(floorf(p[k] * inv_leaf) - (float)min_b[k]) — float arithmetic, one multiply, no FMA.
 *   Leaf index: c0 + c1 * div_b0 + c2 * div_b0 * div_b1 in int64: wherever lsr_voxel_grid_filter_pc2 accepts the cloud, the number it uses.
 *   Output: one record per occupied leaf, in ascending leaf index; x, y, z and intensity are each the float sum of the leaf's points
 *   in ascending input index divided by (float) count.  An input layout without intensity yields intensity 0; an output layout
 *   without intensity has no such field.  Every other byte of an output record is zero.
 *   Limits, both LSR_ERR_INDEX_OVERFLOW: any |min_b[k]| or |max_b[k]| >= 2^24 (a float coordinate carries no leaf resolution there;
 *   below it the float subtraction above is exact and equals PCL's integer one); any div_b[k] > 2^21 (so the index stays below
 *   2^63).  Records: at most INT32_MAX / 2 in one call (what the sort orders), LSR_ERR_INDEX_OVERFLOW beyond.
 *   Consequence: for every cloud lsr_voxel_grid_filter_pc2 accepts this filter returns the same bytes.  The output does not depend on
 *   where the buffers live and is bit-identical from call to call.
 * lsr_voxel_grid_filter_map: n_points records of in_layout at `data` (host, or HIP device pointer with on_device != 0) -> records of
 * out_layout at out_data (host, or HIP device buffer with out_on_device != 0) of capacity_points records; *n_out = the number of occupied
 * leaves.  out_data == NULL: only *n_out is set (capacity_points is ignored).  capacity_points below the count: LSR_ERR_INVALID_ARGUMENT
 * with *n_out set to the count and out_data untouched.  A cloud without a finite point (n_points == 0 too) is LSR_OK with *n_out = 0.
 * Layout, alignment and device-input ordering rules: those of lsr_assemble_map; LSR_ERR_INVALID_ARGUMENT also for a leaf that is not > 0
 * (NaN included) and for an output range that overlaps the input records.  Every other error leaves all outputs untouched.  Two host
 * waits per call: one for the bounding box, one for the leaf count, which sizes the output.  The scratch is kept on the object; a failed
 * reservation is LSR_ERR_HIP.  What the object otherwise answers (target, source, final transformation, fitness) is unchanged.
 * LSR_MAP_FILTER_KEY_BITS reports the index bits of the last call. */
int lsr_voxel_grid_filter_map(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout, int on_device, float leaf,
                              void* out_data, size_t capacity_points, const lsr_pc2_layout* out_layout, int out_on_device, size_t* n_out);
/* lsr_assemble_map into a buffer of pcl::PointXYZI records kept on the object (the one lsr_save_map_pcd assembles into), followed by the
 * filter from it: the bytes of those two calls made apart, the raw map never leaving HBM.  No first_record: a leaf mixes submaps.
 * Arguments and errors: those of the two; out_data == NULL and a capacity below the count as above. */
int lsr_assemble_map_filtered(lsr_handle h, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout, int on_device,
                              const double* poses16 /* nullable */, float leaf, void* out_data, size_t capacity_points,
                              const lsr_pc2_layout* out_layout, int out_on_device, size_t* n_out);
/* That, into a second buffer of pcl::PointXYZI records kept on the object, followed by lsr_save_pcd from it with data_kind: the file is
 * byte-equal to the steps made apart.  *n_points (nullable) = the records in the file, *n_bytes = its size.  A map without a finite
 * point is LSR_ERR_INVALID_ARGUMENT, like an empty one. */
int lsr_save_map_pcd_filtered(lsr_handle h, const char* path, const lsr_submap* submaps, int num_submaps, const lsr_pc2_layout* in_layout,
                              int on_device, const double* poses16 /* nullable */, float leaf, int data_kind,
                              size_t* n_points /* nullable */, size_t* n_bytes);

/* ---- localising in a saved map: the target cut from the resident map ------------------------- */
/* A saved map is far larger than what one scan can meet, and setInputTarget lays one int32 cell table over the bounding box of whatever
 * it is given (a 6 km x 6 km x 600 m map at resolution 1.0 is LSR_ERR_INDEX_OVERFLOW).  These entries cut the records inside a box of
 * voxel cells around the pose out of the resident map, in input order, on the device, and build the ordinary target from them.
 * The definition (csrc/map_window.hip; the predicate: csrc/voxel_device.hpp in_window), all arithmetic in fp32:
 *   A window is a leaf size and, per axis k, an inclusive range lo[k] .. hi[k] of ABSOLUTE cells of the lattice anchored at the origin.
 *   inv_leaf = 1.0f / leaf.  For a record with the coordinates p[0..2], f[k] = floorf(p[k] * inv_leaf) — one multiply, then the floor; no
 *   FMA can form.  The record is KEPT iff p[0], p[1], p[2] are all finite and (float)lo[k] <= f[k] && f[k] <= (float)hi[k] for k = 0, 1, 2.
 *   The comparison is made in float; nothing is converted to an integer (an f beyond the int range, +-inf included, is simply outside).
 *   Requirements: leaf > 0 (NaN refused), lo[k] <= hi[k], |lo[k]| < 2^24 and |hi[k]| < 2^24 (there (float) of a cell is exact); anything
 *   else is LSR_ERR_INVALID_ARGUMENT.  Inside that limit f[k] is, exactly, the absolute cell the voxel grids here assign the point:
 *   VoxelGrid / VoxelGridCovariance compute (int)(floorf(p[k] * inv_leaf) - (float)min_b[k]) with the same inv_leaf, an integer shift of f.
 *   Output: the kept records in ascending input index.  Of each, x, y, z and intensity are copied bit for bit from in_layout's offsets to
 *   out_layout's; an input layout without intensity yields intensity +0, an output layout without intensity has no such field.  Every
 *   other byte of an output record is zero.
 *   Consequence: with leaf = the NDT resolution, the target built from the cut holds in every cell of the window exactly the points, in
 *   the same order, that a target built from the whole map holds there: the leaves have the same bits, and so has every registration
 *   whose lookups stay inside the window (DIRECT7 / DIRECT1 / DIRECT26; not KDTREE, and not GICP, whose neighbours at the border differ).
 * lsr_map_window_around (host only, no handle): lo[k] = (int32)floorf((float)(center[k] - half_extent[k]) * inv_leaf), hi[k] likewise with
 * +; the difference and the sum in double, ONE conversion to float, then the multiply and the floor of the predicate.  Null pointers, a
 * leaf that is not > 0, a centre or half extent that is not finite, a negative half extent: LSR_ERR_INVALID_ARGUMENT; a |lo[k]| or |hi[k]|
 * of 2^24 or more: LSR_ERR_INDEX_OVERFLOW.  No error touches *w. */
typedef struct lsr_map_window { float leaf; int32_t lo[3], hi[3]; } lsr_map_window;   /* inclusive absolute cells */
int lsr_map_window_around(const double center[3], const double half_extent[3], float leaf, lsr_map_window* w);
/* n_points records of in_layout at `data` (host, or HIP device pointer with on_device != 0) -> the kept records, of out_layout, at
 * out_data (host, or HIP device buffer with out_on_device != 0) of capacity_points records; *n_out = how many were kept.  The contract of
 * lsr_voxel_grid_filter_map: out_data == NULL only counts (capacity_points is ignored); capacity_points below the count is
 * LSR_ERR_INVALID_ARGUMENT with *n_out set to the count and out_data untouched; an output range that overlaps the input records is
 * LSR_ERR_INVALID_ARGUMENT; nothing kept (n_points == 0 too) is LSR_OK with *n_out = 0.  Layout, alignment, staging and stream-ordering
 * rules: those of lsr_assemble_map.  At most INT32_MAX records (LSR_ERR_INDEX_OVERFLOW beyond); byte offsets are size_t throughout.
 * Every other error leaves all outputs untouched.  Three launches on the object's stream, and no workgroup waits for another: the kept
 * records counted per workgroup of 256; the counts scanned by one workgroup of 1024 threads; the records written, each ranked among its
 * workgroup's kept ones by the same predicate.  One host wait, for the count, which sizes the output.  Two forms with the same bytes, as
 * in lsr_assemble_map: 16-byte loads and stores when both layouts are {32; 0, 4, 8, 16} and both bases 16-byte aligned, field by field
 * otherwise.  The bytes do not depend on where the buffers live and are identical from call to call.  What the object otherwise
 * answers (target, source, final transformation, fitness) is unchanged.  LSR_MAP_WINDOW_MS reports the launches' time. */
int lsr_crop_map(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout, int on_device,
                 const lsr_map_window* w, void* out_data, size_t capacity_points, const lsr_pc2_layout* out_layout,
                 int out_on_device, size_t* n_out);
/* setInputTarget from a window of the map: lsr_crop_map into a device buffer of pcl::PointXYZI records {32; 0, 4, 8, 16} kept on the
 * object, then lsr_set_input_target_device over that buffer — the same target, bit for bit, as those two calls made by hand.  *n_kept =
 * the records kept.  A window that keeps nothing is LSR_ERR_INVALID_ARGUMENT with *n_kept = 0, and the previous target stays.  One host
 * wait in front of the target build: for the count. */
int lsr_set_input_target_window(lsr_handle h, const void* data, size_t n_points, const lsr_pc2_layout* in_layout,
                                int on_device, const lsr_map_window* w, size_t* n_kept);

/* ---- reading .pcd files (the other half of map.pcd) ------------------------------------------ */
/* PCD v0.7 files, DATA ascii, DATA binary and (with LSR_PCD_READ_COMPRESSED = 1) DATA binary_compressed, decoded on the device into records of an lsr_pc2_layout.  The semantics are RESTATED from
 * knowledge of the format and of the C library, and unpinned, like SURVEY.md 9.10 (the reference has no reader: "map save only").
 * Header (parsed on the host): lines ending in '\n'; `#` lines are comments; entries VERSION, FIELDS (or COLUMNS), SIZE, TYPE, COUNT
 * (default all 1), WIDTH, HEIGHT (default 1), VIEWPOINT (default 0 0 0 1 0 0 0; returned, never applied), POINTS (default WIDTH * HEIGHT)
 * and DATA; any other entry is passed over.  x, y, z are required, each SIZE 4 TYPE F COUNT 1; intensity is optional, of the same type
 * (absent: the output field is +0).  Every other field, `_` included, in any order and with any COUNT, is skipped.
 * ASCII body: lines end at '\n' (the last may lack one); values are separated by runs of blank, '\t' or '\r'; a line without a value is
 * skipped; the first POINTS lines with a value are the points, in order, later lines are ignored; surplus values on a line are ignored.
 * A point line is measured from its first byte that is not a blank: more than LSR_PCD_READ_MAX_LINE_BYTES bytes from there to its '\n' is an
 * error.  A value is the decimal subset of what strtof takes in the C locale — [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?,
 * or [+-]? (inf | infinity | nan) in any letter case; hex floats, nan(...), trailing characters are refused — and becomes the fp32 nearest
 * its exact value, ties to even, overflow to +-inf, gradual underflow through the denormals to +-0, -0 kept: glibc's strtof in the default
 * rounding mode, by integer arithmetic on the device (values the device cannot decide, possible only beyond 19 significant digits, are
 * settled by strtof on the host: LSR_PCD_UNRESOLVED_TOKENS).  nan, +nan = 0x7fc00000, -nan = 0xffc00000.
 * Binary body: POINTS records of (sum of SIZE * COUNT) bytes from the byte behind the DATA line, the four fields copied bit for bit.
 * Compressed body (read only with LSR_PCD_READ_COMPRESSED = 1; restated from knowledge of PCL and liblzf, unpinned): uint32 compressed_size,
 * uint32 uncompressed_size, little endian, then compressed_size bytes of ONE LZF stream; bytes behind it are ignored.  The inflated image
 * has uncompressed_size = POINTS * (sum of SIZE * COUNT) bytes and is field-major: per entry of FIELDS, in header order (`_` and skipped
 * fields included), a block of POINTS * SIZE * COUNT bytes, point i at i * SIZE * COUNT inside it.  The stream is liblzf's: a control
 * byte c < 32 copies the next c + 1 bytes; otherwise len = c >> 5 (len == 7: len += next byte), distance = ((c & 31) << 8 | next byte) + 1,
 * and len + 2 bytes are copied from `distance` bytes back in the output, byte by byte (distance < len + 2 repeats a pattern).  It is
 * inflated on the device (csrc/pcd_lzf.hip); the host reads the two size words and nothing else of the body.  Both sizes are at most
 * 2^31 - 1.  The four fields' bytes are copied bit for bit, as from a binary body.
 * Output: records of out_layout (rules and refusals of lsr_assemble_map's output layout; offset_intensity < 0 drops the intensity), every
 * byte outside the fields zero.
 * Errors: LSR_ERR_INVALID_ARGUMENT — a required entry missing or malformed ("header incomplete" when the bytes end before the DATA
 * line), x, y or z absent, POINTS != WIDTH * HEIGHT, POINTS == 0; an ASCII line with fewer values than the fields demand, a value outside
 * the grammar, a line too long, fewer point lines than POINTS (lsr_last_error() names the file byte offset of the line's first byte; of
 * several bad lines the earliest); a binary body shorter than POINTS records; capacity_points below POINTS.  A compressed body, in this
 * order: shorter than the 8 bytes of its size words; (LSR_ERR_INDEX_OVERFLOW) a size above 2^31 - 1; uncompressed_size != POINTS * record
 * bytes; compressed_size 0; compressed_size above the bytes that follow; capacity_points below POINTS; then, found on the device, a token
 * that passes the end of the stream, a reference to before the first output byte, output past uncompressed_size (lsr_last_error() names
 * the file byte offset of the token's control byte, "byte offset N"; of several bad tokens the earliest) and a stream that ends with
 * fewer than uncompressed_size bytes put out (no offset).  LSR_ERR_NOT_IMPLEMENTED — DATA binary_compressed on an object without
 * LSR_PCD_READ_COMPRESSED = 1 (the default); x, y, z or intensity not a 4-byte float (this one first).  LSR_ERR_INDEX_OVERFLOW — more than
 * INT32_MAX points. */
#define LSR_PCD_READ_MAX_LINE_BYTES 1024
typedef struct lsr_pcd_info {
  uint64_t n_points, width, height, data_offset; /* data_offset: of the body's first byte */
  uint32_t point_step;                           /* bytes of a binary record: the sum of SIZE * COUNT */
  int32_t data_kind /* 0 ascii, 1 binary, 2 binary_compressed */, has_intensity, n_fields;
  double viewpoint[7];
} lsr_pcd_info;
/* The header at the head of a file image (host memory; the image may be cut anywhere behind the DATA line).  Host only, no handle.  With
 * DATA binary_compressed *info is filled (data_kind 2) and the status is LSR_ERR_NOT_IMPLEMENTED; no other error touches *info. */
int lsr_parse_pcd_header(const void* bytes, size_t n_bytes, lsr_pcd_info* info);
/* A whole file image (host pointer, or HIP device pointer with on_device != 0; any alignment) -> its records in out_records (host, or HIP
 * device buffer with out_on_device != 0; 4-byte aligned) of capacity_points records; *n_out = POINTS.  The inverse of
 * lsr_format_pcd_ascii.  out_records == NULL: only *n_out is set (out_layout and capacity_points are ignored).  A body of 2^32 bytes or
 * more is LSR_ERR_INDEX_OVERFLOW: files of any size go through lsr_load_pcd.  No error touches out_records or *n_out.  What the object
 * answers afterwards (target, source, final transformation, fitness) is unchanged. */
int lsr_decode_pcd(lsr_handle h, const void* image, size_t n_bytes, int on_device, void* out_records, size_t capacity_points,
                   const lsr_pc2_layout* out_layout, int out_on_device, size_t* n_out);
/* The same from the file `path`, read in pieces of LSR_PCD_READ_PIECE_BYTES through two pinned buffers kept on the object: an ASCII piece
 * is cut at its last '\n' and what lies behind it is carried into the next; the calling thread reads piece k + 1 while piece k is parsed on
 * the object's stream; reading stops once POINTS lines are in.  A compressed body is copied whole into HBM in such pieces (piece k + 1 read
 * while piece k is copied; reading stops after 8 + compressed_size body bytes) and inflated once.  The records do not depend on the piece size.  LSR_ERR_IO, with errno's
 * text in lsr_last_error(), when the file cannot be opened or read. */
int lsr_load_pcd(lsr_handle h, const char* path, void* out_records, size_t capacity_points, const lsr_pc2_layout* out_layout,
                 int out_on_device, size_t* n_out);
/* setInputTarget from a file: lsr_load_pcd into a device buffer of pcl::PointXYZI records {32; 0, 4, 8, 16} kept on the object, then
 * lsr_set_input_target_device over that buffer — the same target, bit for bit, as those two calls made by hand.  *n_points = POINTS. */
int lsr_set_input_target_pcd(lsr_handle h, const char* path, size_t* n_points);

/* ---- pose-graph optimisation --------------------------------------------- */
/* The optimiser half of doPoseAdjustment (graph_based_slam_component.cpp:267-319): g2o's VertexSE3 / EdgeSE3 graph with identity
 * information, vertex 0 fixed, under g2o's Levenberg-Marquardt controller, restated in fp64 (DESIGN.md 4 "Pose-graph optimisation") and solved on the device. */
#define LSR_POSE_GRAPH_MAX_VERTICES 8192
#define LSR_POSE_GRAPH_MAX_BAND 8
#define LSR_POSE_GRAPH_MAX_OFFBAND_EDGES 64
#define LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES 1024
typedef struct lsr_pose_edge {
  int32_t from, to;             /* EdgeSE3::vertices()[0], [1] */
  double measurement[16];       /* from^-1 * to, column-major 4x4 fp64: the layout of lsr_loop_edge.relative_pose */
} lsr_pose_edge;
typedef struct lsr_pose_graph_params {
  int32_t max_iterations;       /* [10] optimizer.optimize(10) (:318); 1 or more */
  int32_t band;                 /* [5]  edges with |from - to| <= band form the block band of the solve (1 .. LSR_POSE_GRAPH_MAX_BAND);
                                 *      it changes where an edge is summed, not the system that is solved: use num_adjacent */
} lsr_pose_graph_params;
enum {
  LSR_POSE_GRAPH_STOP_MAX_ITERATIONS = 0,  /* all max_iterations ran */
  LSR_POSE_GRAPH_STOP_TRIALS = 1,          /* ten trials of one iteration were rejected */
  LSR_POSE_GRAPH_STOP_RHO_ZERO = 2,        /* the gain ratio was exactly zero */
  LSR_POSE_GRAPH_STOP_LAMBDA = 3           /* lambda left the finite numbers */
};
typedef struct lsr_pose_graph_result {
  int32_t iterations;           /* iterations run */
  int32_t trials;               /* solves in all (accepted and rejected) */
  double chi2_before;           /* sum e^T e at the incoming poses (no factor 1/2) */
  double chi2_after;            /* ... at the returned poses */
  double lambda;                /* the damping after the last iteration */
  int32_t stop_reason;          /* LSR_POSE_GRAPH_STOP_* */
  int32_t reserved;
  double device_ms;             /* hipEvent time from the first upload to the last read-back on the object's stream */
} lsr_pose_graph_result;
typedef struct lsr_pose_graph_trace {
  int32_t trials;               /* solves of this iteration */
  int32_t reserved;
  double chi2, lambda, rho;     /* after the iteration: accepted chi2, damping, the last gain ratio */
} lsr_pose_graph_trace;
/* The odometry edges doPoseAdjustment adds (:289-303), in its order: for every i > num_adjacent (strictly) and j = 0 .. num_adjacent-1
 * the edge (i - num_adjacent + j -> i) measured from the incoming poses (poses16: n column-major fp64 4x4).  Vertices 0 .. num_adjacent
 * get none, as there.  Host only, needs no device.  *n_out = the number of edges; more than `capacity` of them: LSR_ERR_INVALID_ARGUMENT
 * with *n_out set and `out` untouched.  Null poses16 / n_out, n < 1 or num_adjacent < 1: LSR_ERR_INVALID_ARGUMENT. */
int lsr_pose_graph_edges(const double* poses16, int n, int num_adjacent, lsr_pose_edge* out, size_t capacity, size_t* n_out);
/* optimizer.initializeOptimization(); optimizer.optimize(max_iterations) (:317-318) over n vertices (poses16_in, vertex 0 fixed) and
 * n_edges edges — the caller passes the odometry edges (lsr_pose_graph_edges) followed by one edge per accumulated loop edge
 * (from = id_from, to = id_to, measurement = relative_pose; :308-315); a pair may occur twice.  poses16_out: n column-major fp64 4x4,
 * what lsr_assemble_map takes as poses16 (may be poses16_in).  params NULL = the defaults in brackets.  trace (nullable): room for
 * max_iterations entries, one written per iteration run.  The linear solve is exact (band Cholesky + Woodbury over the edges outside
 * the band; an edge into vertex 0 counts as inside); a host loop reads a few scalars per trial.  Results do not depend on `band`
 * beyond rounding and are bit-identical from call to call.
 * LSR_ERR_INVALID_ARGUMENT: null handle, poses, edges (with n_edges > 0), poses16_out or result; n < 1; n > LSR_POSE_GRAPH_MAX_VERTICES;
 * n_edges < 0 or above 2^20; an edge with from == to or an index outside [0, n); max_iterations < 1; band outside
 * 1 .. LSR_POSE_GRAPH_MAX_BAND; more than LSR_POSE_GRAPH_MAX_OFFBAND_EDGES edges outside the band.  LSR_ERR_HIP: a HIP call failed, or
 * the host could not allocate its copy of the graph.  Outputs are untouched on every error.  n == 1 or n_edges == 0: LSR_OK, the input poses, zero iterations.  Writing pose_graph.g2o (:319) stays the caller's. */
int lsr_optimize_pose_graph(lsr_handle h, const double* poses16_in, int n, const lsr_pose_edge* edges, int n_edges,
                            const lsr_pose_graph_params* params /* nullable */, double* poses16_out, lsr_pose_graph_result* result,
                            lsr_pose_graph_trace* trace /* nullable */);
/* The same call for a drive of ordinary length: the reference keeps every accepted loop edge for the life of the node (loop_edges_ only
 * grows, :247; all of them are added, :308-315), so a revisit of two minutes passes LSR_POSE_GRAPH_MAX_OFFBAND_EDGES.  Same nine
 * parameters, same contract — outputs untouched on every error, n == 1 or n_edges == 0 served trivially — with
 * LSR_POSE_GRAPH_LONG_MAX_OFFBAND_EDGES in the place of LSR_POSE_GRAPH_MAX_OFFBAND_EDGES.  With at most LSR_POSE_GRAPH_MAX_OFFBAND_EDGES
 * edges outside the band it runs what lsr_optimize_pose_graph runs and returns the same bits.  Above, the dense part of the Woodbury
 * split (6L x 6L, L the edges outside the band) is a blocked fp64 Cholesky over many workgroups and the rows are combined a wave per
 * row: the same system, another summation order (DESIGN.md 4 "Pose-graph optimisation" has the measured differences), bit-identical
 * from call to call.
 * Workspace, reserved on the object when such a graph arrives and kept: the right-hand sides W, 6(n - 1) x (1 + 6L) doubles — 2.4 GB at
 * 8192 vertices and 1024 edges outside the band, 0.6 GB at 2048 vertices — and the dense matrix C, 36 L^2 doubles, 302 MB at 1024
 * edges.  A reservation that fails is LSR_ERR_HIP with the outputs untouched. */
int lsr_optimize_pose_graph_long(lsr_handle h, const double* poses16_in, int n, const lsr_pose_edge* edges, int n_edges,
                                 const lsr_pose_graph_params* params /* nullable */, double* poses16_out, lsr_pose_graph_result* result,
                                 lsr_pose_graph_trace* trace /* nullable */);

/* ---- inspection (parity tests / profiling; not used by the ROS nodes) ------------------- */
/* NDT voxel grid: info[0..2]=min_b, [3..5]=max_b, [6]=#leaves (any point count), [7]=#leaves usable (n>=6, valid cov) */
int lsr_ndt_grid_info(lsr_handle h, int32_t* info8);
/* Dump all leaves sorted by linear index: idx[L], npts[L] (-1 = invalidated), mean[L*3], icov[L*9] (row-major). */
int lsr_ndt_grid_dump(lsr_handle h, int32_t* idx, int32_t* npts, double* mean, double* icov);
/* The FLOAT centroids of the leaves (pclomp::VoxelGridCovariance::Leaf::centroid: the float running sum of a leaf's points in cloud
 * order over (float) count) — the points of the voxel-centroid kd-tree that the KDTREE neighbourhood searches —, in the order of
 * lsr_ndt_grid_dump: centroid[L*3]; NaN for leaves that are not in the kd-tree (fewer than 6 points).  Leaves whose covariance the
 * eigen check invalidated (npts = -1) are in the kd-tree and have their centroid. */
int lsr_ndt_grid_centroids(lsr_handle h, float* centroid);
/* One derivative pass at pose p = (tx,ty,tz,rx,ry,rz); T16 (nullable, col-major) overrides the point
 * transform like the first pass of align().  grad: 6, hess: 36 (row-major).
 * compute_hessian: 0 the gradient-only pass of a line-search trial (hess comes back zero), 1 the pass with Hessian,
 * 2 the fused pass of a search's tenth trial: score and gradient are the bits of form 0, the Hessian the bits of form 1. */
int lsr_ndt_derivatives(lsr_handle h, const double* p6, const float* T16, int compute_hessian, double* score,
                        double* grad, double* hess);
/* The same; pairs (nullable) receives the number of valid (point, voxel) pairs of the pass. */
int lsr_ndt_derivatives_pairs(lsr_handle h, const double* p6, const float* T16, int compute_hessian, double* score,
                              double* grad, double* hess, double* pairs);

/* ---- NDT pose search: score the source over a lattice of poses, refine the distinct best ------------------------------------
 * For an object that has a target and a source but no guess inside NDT's basin of convergence (a vehicle switched on somewhere in a
 * saved map).  No reference site exists — the reference's answer is a person clicking `initial_pose` in rviz —: the definitions
 * below are this project's (unpinned).
 *
 * lsr_ndt_score_poses: poses16 = count column-major 4x4 float transforms on the host, in the form of lsr_align's guess;
 * 1 <= count <= LSR_POSE_SEARCH_MAX_POSES.  score[c] and pairs[c] (pairs nullable) are exactly the score and pairs that
 * lsr_ndt_derivatives_pairs(h, p, &poses16[16 c], 0, ...) returns for this target, source, resolution, outlier ratio and
 * neighbourhood, bit for bit (the score of a pass with T16 given does not depend on p) — all poses in ONE launch.  DIRECT7, DIRECT1
 * and DIRECT26, in the table mode the object's derivative passes use; KDTREE is LSR_ERR_NOT_IMPLEMENTED.  Without a target or a
 * source the call fails as lsr_ndt_derivatives does.  LSR_ERR_INVALID_ARGUMENT, outputs untouched: null handle, poses16 or score;
 * count == 0 or above the limit; a pose entry that is not finite.  What the object otherwise answers (target, source, final
 * transformation, converged, fitness) is unchanged.  LSR_POSE_SEARCH_MS reports the launch's time. */
#define LSR_POSE_SEARCH_MAX_POSES (1 << 20)
#define LSR_POSE_SEARCH_MAX_KEPT 16
int lsr_ndt_score_poses(lsr_handle h, const float* poses16, size_t count, double* score, double* pairs /* nullable */);

/* A lattice of poses around a centre: n[0] x n[1] x n[2] translations, `step` apart per axis, times n_yaw headings, yaw_step apart,
 * all centred.  Candidate c = ((m n[2] + k) n[1] + j) n[0] + i has the offsets (i - (n[0] - 1) / 2.0) step[0], (j - ...) step[1],
 * (k - ...) step[2] and the heading psi = (m - (n_yaw - 1) / 2.0) yaw_step: R_c = Rz(psi) R_center, t_c = t_center + offsets, in
 * double from the float centre with the C library's cos and sin; each of the 12 entries is rounded to float once, the last row is
 * 0 0 0 1.  Host only, no handle.  *count = the number of poses; poses16 == NULL only counts; capacity (in poses) below the count:
 * LSR_ERR_INVALID_ARGUMENT with *count set.  An n below 1, a product above LSR_POSE_SEARCH_MAX_POSES, a step or a centre entry
 * that is not finite, a null centre, lattice or count: LSR_ERR_INVALID_ARGUMENT. */
typedef struct lsr_pose_lattice { int32_t n[3]; double step[3]; int32_t n_yaw; double yaw_step; } lsr_pose_lattice;
int lsr_pose_lattice_poses(const float* center16, const lsr_pose_lattice* L, float* poses16, size_t capacity, size_t* count);

/* The distinct best of a scored list: the candidates in order of descending score (ties: ascending index; a score that is NaN or not
 * > 0 is never kept) are walked greedily, and one that is close to an already kept one is skipped.  Close: the translation distance
 * (double, sqrt(dx dx + dy dy + dz dz)) is < min_sep_m AND (trace(R_a^T R_b) - 1) / 2 > cos(min_sep_rad).  Stops at top_k kept,
 * 1 <= top_k <= LSR_POSE_SEARCH_MAX_KEPT.  kept[0 .. *n_kept) = their indices, best first.  Host only, sequential on purpose. */
int lsr_select_poses(const double* score, const float* poses16, size_t count, int top_k, double min_sep_m, double min_sep_rad,
                     int32_t* kept, int* n_kept);

/* The whole search: the lattice around center16, its scores, the selection; then every kept candidate is refined by the object's
 * own NDT schedule, all of them as ONE candidate set (worker objects on the object's stream that share its target and hold a copy
 * of its source, as lsr_search_loop(top_k > 1) keeps them) — a refined pose has the bits lsr_align(h, candidate) gives alone.  The
 * winner is the largest refined[e].score (trans_probability), ties to the lower rank; best16 and *result receive the winner's and
 * become the object's final transformation and converged flag, as after lsr_align.  Nothing kept: LSR_OK with n_kept = 0,
 * winner = -1, best16 untouched and result->converged = 0.  report (nullable): kept[e], coarse_score[e], refined16[16 e ..] and
 * refined[e] per kept candidate e, best coarse score first.  Errors of the three entries above; a GICP object and a top_k outside
 * 1 .. 16 are LSR_ERR_INVALID_ARGUMENT. */
typedef struct lsr_pose_search_params { lsr_pose_lattice lattice; int32_t top_k; double min_sep_m, min_sep_rad; } lsr_pose_search_params;
typedef struct lsr_pose_search_report { int32_t n_candidates, n_kept, winner; int32_t kept[16]; double coarse_score[16];
                                        float refined16[16 * 16]; lsr_result refined[16]; } lsr_pose_search_report;
int lsr_ndt_search_pose(lsr_handle h, const float* center16, const lsr_pose_search_params* p, float* best16, lsr_result* result,
                        lsr_pose_search_report* report /* nullable */);

/* The appearance loop gate (described with the Scan Context entries above, behind lsr_search_loop). */
typedef struct lsr_appearance_loop_params {
  lsr_loop_params loop;
  lsr_scan_context_params sc;
  double sc_distance_threshold;
  lsr_pose_search_params search;
} lsr_appearance_loop_params;
int lsr_search_loop_appearance(lsr_handle h, const lsr_submap* submaps, int num_submaps, size_t stride_bytes, int on_device,
                               const float* descriptors, int num_descriptors, int desc_on_device,
                               const lsr_appearance_loop_params* params, lsr_loop_edge* edges, int32_t* shifts, float* sc_dist,
                               int edge_capacity, int* n_evaluated);

/* GICP per-point covariances after setInput*: which = 0 source, 1 target (regularised, as the optimiser uses them);
 * 2 source, 3 target: the k-neighbour sample covariance BEFORE the eigen-regularisation.  cov: n*9 doubles. */
int lsr_gicp_covariances(lsr_handle h, int which, double* cov);
/* GICP, one linearisation as lsr_align(h, guess16) runs it: the first correspondence pass and the first Gauss-Newton accumulation
 * of an outer iteration whose transformation_ is trans16 (col-major; NULL = identity, the first outer iteration), by the launches
 * of lsr_align itself; nothing else of the outer
 * iteration runs, and a later lsr_align returns what it would have returned without the call.  Inspection only (parity tests).
 * use_seeds != 0: the neighbours the previous lsr_align / lsr_gicp_linearize on this source and target left behind are offered as
 * search seeds, as from the second outer iteration on (LSR_ERR_INVALID_ARGUMENT when there are none).
 * Outputs, each nullable: out[n*3] = guess * source; nn_idx[n] neighbour in the target (-1: none within the gate);
 * valid[n]; M6[n*6] = (C2_j + R C1_i R^T)^-1 as 00 01 02 11 12 22 (zero where valid = 0); q[n*3] the paired target point;
 * x6 / T12 (row-major 3x4, fp32) / dR27 (dR/dphi, dR/dtheta, dR/dpsi, row-major) of the state the accumulation ran at;
 * m = the pair count the chain adopted; sums28 = the reduced sums before the division by m: [0] sum r^T M r, [1..6] J^T M r,
 * [7..27] the upper triangle of J^T M J row by row.  m < 4 returns LSR_OK and m; sums28 then carries no meaning.
 * LSR_ERR_TOO_FEW_POINTS as lsr_align. */
int lsr_gicp_linearize(lsr_handle h, const float* guess16, const float* trans16, int use_seeds, float* out, int32_t* nn_idx,
                       int32_t* valid, double* M6, float* q, double* x6, float* T12, double* dR27, int32_t* m, double* sums28);
/* GICP, ONE outer iteration under the BFGS inner optimiser as lsr_align(h, guess16) runs it with LSR_GICP_SOLVER = LSR_GICP_BFGS
 * (whatever the key says): one correspondence pass at transformation_ = trans16 (col-major; NULL = identity), then that outer
 * iteration's whole inner loop, by the launches of lsr_align itself; a later lsr_align returns what it would have returned without
 * the call.  Inspection only (parity tests).  Outputs, each nullable.  Per cost/gradient evaluation e, in order, for the first
 * `capacity` of them: x6[6 e ..] the point, f[e] the mean cost, g6[6 e ..] the gradient, inner[e] the inner iteration it belonged to
 * (0 = the evaluation at the start x, k = the line search of the k-th step).  n_evals = evaluations in all (may exceed capacity);
 * n_inner = steps taken; reason = why the inner loop ended: 1 no progress, 2 gradient tolerance (|g| < 1e-2), 3 max_inner_iterations
 * reached, 0 left still running (max_inner_iterations < 1: the reference's solver throws), 4 a non-finite cost or gradient;
 * x6_final = where it ended; m = the pair count (m < 4 returns LSR_OK, m and n_evals = 0).  LSR_ERR_TOO_FEW_POINTS as lsr_align. */
int lsr_gicp_bfgs_trace(lsr_handle h, const float* guess16, const float* trans16, int32_t capacity, double* x6, double* f, double* g6,
                        int32_t* inner, int32_t* n_evals, int32_t* n_inner, int32_t* reason, double* x6_final, int32_t* m);
/* 1-NN of the source transformed by T16 (nullable = identity) in the target: idx[n], d2[n]. */
int lsr_nearest_neighbors(lsr_handle h, const float* T16, int32_t* idx, float* d2);
int lsr_get_profile(lsr_handle h, lsr_profile* out, int reset);
/* Host-only self check (needs no device): the angular coefficient tables of NDT eq. 6.19 / 6.21 at pose p6 by the scalar
 * formulas (jang_ref[24], hang_ref[48]) and by the 72-entry table the device evaluates one entry per lane (jang_tab, hang_tab). */
int lsr_debug_angle_tables(const double* p6, int d1_sign, float* jang_ref, float* hang_ref, float* jang_tab, float* hang_tab);
/* Host-only view of the guess decomposition (needs no device): p6 = the pose vector (x, y, z, roll, pitch, yaw) with which
 * lsr_align starts from guess16 (column-major 4x4, nullable = identity) — the fp32 Euler angles of Eigen's eulerAngles(0,1,2),
 * alias branch included (a rotation whose roll comes out positive is returned as (roll - pi, pi - pitch, yaw -+ pi), negated). */
int lsr_debug_guess_pose(const float* guess16, double* p6);
/* The three entries below inspect the on-device NDT controller (Newton step, More-Thuente line search, 6x6 solve) apart from the
 * derivative pass: each launches one workgroup of one wave that calls the device functions of the derivative kernels as they are.
 * Any registration object serves as h (its device and stream are used; no target or source is needed).  A null pointer or a count
 * outside its range is LSR_ERR_INVALID_ARGUMENT before any device is touched.
 *
 * The controller on prepared sums.  The state starts as lsr_align leaves it before its first launch, with the pose p6 given
 * directly.  rows: n_rows x 29 doubles, each the reduced sums of one derivative pass as the kernels lay them out (score, gradient[6],
 * pair count, the upper triangle of the Hessian row by row [21]).  Row after row, until the controller has finished, the sums are
 * handed to the controller step and one trace row of LSR_NDT_REPLAY_TRACE doubles is written: phase, want_hessian, the request
 * flags, done, converged, nr_iterations, n_evals, n_passes, step_iterations, open_interval, interval_converged, a_t, a_l, f_l, g_l,
 * a_u, f_u, g_u, phi_0, d_phi_0, p[6], x_t[6], dir[6], score, g[6], trans_probability, last_pairs.  *n_used = rows consumed;
 * trace rows beyond it are zero.  1 <= n_rows <= LSR_NDT_REPLAY_MAX_ROWS, n_points >= 1. */
#define LSR_NDT_REPLAY_MAX_ROWS 512
#define LSR_NDT_REPLAY_TRACE 47
#define LSR_DEBUG_MAX_COUNT (1 << 20)
int lsr_debug_ndt_controller_replay(lsr_handle h, const double* p6, double step_size, double trans_eps, int max_iterations,
                                    int n_points, const double* rows, int n_rows, double* trace, int* n_used);
/* delta6[6 i ..] = the Newton step -H^-1 g of system i (Hu21[21 i ..] the upper triangle row by row, g6[6 i ..]) by the controller's
 * one-wave elimination, the systems one after another.  1 <= count <= LSR_DEBUG_MAX_COUNT. */
int lsr_debug_ndt_solve6(lsr_handle h, const double* Hu21, const double* g6, int count, double* delta6);
/* quot[i] = a[i] / b[i] and root[i] = sqrt(a[i]) by the line search's fast fp64 division and square root.
 * 1 <= count <= LSR_DEBUG_MAX_COUNT. */
int lsr_debug_mt_math(lsr_handle h, const double* a, const double* b, int count, double* quot, double* root);
/* The four entries below inspect the primitives every voxel path stands on (csrc/lsd_sort.hip): the stable LSD radix sort of
 * (uint32 key, int32 value) pairs, the exclusive int32 scan, and the runs of equal keys of a sorted sequence (run table, float
 * centroid of every run, run count).  Each is ONE call of the primitive as the library's own paths call it, on host arrays.
 * Any registration object serves as h: its device and stream are used and nothing else of it.  Every device buffer, the sort's and the
 * scan's table and the runs' scratch with its host mailbox are the entry's OWN and are released before it returns, so a build pending on
 * the object is not disturbed and a later lsr_align returns what it would have returned without the call.  The stream is synchronised
 * before the entry returns.  A null pointer, a size outside 1 .. LSR_DEBUG_SORT_MAX or any other argument outside its range is
 * LSR_ERR_INVALID_ARGUMENT before the handle is looked at and before anything is allocated or written; then a null handle is.
 *
 * What the primitives will launch for n elements, on the host (needs no device).  out[LSR_DEBUG_LSD_PLAN_WORDS]: for the sort of n pairs on
 * end_bit bits {passes, bits per pass, 64-key steps per wave (8 or 16: workgroups of 2048 or 4096 keys), workgroups, 1 if every
 * workgroup prefixes the histogram rows itself (the fused scatter) else 0, covered_bits = passes * bits}; for the scan of n ints
 * {4096-element blocks, 1 if one launch serves (one block) else 0, block sums per thread of the middle launch}; for the runs of n
 * keys {256-key blocks, block counts per thread of the scanning launch}.  1 <= end_bit <= 32. */
#define LSR_DEBUG_SORT_MAX (1 << 24)
#define LSR_DEBUG_LSD_PLAN_WORDS 11
#define LSR_DEBUG_CANARY_F32_BITS 0x7FC0DEADu
int lsr_debug_lsd_plan(size_t n, int end_bit, int* out);
/* One sort.  The pairs come back ordered by the low covered_bits (>= end_bit) bits of the key, equal ones in input order; the bits
 * above are carried unchanged (the library's callers keep their keys below 2^end_bit).  vals == NULL: the values are 0 .. n - 1.
 * alias_vals != 0 (needs vals): the sort is handed ONE buffer as its first value side and as that side's spare, as the map filter
 * does.  *result_in_b: 1 if the sort left its result on its second side (an odd number of passes), else 0; keys_out / vals_out are
 * copied from the side it names.  The table is filled with 0xFF bytes before the call, as a larger sort before it might have left it. */
int lsr_debug_sort_pairs_u32(lsr_handle h, const uint32_t* keys, const int32_t* vals, size_t n, int end_bit, int alias_vals,
                             uint32_t* keys_out, int32_t* vals_out, int* result_in_b);
/* One exclusive scan: out[i] = in[0] + .. + in[i - 1] in int32.  On the device `in` starts in_shift ints and `out` out_shift ints
 * (each 0 .. 3) past a 16-byte boundary. */
int lsr_debug_exclusive_scan_i32(lsr_handle h, const int32_t* in, size_t n, int in_shift, int out_shift, int32_t* out);
/* The runs of equal keys of keys_sorted[n]: heads counted and scanned (with the count left in device memory too), the run table, the
 * centroid of every run, then the count read from the host mailbox.  order[n] (each 0 .. n - 1) names the point of every sorted
 * position in the planes x, y, z, w (w nullable; cw is null exactly when w is).  The run of key `sentinel` gets no centroid;
 * sentinel_on_device != 0: the kernel reads the sentinel from device memory and is handed ~sentinel by value.
 * run_key / run_off: n + 1 entries, run r covers the sorted positions [run_off[r], run_off[r + 1]); cx, cy, cz, cw: n entries, one
 * per run in key order.  Before the launches the device outputs are filled with a canary, 0xFFFFFFFF words in the tables and floats
 * of the bits LSR_DEBUG_CANARY_F32_BITS (a NaN) in the centroids: what comes back as canary was not written.
 * *n_runs: the count from the mailbox; *n_runs_dev: the count left in device memory. */
int lsr_debug_sorted_runs(lsr_handle h, const uint32_t* keys_sorted, const int32_t* order, size_t n, const float* x, const float* y,
                          const float* z, const float* w, uint32_t sentinel, int sentinel_on_device, uint32_t* run_key, int32_t* run_off,
                          float* cx, float* cy, float* cz, float* cw, int* n_runs, int* n_runs_dev);

#ifdef __cplusplus
}
#endif
#endif /* LIDARSLAM_REG_H */

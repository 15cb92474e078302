/*
 * slamfusion.h — C ABI of libslamfusion.so: MI355X-native (gfx950, hand-written HIP)
 * scan-to-map registration hot path, drop-in for that path of
 * viniciusvidal2/slam-sensor-fusion.  Plain C types only; no torch, PCL or Eigen types.
 *
 * The reference has no FFI/plugin interface: the seam is the C++ class
 * ICPPointToPoint (localization/include/localization/icp_point_to_point.h:41-136), the
 * free functions of localization/include/localization/point_cloud_processing.hpp:31-92,
 * the PCL VoxelGrid call (localization/src/global_map_frames_manager.cpp:142-146) and,
 * in the Python twin, three Open3D calls (localization_python/localization_python/
 * localization_node.py:47,222-225,233-237).  Each entry point below cites what it
 * replaces.  INTEGRATION.md shows the reference-side bindings.
 *
 * Conventions
 *   - 4x4 matrices: ROW-MAJOR arrays of 16 (Eigen::Matrix4f in the reference is
 *     column-major: pass M.transpose().data() or use include/localization adapters).
 *   - Point clouds: AoS xyz float32 triplets (pcl::PointXYZ minus its padding).
 *   - Every call returns sf_status (0 = ok, < 0 = infrastructure error; text from
 *     sf_last_error()).  Algorithmic "no lock" is NOT an error: it is reported exactly
 *     like the reference, in sf_icp_result (initial transform, error 1e6, iterations 0,
 *     converged 0 — icp_point_to_point.cpp:196-200, icp_point_to_point.h:28-39).
 *   - Not thread-safe: one sf_ctx per host thread (the reference is single-threaded,
 *     localization/src/main.cpp:18).  One HIP stream per context; calls that return
 *     data to the host synchronise that stream, all others only enqueue.
 *   - There is NO CPU fallback: without a HIP device sf_ctx_create fails.
 */
#ifndef SLAMFUSION_H
#define SLAMFUSION_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_VERSION 210

typedef enum {
    SF_OK = 0,
    SF_ERR_INVALID = -1,  /* bad argument                                    */
    SF_ERR_HIP = -2,      /* HIP runtime failure (message has the hipError)   */
    SF_ERR_NOMEM = -3,
    SF_ERR_STATE = -4,    /* call order (e.g. align before set_source)        */
    SF_ERR_OVERFLOW = -5, /* index space too large for the requested grid     */
    SF_ERR_COMM = -6      /* multi-GPU: a collective timed out or was aborted by a peer; every rank of the communicator gets it */
} sf_status;

typedef struct sf_ctx sf_ctx;
typedef struct sf_cloud sf_cloud;
typedef struct sf_map sf_map;
typedef struct sf_icp sf_icp;

int sf_version(void);
const char *sf_last_error(void);

/* ------------------------------------------------------------------ context */
/* One context = one device + one stream.  stream == NULL creates a private stream;
 * otherwise the caller's hipStream_t is used (e.g. a torch ExternalStream) and not owned. */
int sf_ctx_create(int device_id, void *hip_stream, sf_ctx **out);
void sf_ctx_destroy(sf_ctx *ctx);
void *sf_ctx_stream(sf_ctx *ctx);
int sf_ctx_synchronize(sf_ctx *ctx);
int sf_ctx_device_name(sf_ctx *ctx, char *buf, int cap);

/* ------------------------------------------------------------------ clouds (device point sets) */
/* a7: setSourcePointCloud / convertPclToEigen upload — icp_point_to_point.cpp:44-47,86-97 */
int sf_cloud_create(sf_ctx *ctx, sf_cloud **out);
void sf_cloud_destroy(sf_cloud *c);
int sf_cloud_upload(sf_cloud *c, const float *xyz, int64_t n);
int sf_cloud_upload_f64(sf_cloud *c, const double *xyz, int64_t n); /* rounds to f32 */
/* enqueue only (no host synchronisation): with PINNED host memory the copy is asynchronous and stream-ordered -- e.g. on a
 * copy stream's context into a staging cloud that a compute stream picks up with sf_icp_set_source_batch_device */
int sf_cloud_upload_async(sf_cloud *c, const float *xyz, int64_t n);
void *sf_cloud_device_ptr(sf_cloud *c); /* float[n][3] on the device (valid until the cloud is modified) */
int sf_cloud_from_device(sf_cloud *c, const void *d_xyz, int64_t n); /* device-to-device copy */
int sf_cloud_size(sf_cloud *c, int64_t *n);
int sf_cloud_download(sf_cloud *c, float *xyz, int64_t cap, int64_t *n);
int sf_cloud_copy(sf_cloud *dst, sf_cloud *src);
/* a1: applyUniformSubsample — point_cloud_processing.hpp:55-74 (no-op when n < step) */
int sf_cloud_subsample(sf_cloud *c, int step);
/* a2: cropPointCloudThroughRadius — point_cloud_processing.hpp:31-53.  center = T[:3,3];
 * keeps d2 < (float)(radius*radius).  sorted != 0 reproduces PCL's ascending
 * (distance, index) output order; sorted == 0 keeps index order (faster). */
int sf_cloud_crop_radius(sf_cloud *c, const float center[3], double radius, int sorted);
/* a3: removeFloor — point_cloud_processing.hpp:76-92 (keep z > 0) */
int sf_cloud_remove_floor(sf_cloud *c);
/* a19: readFilterPtcRegionPoints — localization_node.py:105-115 (inclusive AABB, NaN skipped) */
int sf_cloud_crop_aabb(sf_cloud *c, const double lo[3], const double hi[3]);
/* a20: OrientedBoundingBox crop — localization_node.py:222-225; R row-major 3x3 */
int sf_cloud_crop_obb(sf_cloud *c, const double center[3], const double R[9], const double extent[3]);
/* a8: applyTransformation — icp_point_to_point.cpp:99-110 (general affine 3x4, float32,
 * unfused multiply/add so results are bit-identical to the reference's x86-64 build) */
int sf_cloud_transform(sf_cloud *c, const float T[16]);
/* `*map_cloud += *cloud` — global_map_frames_manager.cpp:131: dst <- [dst; src] on the device (src unchanged).
 * Map growth = transform the registered scan into the map frame, append, voxel-downsample, sf_map_build. */
int sf_cloud_append(sf_cloud *dst, const sf_cloud *src);
/* indices (into the cloud before the call) kept by the LAST crop/subsample on this cloud */
int sf_cloud_last_indices(sf_cloud *c, int32_t *idx, int64_t cap, int64_t *n);

/* f-2: PointCloud2 -> xyz on the device (pcl::fromROSMsg, localization_node.cpp:290-291;
 * pc2.read_points, localization_node.py:106-111): raw little-endian message buffer,
 * n_points = width*height, float32 fields at byte offsets off_x/y/z inside point_step */
int sf_cloud_from_pointcloud2(sf_cloud *c, const void *data, int64_t n_points, int point_step, int off_x, int off_y, int off_z);
/* the whole sensor_msgs/PointCloud2 contract, checked: data_bytes must cover height rows of row_step bytes
 * (row_step = 0: width * point_step), x/y/z datatype 7 (FLOAT32) or 8 (FLOAT64, rounded to float32 like
 * pcl::fromROSMsg's field mapping), big-endian payloads are refused (SF_ERR_INVALID).  No allocation and no host
 * synchronisation per call once the staging buffer has grown to the message size. */
#define SF_PC2_FLOAT32 7
#define SF_PC2_FLOAT64 8
int sf_cloud_from_pointcloud2_msg(sf_cloud *c, const void *data, int64_t data_bytes, int64_t width, int64_t height, int point_step, int64_t row_step,
                                  int off_x, int off_y, int off_z, int datatype, int is_bigendian);
/* f-3: PCD v0.7 files (ascii / binary / binary_compressed read; "DATA binary" write exactly
 * as pcl::io::savePCDFileBinary does for PointXYZ — mapping/src/map_data_save_node.cpp:74) */
int sf_cloud_load_pcd(sf_cloud *c, const char *path);
int sf_cloud_save_pcd(sf_cloud *c, const char *path);
int sf_pcd_read(const char *path, float **xyz, int64_t *n); /* caller frees with sf_free */
int sf_pcd_write_binary(const char *path, const float *xyz, int64_t n);
void sf_free(void *p);

/* a4 / a5: voxel grids.  flavour SF_VOXEL_PCL = pcl::VoxelGrid float32
 * (global_map_frames_manager.cpp:142-146): int32 linear index, ascending-index output,
 * on int32 overflow the cloud is left unchanged and *status_flags gets
 * SF_FLAG_VOXEL_OVERFLOW (PCL warns and returns its input).  SF_VOXEL_O3D = Open3D
 * voxel_down_sample float64 (localization_node.py:47): origin min_bound - v/2, output
 * ordered by (i,j,k). */
#define SF_VOXEL_PCL 0
#define SF_VOXEL_O3D 1
/* EXTENSION (no reference counterpart): pcl::VoxelGrid's arithmetic with the linear index kept in 64 bits, for maps
 * past 2^31 voxels (BASELINE config 5: a 50 M-point city at leaf 0.1 m) where PCL -- and SF_VOXEL_PCL -- return the
 * cloud unfiltered.  Wherever SF_VOXEL_PCL does not overflow the two give identical ids, order and centroids. */
#define SF_VOXEL_PCL64 2
#define SF_FLAG_VOXEL_OVERFLOW 1
int sf_cloud_voxel_downsample(sf_cloud *c, double leaf, int flavour, int *status_flags);
/* Incremental map growth: exactly sf_cloud_append(map, pending) + sf_cloud_voxel_downsample(map, leaf, SF_VOXEL_PCL, ...)
 * (`*map_cloud += *cloud` + the voxel filter, global_map_frames_manager.cpp:131,142-146) -- bit for bit -- computed as a MERGE
 * when `map` is itself voxel-filtered at that leaf: only the pending points are sorted, their voxels found among the map's by
 * binary search, touched centroids re-summed in point order, one copy pass opens the gaps for the new voxels.  Falls back to
 * the two calls whenever the preconditions do not hold (map keys not strictly ascending under the union's geometry, index
 * overflow, an empty side); *merged (may be NULL) says which way it went.  Both clouds on the same context. */
int sf_cloud_voxel_merge(sf_cloud *map, sf_cloud *pending, double leaf, int *status_flags, int *merged);
/* maps smaller than this take the full path inside sf_cloud_voxel_merge (default 4 000 000 points: below, the full filter is as fast);
 * returns the previous value, n < 0 only reads it */
int sf_cloud_voxel_merge_min_points(int64_t n);
/* introspection for parity tests: per-input-point voxel ids of the LAST downsample
 * (PCL: int32 linear index, -1 for non-finite; O3D: int32 i,j,k triplets) and the ids /
 * float64 means of the output voxels (O3D flavour keeps float64 means). */
int sf_cloud_voxel_point_ids(sf_cloud *c, int32_t *ids, int64_t cap_values, int64_t *n_values);
int sf_cloud_voxel_out_ids(sf_cloud *c, int32_t *ids, int64_t cap_values, int64_t *n_values);
int sf_cloud_voxel_out_means_f64(sf_cloud *c, double *xyz, int64_t cap_points, int64_t *n_points);
int sf_cloud_voxel_point_ids64(sf_cloud *c, int64_t *ids, int64_t cap_values, int64_t *n_values); /* after SF_VOXEL_PCL64 */
int sf_cloud_voxel_out_ids64(sf_cloud *c, int64_t *ids, int64_t cap_values, int64_t *n_values);

/* ------------------------------------------------------------------ map (NN index) */
/* a6: setTargetPointCloud — icp_point_to_point.cpp:49-55.  Instead of a FLANN kd-tree
 * over a 10 m crop rebuilt every 3 m, the WHOLE map gets one device-resident uniform-grid
 * index (cell size `cell`, 0 = automatic); the reference's crop becomes a window.
 * An axis holds at most 2^24 = 16 777 216 cells (float32 counts no further): an explicit `cell` that needs more on any axis, or a
 * table that does not fit, is SF_ERR_OVERFLOW and the map stays unbuilt; an automatic cell grows until both hold. */
int sf_map_create(sf_ctx *ctx, sf_map **out);
void sf_map_destroy(sf_map *m);
int sf_map_build(sf_map *m, sf_cloud *cloud, float cell);
int sf_map_size(sf_map *m, int64_t *n);
int sf_map_cell_size(sf_map *m, float *cell, int32_t dims[3]);
/* The index carried over a growth step (`*map_cloud += *cloud` + voxel filter + setTargetPointCloud:
 * global_map_frames_manager.cpp:131,142-146, icp_point_to_point.cpp:49-55): exactly sf_map_build(m, cloud, <the cell m has>)
 * -- points in cell order with their ids, and the cell table, bit for bit -- computed as a MERGE of the old index with the centroids the last
 * sf_cloud_voxel_merge(cloud, ...) wrote, when `m` indexes `cloud` as it was before that merge and nothing has touched
 * the cloud since: the entries that stay keep their order (one streaming pass), only the new centroids are sorted.
 * Takes the build itself whenever that does not hold (the merge took its full path, the cloud changed in between, the
 * smallest coordinate of the map moved, 64-bit cell ids); *patched (may be NULL) says which way it went: 1 = merged,
 * SF_PATCH_* (<= 0) = built, and why.  Normals and the window are dropped as sf_map_build drops them (the normals stay with
 * sf_map_set_normals_carry, below); re-attach the map to its sf_icp (sf_icp_set_target). */
#define SF_PATCH_NO_MERGE        0   /* no usable record: the merge took its full path, the cloud changed since, another cloud's index */
#define SF_PATCH_BOUND_REPLACED (-1) /* (not returned any more: a replaced bound costs one reduction over the cloud, then the patch goes on) */
#define SF_PATCH_ORIGIN_MOVED   (-2) /* a new centroid lies below the grid origin: every cell changes */
#define SF_PATCH_LIMITS         (-3) /* 2^28 points / 2^32 cells / table memory */
#define SF_PATCH_CLAMPED_POINT  (-4) /* a point the old grid had clamped to its upper face now lies in a cell of its own, whether it stays or the merge replaced it */
int sf_map_patch(sf_map *m, sf_cloud *cloud, int *patched);
/* For a map that is going to grow (sf_map_patch): the grid starts at the multiple of `cells` cells (0 = off, the default: at the
 * smallest coordinates themselves) below the smallest coordinates, so growth by a few metres in any direction -- below the
 * origin too -- leaves every point's cell coordinates, and a patch possible; the table gets at most `cells` empty cells per
 * axis in front of the data.  Takes effect with the next sf_map_build.  Maps that register large BATCHES are better left
 * without: the scans' ordering keys span the empty margin as well (measured: -4 % at the metric configuration with 64). */
int sf_map_set_origin_lattice(sf_map *m, int cells);
/* the index as it lies in HBM, for parity tests: points indexed, cells, grid origin, 1 / cell, the pruning slack;
 * pts4 = float[n][4] (x, y, z, bitcast point id) in cell order, cell_start = uint32[n_cells + 1] (either may be NULL) */
int sf_map_index_info(sf_map *m, int64_t *n_indexed, int64_t *n_cells, float org[3], float *inv_h, float *gap_eps);
int sf_map_download_index(sf_map *m, float *pts4, int64_t cap_points, uint32_t *cell_start, int64_t cap_cells);
/* window = the reference's map crop, applied as a predicate inside the search:
 * sphere: d2(center,p) < (float)(radius*radius) like cropPointCloudThroughRadius
 * (localization_node.cpp:302); obb: like localization_node.py:222-225; none: whole map */
int sf_map_window_none(sf_map *m);
int sf_map_window_sphere(sf_map *m, const float center[3], double radius);
int sf_map_window_obb(sf_map *m, const double center[3], const double R[9], const double extent[3]);
/* number of indexed map points inside the current window (the reference skips the scan when
 * its cropped map is empty, localization_node.py:226-228) */
int sf_map_window_count(sf_map *m, int64_t *n);
/* extension x2 (no reference code): PCA normals from neighbours within `radius` */
int sf_map_estimate_normals(sf_map *m, float radius);
/* the same pass also keeps each point's 3x3 neighbourhood covariance (6 unique float64 entries xx xy xz yy yz zz,
 * centred on the neighbourhood mean, divided by the neighbour count; zeros below 3 neighbours) -- SURVEY x2
 * "normals + covariance", BASELINE config 5 */
int sf_map_estimate_normals_cov(sf_map *m, float radius, int with_covariance);
int sf_map_download_covariances(sf_map *m, double *cov6, int64_t cap_points, int64_t *n); /* original point order */
int sf_map_set_normals(sf_map *m, const float *normals, int64_t n); /* original point order */
/* Normals (and covariances) carried over sf_map_patch.  Off (0, the default): sf_map_patch drops them as described there.  On: the
 * map remembers the `radius` and `with_covariance` of its last sf_map_estimate_normals[_cov] (sf_map_set_normals and
 * sf_map_build forget them), and after sf_map_patch it has normals -- and covariances, if it had them -- that equal
 * sf_map_patch followed by sf_map_estimate_normals_cov(m, radius, with_covariance) bit for bit, on every path:
 *  - where the index was merged (*patched = 1), the entries that stay take their normal, neighbour count and covariance along
 *    in the patch's own pass, and only the new centroids and the points within `radius` of a position the merge added or
 *    removed are estimated again, by the arithmetic of the full pass on the patched index (an untouched neighbourhood is
 *    visited in the same order, so its float64 sums come out the same);
 *  - where the build ran (SF_PATCH_* <= 0), the full estimate runs after it with the remembered arguments.
 * Normals given through sf_map_set_normals are NOT carried (there is nothing to re-estimate the changed part with): the patch
 * drops them, switch on or off.  The window is dropped either way, and the map is re-attached with sf_icp_set_target as before.
 * The re-estimate is enqueued on the context's stream behind the patch; every call that reads the normals is ordered after it. */
int sf_map_set_normals_carry(sf_map *m, int on);
/* what the last sf_map_patch did with the normals:
 * out[0]: 1 = carried over the patch, 0 = re-estimated in full (the patch took the build),
 *         -1 = dropped (switch off, or nothing to carry: no normals, or normals from sf_map_set_normals)
 * out[1]: changed positions (centroids added + old points removed; 0 unless carried)
 * out[2]: points re-estimated (0 when dropped, all indexed points after a build)
 * out[3]: map points */
int sf_map_normals_carry_info(sf_map *m, int64_t out[4]);
int sf_map_download_normals(sf_map *m, float *normals, int32_t *n_neighbors, int64_t cap, int64_t *n);
/* raw exact 1-NN (a9 without the threshold): idx in ORIGINAL point order, d2 squared
 * float32 summed x,y,z like FLANN L2_Simple; idx = -1 if nothing within max_d2. */
int sf_map_nn(sf_map *m, const float *queries, int64_t n, float max_d2, int32_t *idx, float *d2);
#define SF_KNN_MAX 64
/* exact k nearest neighbours of each query among the indexed points the window accepts (as sf_map_nn).
 * Row i of idx / d2 (k entries each): the min(k, m_i) smallest candidates in ascending order of
 * (d2, position in the index), d2 = FLANN L2_Simple in float32 like sf_map_nn, accepted iff d2 < max_d2 (strict);
 * idx in ORIGINAL point order; the unused tail of a row is idx = -1, d2 = +inf.  count[i] = min(k, m_i) (may be NULL).
 * A non-finite query, an empty map, or max_d2 <= 0 or NaN gives count 0 (no search).  SF_ERR_INVALID for k < 1 or k > SF_KNN_MAX. */
int sf_map_knn(sf_map *m, const float *queries, int64_t n, int k, float max_d2, int32_t *idx, float *d2, int32_t *count);
/* extension x2, the k-NN / hybrid form (Open3D KDTreeSearchParamKNN / Hybrid): PCA normal (and covariance) of every map point
 * from its k nearest map points, itself included, within max_radius (<= 0 or inf: no limit).  See DESIGN §13 for the exact rule.
 * The map remembers (k, max_radius, with_covariance) in place of the radius: with sf_map_set_normals_carry on, sf_map_patch is
 * followed by this estimate in full on every path (sf_map_normals_carry_info: {0, 0, n, n}). */
int sf_map_estimate_normals_knn(sf_map *m, int k, float max_radius, int with_covariance);
/* Radius search with variable-length rows (extension, no reference code): pcl radiusSearch, Open3D
 * search_radius_vector_3d (search_hybrid_vector_3d is sf_map_knn(q, max_nn, r2)).  r2 = (float)(radius * radius); row i holds every
 * indexed point p the window accepts with d2(q_i, p) < r2 under the float32, unfused, strict rule of sf_map_nn / sf_map_knn /
 * sf_map_radius_outliers; idx in ORIGINAL point order, d2 the float32 value that was compared.  So min(count_i, 64) and the first 64
 * entries of a distance-ordered row are exactly sf_map_knn(q_i, 64, r2).  A non-finite query or an empty map gives an empty row
 * (no walk).  The rows are CSR: offsets[n + 1] (host, may be NULL), offsets[i + 1] - offsets[i] the count of row i; the entries
 * stay on the device, owned by the map, until the next radius call, sf_map_build or sf_map_patch, and sf_map_radius_results
 * downloads them.
 * search: arbitrary queries (host pointer, as sf_map_knn), the window honoured.  graph: the queries are the map's own points, row i
 *   belongs to ORIGINAL point i, the window is ignored (as the outlier and clustering calls ignore it); a point that is not indexed
 *   has an empty row and appears in no row; a point's own entry (d2 = 0) is in its row, so the counts are sf_map_radius_outliers'.
 * results: the rows, concatenated; either pointer may be NULL; *total is always set (0 with no lists); cap < total with a pointer
 *   given is SF_ERR_INVALID and writes nothing; SF_ERR_STATE when there are no lists (no call so far, or a build or patch since).
 * SF_ERR_INVALID: a radius that is not positive and finite or whose r2 is not; an order that is not one of the two; n < 0.
 * SF_ERR_STATE: a map that is not built.  n == 0 is SF_OK with offsets[0] = 0.  SF_ERR_OVERFLOW: more than 2^32 - 2 entries in all
 * (the offsets on the device are 32-bit, the sort takes no more) -- decided from a 64-bit sum of the counts before anything is
 * reserved or filled; SF_ERR_NOMEM: an allocation failed.  Both leave the map without lists and otherwise usable.
 * stats: the rows, those searched (finite queries / indexed points of a map that is not empty), the rows of count 0, the entries,
 * the longest row.  fill: both forms give the same bytes; automatic is the one measured faster. */
#define SF_RADIUS_ORDER_INDEX    0   /* rows ascend in position in the index (the order of the walk) */
#define SF_RADIUS_ORDER_DISTANCE 1   /* rows ascend in (bits of d2, position in the index): the order of sf_map_knn */
typedef struct { int64_t n_queries, n_searched, n_empty, total, max_count; } sf_radius_stats;
int sf_map_radius_search(sf_map *m, const float *queries, int64_t n, double radius, int order, int64_t *offsets, sf_radius_stats *stats);
int sf_map_radius_graph(sf_map *m, double radius, int order, int64_t *offsets, sf_radius_stats *stats);
int sf_map_radius_results(sf_map *m, int32_t *idx, float *d2, int64_t cap, int64_t *total);
int sf_map_set_radius_fill(sf_map *m, int mode);          /* 0 = automatic (default), 1 = one lane per row, 2 = one wave per row */
int sf_map_radius_launch_ms(sf_map *m, float ms[3]);      /* count+scan, fill, sort of the last call; zeros unless sf_map_profile_launches is on */
/* Outlier removal (extension, no reference code): pcl::StatisticalOutlierRemoval / pcl::RadiusOutlierRemoval,
 * Open3D remove_statistical_outlier / remove_radius_outlier.  The window is ignored, as the normals passes ignore it; the map's
 * index, normals and neighbour table are not modified.
 * Statistical.  The list of point i is its sf_map_knn list (own float32 coordinates, max_d2 = +inf, no window) of K entries:
 *   SF_SOR_PCL: k OTHER points, K = k + 1, k in 1 .. 63;  SF_SOR_O3D: k points, itself among them, K = k, k in 1 .. 64;
 *   any other flavour or k is SF_ERR_INVALID.  cnt = min(K, n_valid).
 *   d_i = (sum over the list positions of sqrt((double)d2), pairwise tree over positions 0 .. 63, absent ones +0.0) divided by
 *   cnt - 1 (PCL: position 0 is the point itself or a coincident one; 0 when cnt < 2) or by cnt (O3D); NaN for a point that is
 *   not indexed (non-finite).  mean = sum(d) / n_valid, stddev = sqrt(sum((d - mean)^2) / (n_valid - 1)) (0 when n_valid < 2),
 *   both float64 sums over the points in ORIGINAL order in the pairwise tree over the array padded with +0.0 to a power of two
 *   (points not indexed contribute +0.0); threshold = mean + std_ratio * stddev.
 *   Keep iff d_i <= threshold (PCL) / d_i < threshold (O3D), compared in float64; points not indexed are not kept.
 *   d_i, the statistics and the flags depend on the cloud alone: not on the cell, the launch or the run.
 *   Divergences from both libraries: the variance is the two-pass form for either flavour (they use sum and sum of squares),
 *   and a cloud with fewer than K points divides by what it has instead of marking every point invalid.
 * Radius.  radius > 0 and finite, min_neighbors >= 0, else SF_ERR_INVALID.  r2 = (float)(radius * radius); count_i = the number
 *   of indexed points p with d2(x_i, p) < r2 under the float32, unfused, strict rule of sf_map_nn / sf_map_knn, the point itself
 *   included (so min(count_i, 64) is the count of sf_map_knn(x_i, 64, r2)); keep iff count_i > min_neighbors, i.e. that many
 *   neighbours besides itself, as both libraries have it.  Points not indexed get count 0 and are not kept.
 * keep [n] (1 / 0), mean_dist [n] / n_neighbors [n] and stats are in ORIGINAL point order; any of them may be NULL.
 * SF_ERR_STATE for a map that is not built.  With sf_map_profile_launches on, the map calls record the device time from their
 * first to their last kernel (the statistical form reads its two sums back in between) for sf_map_last_launch_ms. */
#define SF_SOR_PCL 0
#define SF_SOR_O3D 1
typedef struct { int64_t n_points, n_valid, n_kept; double mean, stddev, threshold; } sf_outlier_stats; /* radius: the doubles are 0 */
int sf_map_statistical_outliers(sf_map *m, int k, double std_ratio, int flavour,
                                uint8_t *keep, double *mean_dist, sf_outlier_stats *stats);   /* original point order; any may be NULL */
int sf_map_radius_outliers(sf_map *m, double radius, int min_neighbors,
                           uint8_t *keep, int32_t *n_neighbors, sf_outlier_stats *stats);
/* The same filters applied to a cloud: it is indexed with a temporary map (`cell` as in sf_map_build, 0 = automatic), flagged by
 * the device code of the map calls and compacted in place like a crop -- the order is kept, sf_cloud_last_indices reports the
 * survivors, the flags never leave the device.  An empty cloud is SF_OK with zero stats. */
int sf_cloud_remove_statistical_outliers(sf_cloud *c, int k, double std_ratio, int flavour, float cell, sf_outlier_stats *stats);
int sf_cloud_remove_radius_outliers(sf_cloud *c, double radius, int min_neighbors, float cell, sf_outlier_stats *stats);
/* Clustering (extension, no reference code): pcl::EuclideanClusterExtraction, Open3D cluster_dbscan, scikit-learn DBSCAN.
 * The window is ignored; the map's index, normals, covariances and neighbour table are not modified.  The labels are a function of
 * the cloud and the parameters alone: not of the cell, the launch or the run.
 * Edges.  r2 = (float)(eps * eps); indexed points i != j are adjacent iff d2(x_i, x_j) < r2 under the float32, unfused, strict rule
 *   of sf_map_radius_outliers (symmetric bit for bit); count_i is that call's count_i at radius = eps, the point itself included.
 * DBSCAN.  eps > 0 and finite, min_points >= 1, else SF_ERR_INVALID.  Point i is core iff count_i >= min_points (it counts itself,
 *   as scikit-learn's min_samples and Open3D's min_points do).  Clusters are the connected components of the graph restricted to
 *   the core points, numbered 0 .. C-1 in ascending order of their smallest core point's ORIGINAL index.  A point that is not core
 *   and has a core neighbour is a border point and gets the smallest label among its core neighbours' clusters; every other point,
 *   those not indexed (non-finite) included, is noise: -1.  These are the labels of scikit-learn's sequential DBSCAN; the one
 *   divergence from the libraries is < in float32 where they have <= in float64.
 * Euclidean.  DBSCAN with min_points = 1 (every indexed point is core; no border, no noise), then a size filter: clusters of fewer
 *   than min_size or more than max_size points get -1 (max_size <= 0: no upper bound; min_size >= 1, else SF_ERR_INVALID) and the
 *   others are renumbered compactly in the same order.  Divergence from PCL: it orders the clusters by size, descending; here the
 *   order is by smallest member index and sizes[] is returned for a caller to sort by.
 * labels [n] in ORIGINAL point order; sizes [min(n_clusters, cap_sizes)] per label, border points included; any of labels, sizes and
 * stats may be NULL.  n_noise: the indexed points labelled -1 (Euclidean: the points the size filter took away); n_kept: the
 * points with label >= 0; largest_size: the largest cluster left (0 when there is none).  SF_ERR_STATE for a map that is not built.
 * With sf_map_profile_launches on, the device time from the first to the last kernel is recorded for sf_map_last_launch_ms. */
typedef struct { int64_t n_points, n_valid, n_core, n_border, n_noise, n_clusters, largest_size, n_kept; } sf_cluster_stats;
int sf_map_cluster_dbscan(sf_map *m, double eps, int min_points,
                          int32_t *labels, int32_t *sizes, int64_t cap_sizes, sf_cluster_stats *stats);
int sf_map_cluster_euclidean(sf_map *m, double tolerance, int64_t min_size, int64_t max_size,
                             int32_t *labels, int32_t *sizes, int64_t cap_sizes, sf_cluster_stats *stats);
/* The same applied to a cloud, as the sf_cloud_remove_*_outliers calls are: a temporary map (`cell` as in sf_map_build), the device
 * code of sf_map_cluster_euclidean, compaction in place -- the order is kept, sf_cloud_last_indices reports the survivors, neither
 * labels nor flags leave the device.  filter_clusters keeps the points whose cluster passes the size filter.  keep_largest_cluster
 * keeps the cluster with the most points, on a tie the one with the smallest label; its stats are those of
 * sf_map_cluster_euclidean(tolerance, 1, 0) except n_kept = largest_size and n_noise = n_valid - n_kept, what the call took away.
 * An empty cloud is SF_OK with zero stats. */
int sf_cloud_filter_clusters(sf_cloud *c, double tolerance, int64_t min_size, int64_t max_size, float cell, sf_cluster_stats *stats);
int sf_cloud_keep_largest_cluster(sf_cloud *c, double tolerance, float cell, sf_cluster_stats *stats);
/* RANSAC plane segmentation and ground removal of a cloud (pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE,
 * Open3D segment_plane; EXTENSION, no reference counterpart -- the reference's floor is sf_cloud_remove_floor's z > 0).  The result is
 * a function of the cloud and the parameters alone (restated in tests/plane_ref_np.py):
 *   samples     mix = the splitmix64 step; hypothesis h of num_hypotheses samples the indices
 *               mix(seed + 0x9E3779B97F4A7C15 (3h + j + 1)) mod n, j = 0, 1, 2.
 *   hypotheses  built on the host in float64, unfused, left to right: N = (p1 - p0) x (p2 - p0), nn = Nx^2 + Ny^2 + Nz^2, N^ = N / sqrt(nn),
 *               d = -(N^ . p0), rounded to float32 once.  Oriented N^ . axis >= 0 with an axis, else the first non-zero of
 *               (N^z, N^y, N^x) is positive.  Degenerate (four NaNs): two equal indices, nn not finite or not > 0, or an axis is
 *               given and |N^ . axis| < axis_min_cos.  The axis is normalised in float64; all zeros mean none.
 *   score       t = (float)distance_threshold; x is an inlier of (a, b, c, d) iff fabsf(s) < t with s = a x; s = s + b y; s = s + c z;
 *               s = s + d in float32, unfused.  Non-finite points and NaN planes never match.
 *   choice      the largest inlier count, on a tie the smallest h.  Below min_inliers no plane is found: found = 0, the plane is
 *               four zeros, no point is an inlier, and the call returns SF_OK.
 *   refit       (refine != 0) over the inliers of the best plane: float64 moments of x - c0, c0 = -d (a, b, c); mean m, covariance,
 *               its smallest eigenvector (the routine of the map normals) signed so that it does not oppose the hypothesis;
 *               d' = -n' . (c0 + m); rounded to float32.  Fewer than 3 inliers or anything non-finite: the hypothesis stands,
 *               refined = 0.  The final inliers (n_inliers) are those of the final plane under the score rule.
 * The same call returns the same bits every time (fixed summation order, integer atomics only).  SF_ERR_INVALID, nothing touched:
 * num_hypotheses outside 1 .. 4096; a threshold that is not finite and > 0; min_inliers < 3; axis_min_cos outside [0, 1]; an axis
 * that is not finite; n >= 2^31.  An empty cloud is SF_OK with zero stats and found = 0 (plane_hypotheses: every hypothesis
 * degenerate, samples -1).  plane_hypotheses, score_planes and segment_plane leave the cloud as it is.  remove_plane compacts in place
 * like a crop -- the order is kept, sf_cloud_last_indices reports the survivors -- keeping the non-inliers, or the inliers when
 * keep_inliers != 0, and removes nothing when no plane is found.  profile != 0: device events around the scoring launches (score_ms)
 * and from the first to the last kernel (total_ms); otherwise both are -1. */
typedef struct { double distance_threshold; int32_t num_hypotheses, refine; uint64_t seed; int64_t min_inliers;
                 double axis[3], axis_min_cos; int32_t profile, pad; } sf_plane_params;
typedef struct { int64_t n_points, n_hypotheses, n_degenerate, best_index, best_count, n_inliers;
                 int32_t found, refined; float score_ms, total_ms; } sf_plane_stats;
void sf_plane_default_params(sf_plane_params *p);   /* 0.1 m, 1024, refine 1, seed 0, min_inliers 3, no axis */
int sf_cloud_plane_hypotheses(sf_cloud *c, const sf_plane_params *p, float *planes /* [H][4] */, int32_t *samples /* [H][3] or NULL */, int64_t *n_degenerate);
int sf_cloud_score_planes(sf_cloud *c, const float *planes, int64_t n_planes /* 1 .. 4096 */, double distance_threshold, int64_t *counts);
int sf_cloud_segment_plane(sf_cloud *c, const sf_plane_params *p, float plane[4], uint8_t *inlier /* [n] or NULL */, sf_plane_stats *stats);
int sf_cloud_remove_plane(sf_cloud *c, const sf_plane_params *p, int keep_inliers, float plane[4], sf_plane_stats *stats);
/* Per-label boxes and multi-box removal (extension, no reference code; PCL getMinMax3D / MomentOfInertiaEstimation after
 * EuclideanClusterExtraction, Open3D get_axis_aligned_bounding_box / get_oriented_bounding_box per cluster).
 * Membership.  Point i belongs to label l = labels[i] iff 0 <= l < n_labels and the point is finite.  A label outside that range
 *   (-1 included) counts as n_ignored whatever the point holds; a non-finite point with a label in range counts as n_nonfinite;
 *   n_points = n_labelled + n_ignored + n_nonfinite.  A label without members: valid = 0, count = 0, every other field zero.
 * lo, hi: the float32 minimum and maximum per coordinate.  Pivot c0 = ((double)lo + (double)hi) / 2.
 * Moments: float64 sums S1 of d = (double)x - c0 and S2 of d d^T over the members; mean = c0 + S1 / count,
 *   cov = S2 / count - (S1 / count)(S1 / count)^T (population; xx xy xz yy yz zz).  The summation order is a function of n and
 *   the labels alone; no float atomics: the same call returns the same bits every time.
 * Axes (the columns of the row-major R).  SF_BOX_AABB: the identity, eigenvalues = the variances xx, yy, zz.
 *   SF_BOX_PCA: the symmetric Jacobi eigen-solve of cov, eigenvalues descending, ties in index order; a0 and a1 each signed so
 *   that their component of largest magnitude (the first such on a tie) is positive; a2 = a0 x a1.
 *   SF_BOX_UPRIGHT: u = up normalised in float64 (all zeros: +z); e1 = normalize(u x e_k), k the coordinate of smallest |u_k|
 *   (the first on a tie), e2 = u x e1; c11, c12, c22 the covariance in (e1, e2); theta = atan2(2 c12, c11 - c22) / 2;
 *   a0 = cos(theta) e1 + sin(theta) e2 signed as above, a2 = u, a1 = a2 x a0; eigenvalues = the variances along a0, a1, a2.
 *   A covariance that is not finite: the identity, zero eigenvalues, valid = 2.
 * center, extent: pmin_k, pmax_k = the minimum and maximum over the members of (d_x a_kx + d_y a_ky) + d_z a_kz in float64,
 *   unfused; h_k = (pmin_k + pmax_k) / 2; center_i = c0_i + R[3i] h_0 + R[3i+1] h_1 + R[3i+2] h_2, the exact value rounded once
 *   (evaluated in double-double: the crop subtracts the rounded center, so every further rounding would move the faces against the
 *   members on them); extent_k = pmax_k - pmin_k.  center, R and extent are the arguments of sf_cloud_crop_obb (extent: full
 *   lengths); a member on a face may still miss its own box's crop by the one rounding of center: pass a margin of an ulp of it.
 * SF_ERR_INVALID, nothing touched: n_labels < 0 or > 2^24; n >= 2^31; an unknown mode; an up that is not finite.  An empty cloud
 * is SF_OK with zero stats and every box invalid.  The cloud is not modified.  profile != 0: device_ms = the device time from
 * the first to the last kernel (the label upload excluded), otherwise -1.
 * sf_cloud_cluster_boxes: the labels of sf_map_cluster_euclidean(tolerance, min_size, max_size) on a temporary map of the cloud
 *   (`cell` as in sf_map_build) never leave the device; boxes [min(n_clusters, cap_boxes)] in label order, bit for bit those of
 *   sf_cloud_label_boxes given these labels, whatever the cell.  cstats / bstats may be NULL.
 * sf_cloud_remove_boxes: a point is inside iff it passes sf_cloud_crop_obb's float64 predicate (the same expressions in the same
 *   order) for at least one of the n_boxes boxes, each with extent_k + 2 margin; a non-finite point is never inside.  Compacts in
 *   place like a crop -- the order is kept, sf_cloud_last_indices reports the survivors -- keeping the outside points, or the
 *   inside ones when keep_inside != 0.  n_boxes 0 .. 1024 (0: nothing is inside); a margin that is not finite is SF_ERR_INVALID.
 *   *n_inside (may be NULL) = the points inside. */
#define SF_BOX_AABB 0
#define SF_BOX_PCA 1
#define SF_BOX_UPRIGHT 2
typedef struct { int32_t mode, profile; double up[3]; } sf_box_params;
typedef struct { int64_t count; float lo[3], hi[3]; double mean[3], cov[6];
                 double center[3], R[9], extent[3], eigenvalues[3]; int32_t valid, pad; } sf_label_box;
typedef struct { int64_t n_points, n_labelled, n_ignored, n_nonfinite, n_labels, n_valid; float device_ms; int32_t pad; } sf_box_stats;
int sf_cloud_label_boxes(sf_cloud *c, const int32_t *labels /* host [n] */, int64_t n_labels, const sf_box_params *p,
                         sf_label_box *boxes /* [n_labels] */, sf_box_stats *stats);
int sf_cloud_cluster_boxes(sf_cloud *c, double tolerance, int64_t min_size, int64_t max_size, float cell, const sf_box_params *p,
                           sf_label_box *boxes, int64_t cap_boxes, sf_cluster_stats *cstats, sf_box_stats *bstats);
int sf_cloud_remove_boxes(sf_cloud *c, const double *center /* [B][3] */, const double *R /* [B][9] */, const double *extent /* [B][3] */,
                          int64_t n_boxes /* 0 .. 1024 */, double margin, int keep_inside, int64_t *n_inside);
/* FPFH descriptors and descriptor matching (extension, no reference code; pcl::FPFHEstimation, Open3D compute_fpfh_feature and
 * the nearest-descriptor correspondences both libraries feed to a global registration; DESIGN §21, restated in
 * tests/fpfh_ref_np.py).  The first step from "refine a pose" to "find a pose": estimating the pose from the matches is
 * sf_cloud_register_pairs, below.
 * sf_features: n rows of SF_FPFH_DIM float32 and one validity byte per row on the device, in the ORIGINAL point order of whatever
 *   produced them.  A row that holds a non-finite value is invalid whatever flag came with it (valid NULL: every row is offered as
 *   valid); the byte always comes out as 0 or 1.  download: cap >= n rows, *n = n (SF_ERR_INVALID when cap is too small, *n set).
 * Neighbours.  r2 = (float)(radius * radius); j is a neighbour of i iff both are indexed, j != i and d2(x_i, x_j) < r2 under the
 *   float32, unfused, strict rule of sf_map_radius_outliers (symmetric bit for bit; the same walk, so the same proof that nothing
 *   is lost).  The window is ignored; the map's index, normals, covariances and neighbour table are not modified.
 * Normals.  The stored normal of a point, converted to float64; SF_ORIENT_NONE: as stored; SF_ORIENT_DIRECTION: negated when
 *   n . toward < 0 (Open3D's default with toward = +z); SF_ORIENT_VIEWPOINT: negated when n . (toward - x) < 0 (PCL's viewpoint
 *   rule) -- as the normal is loaded, the stored normals stay as they are.  A point whose normal is all zeros or not finite has no
 *   normal: it contributes to nothing and gets no descriptor.  A map without normals: SF_ERR_STATE.
 * Pair (i, j), float64, unfused, in the order written (dot products and squares left to right over x, y, z): d = x_j - x_i,
 *   L = sqrt(d.d), L == 0 skips the pair; a_i = (n_i.d) / L, a_j = (n_j.d) / L; if |a_i| < |a_j|: source j, target i, d = -d,
 *   phi = -a_j, else source i, target j, phi = a_i; v = d x n_src, |v| == 0 skips the pair, v = v / |v|, w = n_src x v;
 *   alpha = v . n_tgt; theta = atan2(w . n_tgt, n_src . n_tgt).
 * Bins.  floor(11 (theta + pi) / (2 pi)), floor(11 (alpha + 1) / 2), floor(11 (phi + 1) / 2), each clamped to 0 .. 10; a row is
 *   [0, 11) theta, [11, 22) alpha, [22, 33) phi.
 * SPFH.  cnt_i[b] = the pairs of i that were not skipped, per bin; P_i their number; SPFH_i[b] = cnt_i[b] * (100.0 / P_i);
 *   P_i == 0: no SPFH.  sf_map_compute_spfh returns cnt ([n][33]) and P ([n]) in original order, zeros for points without one:
 *   integers, so they depend on the cloud and the parameters alone, not on the cell.
 * FPFH.  Over the neighbours j of i that have an SPFH and d2_ij > 0, in the order the index walks them:
 *   W[b] = sum SPFH_j[b] / (double)d2_ij (d2_ij the float32 value of the neighbour rule: the weight is the squared distance, as in
 *   both libraries); per group of 11 bins S_g = sum W[b] in ascending b; F_i[b] = (S_g > 0 ? W[b] * (100.0 / S_g) : 0) +
 *   SPFH_i[b], rounded to float32 once.  Point i gets a descriptor (valid = 1) iff it has an SPFH, otherwise 33 zeros and 0.
 *   The same call on the same index returns the same bits every time (integer atomics only); another cell moves the float64 sums
 *   W by their rounding, nothing else.
 * SF_ERR_INVALID, nothing touched: a radius that is not finite and > 0, an unknown orient, a toward that is not finite.  An empty
 *   map is SF_OK with zero stats and an empty set.  n_valid: the indexed points; n_featured: the valid rows; n_pairs = sum P_i,
 *   max_pairs = max P_i.  profile != 0: spfh_ms and fpfh_ms are the device-event times of the two passes, otherwise both are -1.
 * sf_cloud_compute_fpfh: a temporary map of the cloud (`cell` as in sf_map_build, 0 = automatic),
 *   sf_map_estimate_normals((float)normal_radius) on it, then the device code of sf_map_compute_fpfh: bit for bit what those
 *   three calls give.  The cloud is not modified.
 * sf_features_match.  D(a, b): float32, unfused, ascending k: acc = 0; for k = 0 .. 32: t = a[k] - b[k]; t = t * t; acc = acc + t.
 *   Invalid rows are never candidates and never queries.  idx[i] = the valid dst row with the smallest (D, index), dist2[i] its D,
 *   second2[i] the smallest D over the OTHER valid rows (+inf when there is none); idx = -1, dist2 = second2 = +inf for an invalid
 *   query or an empty candidate set.  i is accepted iff idx[i] >= 0, and with 0 < ratio < 1 also
 *   dist2[i] < (float)(ratio * ratio) * second2[i], and with mutual != 0 also: the best src row for dst row idx[i] under the same
 *   (D, index) rule is i.  pairs: the accepted (i, idx[i]) in ascending i, truncated at cap_pairs; n_matched counts them all.
 *   idx, dist2, second2 and pairs may be NULL.  SF_ERR_INVALID: different contexts, either side >= 2^31 rows.  profile != 0:
 *   match_ms = the device time from the first to the last kernel, otherwise -1. */
#define SF_FPFH_DIM 33
#define SF_ORIENT_NONE 0
#define SF_ORIENT_DIRECTION 1
#define SF_ORIENT_VIEWPOINT 2
typedef struct sf_features sf_features;
typedef struct { double radius; int32_t orient, profile; double toward[3]; } sf_fpfh_params;
typedef struct { int64_t n_points, n_valid, n_featured, n_pairs, max_pairs; float spfh_ms, fpfh_ms; } sf_fpfh_stats;
typedef struct { double ratio; int32_t mutual, profile; } sf_match_params;   /* ratio <= 0 or >= 1: no ratio test */
typedef struct { int64_t n_src, n_dst, n_src_valid, n_dst_valid, n_matched; float match_ms; int32_t pad; } sf_match_stats;
int sf_features_create(sf_ctx *ctx, sf_features **out);
void sf_features_destroy(sf_features *f);
int sf_features_size(const sf_features *f, int64_t *n);
int sf_features_upload(sf_features *f, const float *rows /* [n][33] */, const uint8_t *valid /* [n] or NULL */, int64_t n);
int sf_features_download(sf_features *f, float *rows /* [cap][33] */, uint8_t *valid /* [cap] or NULL */, int64_t cap, int64_t *n);
void sf_fpfh_default_params(sf_fpfh_params *p);     /* radius 0 (to be set), SF_ORIENT_NONE, no profile, toward +z */
void sf_match_default_params(sf_match_params *p);   /* no ratio test, not mutual, no profile */
int sf_map_compute_fpfh(sf_map *m, const sf_fpfh_params *p, sf_features *out, sf_fpfh_stats *stats);
int sf_map_compute_spfh(sf_map *m, const sf_fpfh_params *p, uint32_t *counts /* [n][33] */, int32_t *n_pairs /* [n] */);
int sf_cloud_compute_fpfh(sf_cloud *c, double normal_radius, const sf_fpfh_params *p, float cell, sf_features *out, sf_fpfh_stats *stats);
int sf_features_match(sf_features *src, sf_features *dst, const sf_match_params *p,
                      int32_t *idx /* [n_src] */, float *dist2 /* [n_src] */, float *second2 /* [n_src] or NULL */,
                      int32_t *pairs /* [cap][2] or NULL */, int64_t cap_pairs, sf_match_stats *stats);
/* RANSAC pose estimation from descriptor matches (extension, no reference code; pcl::SampleConsensusPrerejective, Open3D
 * registration_ransac_based_on_correspondence; DESIGN §22, restated in tests/reg_ref_np.py).  The consumer of sf_features_match:
 * src and dst are two clouds of one context, pairs [m][2] int32 the (i, j) that sf_features_match returns, i into src, j into dst.
 *   pairs       an index outside its cloud: SF_ERR_INVALID, nothing touched.  A pair with a non-finite point is never an inlier and
 *               makes every hypothesis that samples it degenerate (NaN arithmetic).  Scoring runs over the m pairs, not over a
 *               nearest-neighbour search of the whole source.
 *   samples     mix = the splitmix64 step of sf_cloud_segment_plane; hypothesis h of num_hypotheses samples the pairs
 *               k_j = mix(seed + 0x9E3779B97F4A7C15 (3h + j + 1)) mod m, j = 0, 1, 2; (s_j, t_j) are their points widened to float64.
 *   hypothesis  on the device, float64, unfused, in the order written (sums and dot products left to right over x, y, z).
 *               status 1 (degenerate): two equal k_j; c = (s1 - s0) x (s2 - s0), cc = cx cx; cc = cc + cy cy; cc = cc + cz cz not > 0 or
 *               not finite, likewise for t; or the resulting transform is not finite.  status 2 (rejected): edge_similarity > 0 and
 *               for an edge (a, b) of (0,1), (0,2), (1,2) not (ls2 >= e2 * lt2 && lt2 >= e2 * ls2), ls2 = |s_a - s_b|^2,
 *               lt2 = |t_a - t_b|^2 (dx dx, + dy dy, + dz dz), e2 = edge_similarity * edge_similarity -- squared lengths, no square
 *               root.  status 0 otherwise: cs = ((s0 + s1) + s2) / 3, ct likewise, H_ab = sum_j (s_j - cs)_a (t_j - ct)_b in ascending j,
 *               Horn's symmetric 4x4 matrix of H solved by the Jacobi eigen-solve of the library, q = the eigenvector of the largest
 *               eigenvalue (the first index on a tie) divided by its norm and signed q_w >= 0, R the rotation of q (always proper),
 *               t = ct - R cs.  T is row-major 4x4, src -> dst.  Statuses 1 and 2 carry sixteen NaNs.
 *   score       float32, unfused: Tf = the twelve entries of [R | t] rounded to float32, t2 = (float)(distance_threshold *
 *               distance_threshold); qx = Tf00 x; qx = qx + Tf01 y; qx = qx + Tf02 z; qx = qx + Tf03, likewise qy, qz; dx = qx - tx,
 *               dy, dz; d2 = dx dx; d2 = d2 + dy dy; d2 = d2 + dz dz; the pair is an inlier iff d2 < t2.  count_h = the inliers, 0 for
 *               status 1 and 2.
 *   choice      the largest count, on a tie the smallest h (all counts 0: h = 0).  Below min_inliers: found = 0, T = the identity, no
 *               inlier, SF_OK.  top [top_k] (may be NULL when top_k = 0): the best in (count descending, h ascending) order, only
 *               status 0 with count > 0; stats->n_top of them are written.
 *   refit       refine_rounds times: over the inliers of the current Tf the float64 record (n, sum s', sum t', sum s' t'^T) with
 *               s' = s - s_ref, t' = t - t_ref, the references being sample 0 of the chosen hypothesis; H = sum s' t'^T -
 *               (sum s')(sum t')^T / n, cs = s_ref + sum s' / n, ct likewise, then the same solve.  Fewer than 3 inliers or a
 *               transform that is not finite: the previous transform stands and the rounds end (rounds_done counts the others).
 *   outputs     T [16]; inlier [m] (may be NULL) and n_inliers under the final Tf; fitness = n_inliers / m; rmse =
 *               sqrt(sum (double)d2 / n_inliers) (0 without inliers), the sum taken over tiles of 256 consecutive pairs (a non-inlier
 *               adds 0): within each 64 a balanced binary tree over adjacent pairs, the four 64s left to right, the tiles in
 *               ascending order.  Integer atomics only, every order fixed by m and the parameters: the same call returns the same bits.
 * SF_ERR_INVALID, nothing touched: num_hypotheses outside 1 .. 2^20; refine_rounds outside 0 .. 8; min_inliers < 3; top_k outside
 * 0 .. 64; a threshold that is not finite and > 0; an edge_similarity that is NaN or > 1; clouds of different contexts; m < 0 or
 * m >= 2^31.  m < 3 or an empty cloud: SF_OK, found = 0, zero stats (pair_hypotheses: every status 1, samples -1; score_poses: zero
 * counts).  No call modifies a cloud or its last indices.  profile != 0: hyp_ms (gather and hypotheses), score_ms (compaction,
 * scoring, choice) and refit_ms (refit rounds and final flags) are device-event times, otherwise -1.
 * sf_cloud_pair_hypotheses: the first two stages alone.  sf_cloud_score_poses: the scoring stage alone on n_poses (1 .. 2^20)
 * uploaded float32 transforms T12 [n_poses][12] (the rows of [R | t]). */
typedef struct { double distance_threshold, edge_similarity; int32_t num_hypotheses, refine_rounds; int64_t min_inliers;
                 int32_t top_k, profile; uint64_t seed; } sf_reg_params;
typedef struct { int32_t h, status; int64_t count; double T[16]; } sf_reg_candidate;
typedef struct { int64_t n_pairs, n_degenerate, n_rejected, n_scored, best, best_count, n_inliers; int32_t found, rounds_done;
                 double fitness, rmse; float hyp_ms, score_ms, refit_ms; int32_t n_top; } sf_reg_stats;
void sf_reg_default_params(sf_reg_params *p);       /* threshold 0 (to be set), similarity 0.9, 4096, 2 rounds, min_inliers 3, top_k 0, seed 0 */
int sf_cloud_register_pairs(sf_cloud *src, sf_cloud *dst, const int32_t *pairs /* [m][2] */, int64_t m, const sf_reg_params *p,
                            double *T /* [16] */, uint8_t *inlier /* [m] or NULL */, sf_reg_candidate *top /* [top_k] or NULL */, sf_reg_stats *stats);
int sf_cloud_pair_hypotheses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs /* [m][2] */, int64_t m, const sf_reg_params *p,
                             int32_t *samples /* [H][3] or NULL */, int32_t *status /* [H] */, double *T /* [H][16] or NULL */);
int sf_cloud_score_poses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs /* [m][2] */, int64_t m, const float *T12 /* [n_poses][12] */,
                         int64_t n_poses, double distance_threshold, int64_t *counts /* [n_poses] */);
/* ISS keypoints and keypoint-restricted descriptor sets (extension, no reference code; Intrinsic Shape Signatures, Zhong 2009:
 * Open3D compute_iss_keypoints, the unweighted form of pcl::ISSKeypoint3D; DESIGN §23, restated in tests/iss_ref_np.py).  The step in
 * front of the FPFH / match / RANSAC chain: which few hundred points are worth describing and matching.  Every per-point output
 * is in ORIGINAL point order.
 * Neighbours.  rs2 = (float)(salient_radius * salient_radius); N_i = the indexed points j with d2(x_i, x_j) < rs2 under the float32,
 *   unfused, strict rule of sf_map_radius_outliers, the point itself included; count_i = |N_i| is that call's count (the same walk,
 *   the same proof that nothing is lost; symmetric bit for bit).  The window is ignored; the map's index, normals, covariances
 *   and neighbour table are not modified; normals are not needed.
 * Scatter, float64, unfused, in the order written, centred on the point itself: per neighbour d_a = (double)x_j[a] - (double)x_i[a]
 *   (exact); in the order the index walks them s_a = s_a + d_a and q_ab = q_ab + d_a * d_b for ab = xx, xy, xz, yy, yz, zz; then
 *   n = count_i, m_a = s_a / n, C_ab = q_ab / n - m_a * m_b: the unweighted covariance about the neighbourhood mean (Open3D's form;
 *   PCL's scatter about the query point is not offered).
 * Eigenvalues.  The Jacobi eigen-solve of the library on C; the three diagonal values sorted descending, each clamped to
 *   max(lambda, 0): lambda1 >= lambda2 >= lambda3 >= 0.  A point that is not indexed: count 0, three zeros, salient = 0.
 * Salient, compared in float64: count_i >= min_neighbors && lambda2 < gamma_21 * lambda1 && lambda3 < gamma_32 * lambda2 &&
 *   lambda3 > min_lambda3.  The products stand in for the libraries' quotients, so a degenerate neighbourhood (collinear, a single
 *   point) is simply not salient and no NaN arises.  min_lambda3 is an absolute floor in m^2 (not in Open3D): it keeps an exactly or
 *   nearly planar edge, whose lambda3 is rounding noise, out of the competition below.
 * Non-maximum suppression.  rn2 = (float)(non_max_radius * non_max_radius), c_i = the count under the same rule at rn2 (the point
 *   itself included).  i is a keypoint iff it is salient, c_i >= min_neighbors, and no salient j != i with d2(x_i, x_j) < rn2 has
 *   lambda3_j > lambda3_i, or lambda3_j == lambda3_i and j < i in original order.  Points that are not salient never suppress.
 *   (Open3D keeps both members of a tie; here the smallest original index of equal maxima wins: coincident points, one keypoint.)
 * Outputs.  indices: the keypoints in ascending original index, truncated at cap; *n_keypoints counts them all; flags [n]: 1 / 0 per
 *   point; stats: n_valid = the indexed points, n_salient, n_keypoints, max_neighbors = the largest count_i; profile != 0:
 *   saliency_ms / nms_ms are the device-event times of the two passes, otherwise both are -1.  Integer atomics serve the counts
 *   only: the same call on the same index returns the same bits, sf_map_iss_keypoints computes the very lambda that
 *   sf_map_iss_saliency returns (one kernel), and another cell moves s and q by their float64 rounding, nothing else.
 * SF_ERR_INVALID, nothing touched: a radius that is not finite and > 0, a gamma that is NaN or not in (0, 1], a min_lambda3 that is
 *   NaN or negative, min_neighbors < 1, cap < 0, indices == NULL with cap > 0.  SF_ERR_STATE: a map that is not built.  An empty map
 *   is SF_OK with zero stats.
 * sf_cloud_iss_keypoints: a temporary map of the cloud (`cell` as in sf_map_build, 0 = automatic), then the device code of
 *   sf_map_iss_keypoints: bit for bit what those two calls give.  The cloud and its last indices are not modified.
 * sf_features_gather: row r of out = row rows[r] of src with its validity byte, in the order given (repeats allowed); k = 0
 *   empties out.  SF_ERR_INVALID, nothing touched: an index outside src, out == src, different contexts, k < 0. */
typedef struct { double salient_radius, non_max_radius, gamma_21, gamma_32, min_lambda3; int32_t min_neighbors, profile; } sf_iss_params;
typedef struct { int64_t n_points, n_valid, n_salient, n_keypoints, max_neighbors; float saliency_ms, nms_ms; } sf_iss_stats;
void sf_iss_default_params(sf_iss_params *p);   /* radii 0 (to be set), gammas 0.975, min_lambda3 0, min_neighbors 5, no profile */
int sf_map_iss_saliency(sf_map *m, const sf_iss_params *p, double *lambda /* [n][3] */, int32_t *n_neighbors /* [n] */, uint8_t *salient /* [n] */);  /* any may be NULL */
int sf_map_iss_keypoints(sf_map *m, const sf_iss_params *p, int32_t *indices /* [cap] or NULL */, int64_t cap, int64_t *n_keypoints,
                         uint8_t *flags /* [n] or NULL */, sf_iss_stats *stats);
int sf_cloud_iss_keypoints(sf_cloud *c, const sf_iss_params *p, float cell, int32_t *indices, int64_t cap, int64_t *n_keypoints, sf_iss_stats *stats);
int sf_features_gather(sf_features *src, const int32_t *rows /* [k] */, int64_t k, sf_features *out);
/* Normal Distributions Transform scan-to-map registration (extension: Magnusson 2009, PCL's NormalDistributionsTransform; DESIGN §24,
 * restated in tests/ndt_ref_np.py).  No correspondence search and no normals; the basin is about the voxel size.
 * Target voxels.  The grid index of the target at cell = resolution is the one sf_map_build(m, cloud, resolution) makes (origin,
 *   float32 binning, table limits; SF_ERR_OVERFLOW when the table does not fit, or holds 2^31 cells or more).  Per occupied cell,
 *   float64, two passes: count m, mean mu, Sigma = sum (x - mu)(x - mu)^T / (m - 1); the library's Jacobi eigen-solve.  A cell is a
 *   voxel iff m >= min_points and lambda_max is finite and > 0; then lambda~_i = max(lambda_i, min_eig_ratio * lambda_max),
 *   cov = V L~ V^T, B = V L~^-1 V^T.  sf_ndt_download_voxels: the voxels in ascending cell id (cell = (z * dims[1] + y) * dims[0] + x);
 *   mean [n][3], cov and icov [n][6] as xx xy xz yy yz zz; any array may be NULL; cap below the count with an array given is
 *   SF_ERR_INVALID (*n set).  The same target gives the same bits every build.  sf_ndt_set_target_map takes the map's points in
 *   their original order: bit for bit what sf_ndt_set_target_cloud of the cloud gives.  A grown map rebuilds its voxels in full.
 * Objective.  p = outlier_ratio, r = resolution: c1 = 10 (1 - p), c2 = p / r^3, d3 = -ln c2, d1 = -ln(c1 + c2) - d3,
 *   d2 = -2 ln((-ln(c1 e^-1/2 + c2) - d3) / d1).  y = T x in float64 (rows summed left to right, unfused); grid coordinate
 *   (y - org) * inv_h in float64; a point with a coordinate < 0 or >= dims has no home cell and contributes nothing (no clamp).
 *   SF_NDT_DIRECT1: the home cell; SF_NDT_DIRECT7: plus the face neighbours inside the grid.  Each voxel met gives the term
 *   d1 exp(-(d2 / 2) q^T B q), q = y - mu; the score is their sum (d1 < 0: smaller is better).  gradient and hessian are taken at
 *   delta = 0 of y(delta) = M(delta) y, delta = (rx, ry, rz, tx, ty, tz), M = [Rz Ry Rx | t] as everywhere in the library; the
 *   hessian is the full 6 x 6, row-major, symmetric bit for bit.  n_inside: the points that met a voxel; n_terms: the terms.
 * Step.  H = V L V^T (Jacobi), l~_i = max(|l_i|, hessian_floor * max_j |l_j|), delta = -V L~^-1 V^T g, scaled to step_size when
 *   longer (radians and metres together), T <- M(delta) T.  An alignment stops after max_iterations steps, or (converged = 1)
 *   when the applied |delta| < transformation_epsilon.  When an evaluation finds no term, or a Hessian that is all zero or not
 *   finite, SF_NDT_FLAG_NO_OVERLAP is set, the pose stays as it is and score, gradient and hessian are zeros: no NaN is returned.
 *   iterations counts the steps taken, modified those in which an eigenvalue was negative or floored.  score, gradient and
 *   hessian of a result are those at its final pose T (one more pass), bit for bit what sf_ndt_derivatives gives there.
 * sf_ndt_set_source_batch: batch 1 .. 64 scans of n_per_scan points; sf_ndt_set_source_cloud: one scan (copied).  sf_ndt_align
 *   aligns entry 0 from init and fills trace [max_iterations + 1][16] (or NULL) with T_0 .. T_iterations, the rest untouched;
 *   sf_ndt_align_batch takes inits [batch][16] and fills out [batch]: entry b is bit for bit the single alignment of scan b.
 *   sf_ndt_derivatives evaluates entry 0 at poses [k][16] (T, score, gradient, hessian, n_inside, n_terms are filled).  All
 *   iterations are enqueued without a host synchronisation; the call waits once.  profile != 0: build_ms / align_ms of
 *   sf_ndt_stats_read are device-event times of the last voxel build / of the launches of the last alignment or evaluation call
 *   (sf_ndt_derivatives: of its last 64 poses), otherwise -1.
 * SF_ERR_INVALID ("bad arguments"), before any device work: NULL handles; resolution <= 0 or not finite; outlier_ratio outside
 *   (0, 1); min_points < 3; neighbours not 1 or 7; max_iterations outside [0, 1024]; step_size <= 0; batch outside [1, 64]; an
 *   evaluation or alignment before a target and a source are set.  An empty target or source is no error: NO_OVERLAP. */
#define SF_NDT_DIRECT1 1
#define SF_NDT_DIRECT7 7
#define SF_NDT_FLAG_NO_OVERLAP 1
typedef struct sf_ndt sf_ndt;
typedef struct { double resolution, outlier_ratio, step_size, transformation_epsilon, min_eig_ratio, hessian_floor; int32_t min_points, neighbours, max_iterations, profile; } sf_ndt_params;
typedef struct { double T[16], score, gradient[6], hessian[36]; int64_t n_inside, n_terms; int32_t iterations, converged, modified, flags; } sf_ndt_result;
typedef struct { int64_t n_points, n_cells, n_occupied, n_voxels; int32_t dims[3]; float build_ms, align_ms; } sf_ndt_stats;
void sf_ndt_default_params(sf_ndt_params *p);   /* resolution 1, outlier_ratio 0.55, step_size 0.1, transformation_epsilon 1e-4, min_eig_ratio 0.01, hessian_floor 1e-6, min_points 6, DIRECT7, 30 iterations, no profile */
int sf_ndt_create(sf_ctx *ctx, const sf_ndt_params *p, sf_ndt **out);
void sf_ndt_destroy(sf_ndt *ndt);
int sf_ndt_set_target_cloud(sf_ndt *ndt, sf_cloud *cloud);
int sf_ndt_set_target_map(sf_ndt *ndt, sf_map *map);
int sf_ndt_download_voxels(sf_ndt *ndt, int64_t *cell, int32_t *count, double *mean, double *cov, double *icov, int64_t cap, int64_t *n);
int sf_ndt_set_source_cloud(sf_ndt *ndt, sf_cloud *cloud);
int sf_ndt_set_source_batch(sf_ndt *ndt, const float *xyz, int64_t n_per_scan, int batch);
int sf_ndt_derivatives(sf_ndt *ndt, const double *poses, int64_t k, sf_ndt_result *out);
int sf_ndt_align(sf_ndt *ndt, const double init[16], sf_ndt_result *out, double *trace);
int sf_ndt_align_batch(sf_ndt *ndt, const double *inits, sf_ndt_result *out);
int sf_ndt_stats_read(sf_ndt *ndt, sf_ndt_stats *out);
/* Backtracking line search and coarse-to-fine levels for NDT (restated in tests/ndt_ls_ref_np.py).  Off by default: an
 * alignment is then bit for bit the one above.  With sf_ndt_set_line_search(trials >= 1), per batch entry and iteration:
 *   1. the derivatives at T as above: phi0 (the score), g, H; the usability check and SF_NDT_FLAG_NO_OVERLAP as above;
 *   2. d = -V L~^-1 V^T g, the solve above before the scaling (same floor, same `modified`); raw = |d|, not finite: as above;
 *   3. alpha_max = raw > step_max ? step_max / raw : 1.0; slope = ((((g0 d0 + g1 d1) + g2 d2) + g3 d3) + g4 d4) + g5 d5, unfused;
 *   4. trial k = 0 .. trials - 1: alpha_k = ldexp(alpha_max, -k), delta_k[i] = alpha_k * d[i], T_k = M(delta_k) T;
 *   5. phi_k, terms_k: the score and the number of terms of the entry's scan at T_k, bit for bit what sf_ndt_derivatives (and
 *      sf_ndt_scores) return there; all trials of all entries are evaluated in one launch;
 *   6. the smallest k with terms_k > 0, phi_k finite and phi_k <= phi0 + (armijo * alpha_k) * slope is accepted: T <- T_k,
 *      iterations + 1, modified + 1 when an eigenvalue was negative or floored, converged when alpha_k * raw < transformation_epsilon;
 *   7. no trial accepted: flags |= SF_NDT_FLAG_LINE_SEARCH_STALLED, the pose stays, the entry is done with converged = 0 (no
 *      step was taken, so `modified` does not count it).
 *   params.step_size is not used in this mode; the final pass (score, gradient, hessian at the final pose) is as above.
 * sf_ndt_scores: score and n_terms of entry 0 of the source at poses [k][16], any k; a sum that is not finite gives (0, 0).
 * sf_ndt_line_search_read: entry 0 of the last sf_ndt_align, one row per iteration whose trials were evaluated (the stalled one
 *   included, so iterations or iterations + 1 rows): the direction d as `delta`, phi / n_terms of every trial (zeros beyond
 *   `trials`), chosen = the accepted k or -1.  rows may be NULL (cap 0) to ask for *n; cap below the count with rows given is
 *   SF_ERR_INVALID (*n set).  SF_ERR_STATE when the last sf_ndt_align ran without the search, or none has run.
 * sf_ndt_align_levels: several sf_ndt on one target at descending resolution, each with its source set (the same scans), aligned
 *   in turn: level l is bit for bit sf_ndt_align_batch(levels[l]) from the poses where level l - 1 ended (level 0: inits),
 *   whatever that level's flags were; out [batch] is the last level's results verbatim, per_level [n_levels][batch] every level's.
 * SF_ERR_INVALID ("bad arguments"), before any device work: NULL handles; trials outside [0, 16]; step_max not > 0 or not finite;
 *   armijo outside (0, 1); n_levels < 1; levels of different contexts, batch sizes or source sizes; a level without target or
 *   source. */
#define SF_NDT_FLAG_LINE_SEARCH_STALLED 2
#define SF_NDT_MAX_TRIALS 16
typedef struct { int32_t trials, pad; double step_max, armijo; } sf_ndt_line_search;            /* trials 0: off */
typedef struct { double alpha_max, raw_length, phi0, slope, delta[6], phi[16]; int64_t n_terms[16]; int32_t chosen, trials; } sf_ndt_ls_row;  /* chosen -1: stalled */
void sf_ndt_default_line_search(sf_ndt_line_search *p);                                         /* 8 trials, step_max 1.0, armijo 1e-4 */
int sf_ndt_set_line_search(sf_ndt *ndt, const sf_ndt_line_search *p);                           /* NULL or trials 0: off */
int sf_ndt_scores(sf_ndt *ndt, const double *poses, int64_t k, double *score, int64_t *n_terms);/* entry 0 at poses [k][16], any k */
int sf_ndt_line_search_read(sf_ndt *ndt, sf_ndt_ls_row *rows, int64_t cap, int64_t *n);         /* entry 0 of the last sf_ndt_align with the search on: one row per evaluated iteration, the stalled one included */
int sf_ndt_align_levels(sf_ndt *const *levels, int n_levels, const double *inits, sf_ndt_result *out /* [batch] */, sf_ndt_result *per_level /* [n_levels][batch] or NULL */);
/* Range images and visibility-based removal of stale map points (extension, no reference code; the organised cloud of a LiDAR
 * driver, Removert's range-image comparison, OctoMap-style free-space carving; DESIGN §28, restated in tests/visibility_ref_np.py).
 * Everything below is float64, unfused, evaluated left to right as written.
 * Sensor frame.  With a pose T [16] row-major, parent <- sensor (the form sf_icp returns): d_k = (double)p_k - T[4k+3];
 *   x = (T[0] d0 + T[4] d1) + T[8] d2, y = (T[1] d0 + T[5] d1) + T[9] d2, z = (T[2] d0 + T[6] d1) + T[10] d2 -- R^T (p - t), no
 *   inversion.  NULL is the identity through the same expressions: the cloud already is in the sensor frame.  So one call makes an
 *   organised range image of a scan as received, or renders a map from a pose into the scan one would expect there.
 * Range and angles.  h2 = x x + y y; r = sqrt(h2 + z z); az = atan2(y, x); el = atan2(z, sqrt(h2)).
 * Pixel.  PI = the double nearest pi.  u = (az + PI) / (2 PI) * W, col = floor(u), col - W when col >= W (+pi and -pi are one
 *   column); v = (el - el_min) / (el_max - el_min) * H, row = floor(v), row 0 the lowest elevation.  The point is outside
 *   (n_outside) when v < 0, when row >= H, or when r > 0 && min_range <= r && r <= max_range is false; a point with a coordinate
 *   that is not finite counts as n_nonfinite; n_points = n_projected + n_outside + n_nonfinite.
 * Content.  Each pixel holds the minimum over its points of the key ((uint64)bits((float)r) << 32) | (uint32)i, i the point's index
 *   in the cloud: the smallest range and on a tie the smallest index, by one 64-bit integer atomicMin per point (a non-negative
 *   float's bits order like the float; no float atomics), the same bits on every run.  An empty pixel downloads as +inf and -1;
 *   n_filled = the pixels that are not empty.  device_ms = the device time of the fill and the two kernels of the build.
 * SF_ERR_INVALID, nothing touched: width outside 1 .. 16384 or height outside 1 .. 4096; bounds that are not finite or el_min >=
 *   el_max; min_range < 0 or max_range <= min_range; a pose that is not finite; n >= 2^31.  An empty cloud is SF_OK with an empty
 *   image; a build replaces what the image held; a new image is empty.
 * Class of a point against one image (pose: map <- sensor of the scan the image was built from).  The point goes through the
 *   sensor-frame and pixel rule above with the image's parameters; outside, not finite or not indexed: SF_VIS_OUTSIDE.  The window
 *   is the pixels (row + dr, (col + dc) mod W), |dr| <= half_rows, |dc| <= half_cols, rows outside [0, H) skipped.  n_hit = the
 *   pixels of the window that are not empty, r_near / r_far the smallest / largest range among them.  n_hit < min_hits:
 *   SF_VIS_UNKNOWN -- an empty pixel is no evidence, a missing return is never read as free space.  margin = range_margin +
 *   range_ratio * r.  SF_VIS_SEEN_THROUGH iff r + margin < (double)r_near (every ray near it went past it); else SF_VIS_OCCLUDED
 *   iff r - margin > (double)r_far; else SF_VIS_WITHIN.  r comes from IEEE operations and a correctly rounded sqrt, so the class
 *   depends on atan2 only through the two floors.
 * sf_map_visibility: cls [n] in the ORIGINAL point order.  sf_map_visibility_votes: seen_through[i] / within[i] = the number of the
 *   n_images images that class point i SEEN_THROUGH / WITHIN, bit for bit the counts summed over n_images single-image calls; the
 *   map is read once however many images vote.  The class counts of the statistics are sums over the images (a point the index
 *   does not hold counts as outside once per image), n_points and n_valid are the map's (sf_map_index), n_removed is 0.  poses NULL:
 *   every pose the identity.  The map's index, normals, covariances and neighbour table are left alone: a caller who wants a
 *   cleaned map keeps the map's cloud, calls sf_cloud_remove_seen_through on it and then sf_map_build.
 * sf_cloud_remove_seen_through: classifies the cloud's own points (no index is needed or built; n_valid = the finite points) and
 *   removes point i iff seen_through[i] >= min_seen && within[i] <= max_within.  Compacts in place like a crop -- the order is
 *   kept, sf_cloud_last_indices reports the survivors; votes and flags never leave the device; n_removed = the points taken away.
 * SF_ERR_INVALID, nothing touched: half_cols < 0 or half_rows < 0; 2 half_cols + 1 > W for any image; min_hits outside 1 ..
 *   (2 half_cols + 1)(2 half_rows + 1); a margin or ratio that is negative or not finite; n_images outside 1 .. 64; a NULL image
 *   or one of another context; a pose that is not finite; min_seen < 1 or max_within < 0.  A map that is not built is SF_ERR_STATE.
 *   An empty cloud is SF_OK with zero statistics.  With profile != 0, or with sf_map_profile_launches on for the map forms,
 *   device_ms = the device time from the first to the last kernel; otherwise -1. */
typedef struct sf_range_image sf_range_image;
typedef struct { int32_t width, height; double el_min, el_max, min_range, max_range; } sf_range_image_params;
typedef struct { int64_t n_points, n_projected, n_outside, n_nonfinite, n_filled; float device_ms; int32_t pad; } sf_range_image_stats;
void sf_range_image_default_params(sf_range_image_params *p);   /* 2048 x 64, -25 deg .. +3 deg in radians, 0.5 m .. 120 m */
int sf_range_image_create(sf_ctx *ctx, const sf_range_image_params *p, sf_range_image **out);
void sf_range_image_destroy(sf_range_image *img);
int sf_range_image_info(const sf_range_image *img, sf_range_image_params *p);
int sf_range_image_build(sf_range_image *img, sf_cloud *c, const double *pose /* [16] row-major, parent <- sensor, or NULL */, sf_range_image_stats *stats);
int sf_range_image_download(sf_range_image *img, float *range /* [H][W] or NULL */, int32_t *index /* [H][W] or NULL */);
#define SF_VIS_OUTSIDE 0
#define SF_VIS_UNKNOWN 1
#define SF_VIS_WITHIN 2
#define SF_VIS_OCCLUDED 3
#define SF_VIS_SEEN_THROUGH 4
typedef struct { int32_t half_cols, half_rows, min_hits, profile; double range_margin, range_ratio; } sf_visibility_params;
typedef struct { int64_t n_points, n_valid, n_outside, n_unknown, n_within, n_occluded, n_seen_through, n_removed; float device_ms; int32_t pad; } sf_visibility_stats;
void sf_visibility_default_params(sf_visibility_params *p);   /* 1, 1, 1, 0, 0.2 m, 0.01 */
int sf_map_visibility(sf_map *m, sf_range_image *img, const double *pose, const sf_visibility_params *p,
                      uint8_t *cls /* [n], original order, or NULL */, sf_visibility_stats *stats);
int sf_map_visibility_votes(sf_map *m, sf_range_image *const *imgs, const double *poses /* [B][16] */, int64_t n_images /* 1 .. 64 */,
                            const sf_visibility_params *p, uint16_t *seen_through /* [n] or NULL */, uint16_t *within /* [n] or NULL */,
                            sf_visibility_stats *stats);
int sf_cloud_remove_seen_through(sf_cloud *c, sf_range_image *const *imgs, const double *poses, int64_t n_images,
                                 const sf_visibility_params *p, int min_seen, int max_within, sf_visibility_stats *stats);
/* Scan Context place recognition over a keyframe database (extension, no reference code; Kim & Kim, IROS 2018, as used by SC-LIO-SAM
 * and SC-A-LOAM, here without the ring-key pre-filter: the search is exhaustive and exact; DESIGN §29, restated in
 * tests/place_ref_np.py).  Everything below is float64, unfused, evaluated left to right as written, unless said otherwise.
 * Descriptor.  num_rings Nr (1 .. 40), num_sectors Ns (1 .. 120), min_range, max_range (metres, horizontal), sensor_height.
 *   With a pose T [16] row-major, parent <- sensor (NULL: the identity through the same expressions): d_k = (double)p_k - T[4k+3];
 *   x = (T[0] d0 + T[4] d1) + T[8] d2, y = (T[1] d0 + T[5] d1) + T[9] d2, z = (T[2] d0 + T[6] d1) + T[10] d2.
 *   h2 = x x + y y; rho = sqrt(h2); az = atan2(y, x).  Sector: PI = the double nearest pi, u = (az + PI) / (2 PI) * Ns,
 *   col = floor(u), col - Ns when col >= Ns.  Ring: v = rho / max_range * Nr, ring = floor(v).  Height: hgt = (float)(z + sensor_height).
 *   A point with a coordinate that is not finite is n_nonfinite; else it is outside (n_outside) when min_range <= rho is false or
 *   ring >= Nr; else below (n_below) when hgt <= 0; else binned (n_binned).  Bin [ring][col] holds the maximum hgt of its binned
 *   points, float32; an empty bin is +0.  A 32-bit integer atomicMax on the bits of hgt, at most one per point (the lanes of a wave
 *   that share a bin send one): a positive float orders like its bits, so the bin holds the same bits on every run.  n_filled = the bins that are not +0; n_points = n_nonfinite + n_outside +
 *   n_below + n_binned; device_ms = the device time of the fill and the two kernels of the build.
 * Distance.  For a descriptor a: n[j] = sqrt(sum_i a[i][j]^2), i ascending, from 0; u[i][j] = a[i][j] / n[j] where n[j] > 0, else 0;
 *   column j is valid iff n[j] > 0.  For query q, entry c and shift s in 0 .. Ns - 1, over the j ascending for which q's column j and
 *   c's column jc = (j + s) mod Ns are both valid: cos_j = sum_i uq[i][j] * uc[i][jc] (i ascending, multiply then add),
 *   S = S + cos_j, V = V + 1.  d(s) = 1 - S / V, or exactly 1 when V = 0.  D(q, c) = min_s d(s); shift(q, c) = the smallest s that
 *   attains it.  If the query's sensor stands where the entry's stood and is turned by +psi about z, shift * 2 PI / Ns ~ psi: the
 *   candidate pose of a match is T_entry . Rz(shift * (2 PI / Ns)), computed on the host in float64.
 * Top-k.  The k (1 .. 32) entries with the smallest (D, index); slots beyond the database size get index -1, D = +inf, shift 0 and
 *   an all-zero pose.
 * Database.  sf_place_db_add_cloud builds the descriptor on the device and appends it without a host round trip (entry_pose NULL:
 *   the identity); sf_place_db_add_descriptors appends stored rows (poses NULL: identities); the unit columns of an entry are
 *   computed once, at insertion.  The capacity doubles as the database grows and what it held is carried over; sf_place_db_clear
 *   empties it.  sf_place_db_download: cap >= n rows, *n = n (SF_ERR_INVALID when cap is too small, *n set); desc and poses may each
 *   be NULL.  sf_place_db_distances gives D and shift of every pair; sf_place_db_query the top-k per query with the candidate poses
 *   (poses may be NULL); sf_place_db_query_cloud does the same for one cloud whose descriptor never leaves the device.  An empty
 *   database is valid: distances have zero columns and every top-k slot is empty.  match_ms / select_ms: the device time of the
 *   match (the queries' unit columns included) and of the selection.
 * SF_ERR_INVALID, nothing touched: num_rings outside 1 .. 40 or num_sectors outside 1 .. 120; ranges or a height that are not
 *   finite, min_range < 0 or max_range <= min_range; a pose that is not finite; a cloud of another context or with 2^31 points or
 *   more; a descriptor given by the host (an entry or a query) that holds a negative or non-finite value; Q outside 1 .. 64; k
 *   outside 1 .. 32. */
typedef struct { int32_t num_rings, num_sectors; double min_range, max_range, sensor_height; } sf_place_params;
typedef struct { int64_t n_points, n_nonfinite, n_outside, n_below, n_binned, n_filled; float device_ms; int32_t pad; } sf_place_stats;
typedef struct { int64_t n_queries, n_entries; float match_ms, select_ms; } sf_place_match_stats;
void sf_place_default_params(sf_place_params *p);   /* 20 x 60, 0.5 m .. 80 m, sensor 2 m above the ground */
int sf_cloud_scan_context(sf_cloud *c, const double *pose /* [16] or NULL */, const sf_place_params *p, float *desc /* [Nr][Ns] or NULL */, sf_place_stats *stats);
typedef struct sf_place_db sf_place_db;
int sf_place_db_create(sf_ctx *ctx, const sf_place_params *p, sf_place_db **out);
void sf_place_db_destroy(sf_place_db *db);
int sf_place_db_info(const sf_place_db *db, sf_place_params *p, int64_t *n_entries);
int sf_place_db_clear(sf_place_db *db);
int sf_place_db_add_cloud(sf_place_db *db, sf_cloud *c, const double *pose, const double *entry_pose /* [16] */, int64_t *index, sf_place_stats *stats);
int sf_place_db_add_descriptors(sf_place_db *db, const float *desc /* [n][Nr][Ns] */, const double *poses /* [n][16] */, int64_t n);
int sf_place_db_download(sf_place_db *db, float *desc, double *poses, int64_t cap, int64_t *n);
int sf_place_db_distances(sf_place_db *db, const float *queries /* [Q][Nr][Ns] */, int64_t Q /* 1 .. 64 */, double *dist /* [Q][N] */, int32_t *shift /* [Q][N] */,
                          sf_place_match_stats *stats);
int sf_place_db_query(sf_place_db *db, const float *queries, int64_t Q, int k /* 1 .. 32 */, int32_t *idx /* [Q][k] */, double *dist /* [Q][k] */,
                      int32_t *shift /* [Q][k] */, double *poses /* [Q][k][16] or NULL */, sf_place_match_stats *stats);
int sf_place_db_query_cloud(sf_place_db *db, sf_cloud *c, const double *pose, int k, int32_t *idx /* [k] */, double *dist, int32_t *shift,
                            double *poses /* [k][16] or NULL */, sf_place_match_stats *stats, sf_place_stats *build_stats /* or NULL */);
/* measurement (tools/knn_bench.py, tools/outlier_bench.py, tools/cluster_bench.py): with the switch on, sf_map_nn, sf_map_knn,
 * sf_map_estimate_normals[_cov|_knn], sf_map_*_outliers and sf_map_cluster_* record device events around their kernel launches (not
 * the copies); sf_map_last_launch_ms reads the latest (SF_ERR_STATE if there is none). */
int sf_map_profile_launches(sf_map *m, int on);
int sf_map_last_launch_ms(sf_map *m, float *ms);
/* Neighbour table: per indexed point one 32-byte entry -- the sorted positions of its up to 7 nearest other points
 * (within just under one cell, among the 27 cells around its own) and a radius inside which there is no further point.  The
 * launch list of O3D_P2P / P2PLANE alignments (neighbour reuse on, no window, unsharded, no robust kernel) consults it when a
 * cached neighbour no longer certifies: the answer is the full search's, bit for bit, or the lane searches as before.
 * sf_map_build_neighbour_table builds it now (kept until sf_map_build / sf_map_patch move the points; a normals pass keeps it).
 * sf_map_set_neighbour_table: 0 never consulted, 2 always (an alignment builds a missing one first), 1 (default) auto: a table
 * at hand is consulted; a missing one is built only for a batch of at least 700 000 queries against a map that has not been
 * rebuilt or patched since it first served an alignment -- the owner of a growing map builds it when that is worthwhile.
 * sf_map_neighbour_table_info: out = {present, entries, bytes, device time of the last build in whole ms (rounded up; -1 unless
 * sf_map_profile_launches was on)}. */
int sf_map_build_neighbour_table(sf_map *m);
int sf_map_set_neighbour_table(sf_map *m, int mode);
int sf_map_neighbour_table_info(sf_map *m, int64_t out[4]);
/* the table as it lies on the device (parity tests): [n][8] uint32 -- seven sorted positions (0xffffffff: none), the radius's float bits */
int sf_map_download_neighbour_table(sf_map *m, uint32_t *table, int64_t cap_entries, int64_t *n);
/* test entry of the table look-up alone: query i starts from the indexed point at SORTED position seed_pos[i] (as
 * sf_map_download_index lists them; negative or out of range: no seed).  served[i] = 1: idx / d2 are sf_map_nn's answer, bit for
 * bit; served[i] = 0: undecided (idx = -1, d2 = +inf).  Needs a table and no window. */
int sf_map_nn_seeded(sf_map *m, const float *queries, int64_t n, const int32_t *seed_pos, float max_d2, int32_t *idx, float *d2, uint8_t *served);
/* Stage 0 of the look-up: behind the table lies one float per indexed point, its nearest gap g1 -- the distance to the nearest
 * other point, rounded down (the table's cap when nothing is listed, 0 for a coincident twin).  A query within g1 / 2 of its
 * cached neighbour is settled by that one value: the neighbour is still the exact nearest and g1 less the query's distance
 * bounds the runner-up.  sf_map_download_nearest_gap: [n] float32 in sorted order (parity tests).  sf_map_nn_seeded_stages:
 * sf_map_nn_seeded with stage[i] = 0 not served, 1 settled by the gap alone, 2 by the table, and lb2[i] the squared runner-up
 * bound a served query leaves (0 where not served). */
int sf_map_download_nearest_gap(sf_map *m, float *gap, int64_t cap_entries, int64_t *n);
int sf_map_nn_seeded_stages(sf_map *m, const float *queries, int64_t n, const int32_t *seed_pos, float max_d2, int32_t *idx, float *d2, uint8_t *stage, float *lb2);

/* ------------------------------------------------------------------ ICP */
/* a13: ICPResult — icp_point_to_point.h:28-39 (+ float64 and diagnostics) */
typedef struct {
    float T[16];        /* transformation (row-major)                               */
    float error;        /* ref_cpp: last_error_ ; o3d/p2plane: inlier_rmse           */
    int32_t iterations; /* steps applied                                             */
    int32_t converged;  /* has_converged                                             */
    int32_t n_corr;     /* correspondences of the last search                        */
    int32_t n_research; /* correspondence searches performed                         */
    int32_t flags;      /* SF_ICP_FLAG_*                                             */
    double fitness;     /* o3d/p2plane: n_corr / n_source                            */
    double rmse;        /* o3d/p2plane                                               */
    double T64[16];     /* same transformation before rounding to float             */
} sf_icp_result;
#define SF_ICP_FLAG_FEW_CORR 1   /* < 10 correspondences: reference returns the initial T */
#define SF_ICP_FLAG_SINGULAR 2   /* p2plane normal equations not positive definite       */
#define SF_ICP_FLAG_BARRIER_TIMEOUT 8 /* internal: a grid barrier of the single-launch REF_CPP form gave up; sf_icp_fetch_results turns it into SF_ERR_HIP */
#define SF_ICP_FLAG_SHARD_STALE 4 /* sharded stepping: the scan moved out of the margin of this rank's owned-query arrays and stopped; resume with sf_icp_step_begin(first = 2) */

/* modes: REF_CPP = ICPPointToPoint::calculateAlignment (icp_point_to_point.cpp:185-254,
 * lazy re-search, d2 < max_correspondence_dist quirk of :70);  O3D_P2P = Open3D
 * registration_icp point-to-point as called at localization_node.py:233-237;
 * P2PLANE = extension x1, Gauss-Newton, exactly num_iterations iterations. */
#define SF_ICP_REF_CPP 0
#define SF_ICP_O3D_P2P 1
#define SF_ICP_P2PLANE 2

/* ctor — icp_point_to_point.h:49 / icp_point_to_point.cpp:3-12 */
int sf_icp_create(sf_ctx *ctx, float max_correspondence_dist, int num_iterations,
                  float acceptable_mean_error, float transformation_epsilon, sf_icp **out);
void sf_icp_destroy(sf_icp *icp);
/* setters — icp_point_to_point.cpp:14-42 */
int sf_icp_set_max_correspondence_dist(sf_icp *icp, float v);
int sf_icp_set_num_iterations(sf_icp *icp, int v);
int sf_icp_set_transformation_epsilon(sf_icp *icp, float v);
int sf_icp_set_acceptable_mean_error(sf_icp *icp, float v);
int sf_icp_set_initial_transformation(sf_icp *icp, const float T[16]);
int sf_icp_set_initial_transformation_f64(sf_icp *icp, const double T[16]);
int sf_icp_set_debug_mode(sf_icp *icp, int on);
/* setSourcePointCloud — icp_point_to_point.cpp:44-47 (copies; caller keeps its cloud) */
int sf_icp_set_source(sf_icp *icp, const float *xyz, int64_t n);
int sf_icp_set_source_cloud(sf_icp *icp, sf_cloud *cloud);
/* The node's scan preprocessing and setSourcePointCloud in one pass, without a host synchronisation
 * (localization_node.cpp:290-297,333): the source becomes every stride-th point of `raw` that is finite and within `radius`
 * of `center`, in index order -- exactly sf_cloud_subsample(stride) + sf_cloud_crop_radius(center, radius, 0) +
 * sf_icp_set_source_cloud, same predicates, same points.  `raw` is left untouched; the count stays on the device, so the
 * source serves unsharded single-scan REF_CPP alignments only.  sf_icp_source_count: the number of points the last fetched
 * single-scan REF_CPP alignment ran on. */
int sf_icp_set_source_scan(sf_icp *icp, sf_cloud *raw, int stride, const float center[3], double radius);
int sf_icp_source_count(sf_icp *icp, int64_t *n);
/* setTargetPointCloud — icp_point_to_point.cpp:49-55: either index a cloud privately
 * (reference semantics) or share a prebuilt whole-map index (no copy, no rebuild). */
int sf_icp_set_target(sf_icp *icp, const float *xyz, int64_t n);
int sf_icp_set_target_map(sf_icp *icp, sf_map *map);
/* calculateAlignment — icp_point_to_point.cpp:185-254 */
int sf_icp_align(sf_icp *icp, int mode, sf_icp_result *out);

/* batched throughput form: `batch` scans of n_per_scan points each (xyz contiguous,
 * scan-major), one initial transform per scan (inits = batch*16 doubles, NULL = identity),
 * all registered concurrently against the same target map in ONE kernel sequence.
 * Lifetime of `xyz` (pinned memory: the copy is asynchronous): with the pipeline on (sf_icp_set_pipeline), a host buffer set
 * while an alignment is unfetched is read on an internal stream, not on the context's -- synchronising the context's stream
 * does not mean it has been consumed -- and it is free again only once that batch's alignment has been fetched
 * (sf_icp_fetch_results / sf_icp_fetch_previous).  A streaming loop therefore takes two host buffers in turn.  Otherwise
 * (nothing unfetched, pipeline off) the copy is ordered on the context's stream.
 * A source set ahead in this way is adopted by whichever alignment comes next, also a stepped or a sharded one
 * (sf_icp_step_begin with first != 0, sf_icp_align_sharded*, sf_icp_align_group): it waits for the upload and sizes its
 * buffers for the new batch. */
int sf_icp_set_source_batch(sf_icp *icp, const float *xyz, int64_t n_per_scan, int batch);
int sf_icp_set_source_batch_device(sf_icp *icp, const void *d_xyz, int64_t n_per_scan, int batch);
int sf_icp_set_initial_batch_f64(sf_icp *icp, const double *inits);
int sf_icp_align_batch(sf_icp *icp, int mode, sf_icp_result *out /* batch entries */);
/* enqueue only (no host sync); results fetched later.  sf_icp_fetch_results returns the LATEST enqueued alignment as it
 * was enqueued (`out`: as many entries as ITS batch) -- a source or priors set since belong to the next alignment. */
int sf_icp_align_batch_async(sf_icp *icp, int mode);
int sf_icp_fetch_results(sf_icp *icp, sf_icp_result *out);
/* The results of the alignment enqueued BEFORE the latest one, when the two ran side by side (two
 * sf_icp_align_batch_async calls with no fetch between them, sf_icp_set_pipeline on, launch list): waits for that
 * alignment only, the latest one goes on running.  The streaming loop is "set the next batch, enqueue its alignment,
 * fetch the previous one's result": every result reaches the host and the device never drains.  `out`: as many
 * entries as THAT alignment's batch.  SF_ERR_STATE when there is nothing to fetch: the latest alignment did not run
 * beside its predecessor (a fetch in between, pipeline off, a single-launch or profiled alignment) -- then the
 * predecessor's states have been overwritten -- or the call was made already.  No reference counterpart (one scan per
 * callback, localization_node.cpp:337). */
int sf_icp_fetch_previous(sf_icp *icp, sf_icp_result *out);
int sf_icp_use_graph(sf_icp *icp, int on); /* replay the launch sequence as a hipGraph */
/* how often the launch sequence was captured / launched as a graph since creation (a capture per alignment means the
 * cache key keeps changing).  REF_CPP with ONE scan reads the scan's point count and the map window from device memory,
 * so scans of similar size (same count rounded up to 4096) and a moving window replay the same graph. */
int sf_icp_graph_counts(sf_icp *icp, int64_t *captures, int64_t *launches);
/* Alignments small enough for every workgroup to be resident at once (the nodes' per-scan paths: ~13 k points; on MI355X
 * up to 65 k points in REF_CPP and O3D_P2P, 131 k in P2PLANE, summed over the batch -- from the occupancy query, minus one
 * workgroup per CU) run as ONE launch -- search, record,
 * controller / solve and step behind in-kernel grid barriers (REF_CPP: icp_point_to_point.cpp:185-254), bit-identical to
 * the launch list; on by default, larger alignments, sharded and profiled ones take the launch list.
 * sf_icp_fused_count: how many alignments have taken the single-launch form since creation. */
int sf_icp_set_fused(sf_icp *icp, int on);
int sf_icp_fused_count(sf_icp *icp, int64_t *launches);
/* Residency of a single-launch grid is kept by a per-device ledger of the grids in flight (all contexts of the process);
 * an alignment that does not fit takes the launch list.  Should a grid barrier still give up (another PROCESS holding the
 * compute units), the alignment is redone through the launch list inside sf_icp_fetch_results and the object stays on
 * the launch list: sf_icp_fused_redone counts how often that happened.  The redo aligns what was enqueued -- that
 * alignment's source, priors and mode -- also when the next batch's source and priors have been set since (pipeline on: the
 * two source sets); with the pipeline off a source set since has replaced it in place, and the fetch returns SF_ERR_STATE. */
int sf_icp_fused_redone(sf_icp *icp, int64_t *redone);
int sf_icp_test_inject_barrier_timeout(sf_icp *icp); /* test hook: treat the next single-launch alignment as timed out (exercises the redo) */
/* Order in which the points of a scan are walked by O3D_P2P / P2PLANE.  The correspondences and
 * every per-point term are independent of it; only the rounding of the record sums changes
 * (deterministically for a given order).  CELL sorts each scan by the map-grid cell of its points
 * under the initial pose at the start of every alignment (on the device, inside sf_icp_align*), so
 * that scans in flight share map lines in L2; AUTO = CELL when scans x points >= 300 000. */
#define SF_ORDER_AUTO 0
#define SF_ORDER_AS_GIVEN 1
#define SF_ORDER_CELL 2
int sf_icp_set_query_order(sf_icp *icp, int order);
/* Neighbour reuse (default on, O3D_P2P / P2PLANE).  Every full search also proves a lower bound on
 * the distance from the query to every map point other than its neighbour; in a later iteration a
 * query that has moved by less than the slack of that bound provably keeps its neighbour, and its
 * search is skipped.  Results are bit-identical with the switch on or off (tested); it only
 * changes how much of the "nearest neighbour every iteration" work has to be redone. */
int sf_icp_set_nn_reuse(sf_icp *icp, int on);
/* Scans above `points` points (at most 131 072: what the single-launch kernels can take) are registered through the launch list with
 * two queries per lane -- the form the frozen pairs need.  Without a call the rule is: above 131 072 points always; above 65 536 when
 * the batch has more rows than any single-launch kernel keeps resident (so no alignment of that shape could run as one launch:
 * nothing to stay bit-compatible with) -- a full 64-ring scan (<= 130 048 returns) registered in a batch is wide and may freeze,
 * registered alone it is not.  A call makes `points` the whole rule.  The limit is part of the summation order: results on either
 * side of it agree to float64 rounding, not bitwise. */
int sf_icp_set_wide_scan_points(sf_icp *icp, int64_t points);
/* Consecutive sf_icp_align_batch_async calls on unchanged inputs (source, initial poses, target) overlap: a launch list
 * enqueued while an earlier alignment of this object has not been fetched yet runs on an internal stream with its own copy of
 * everything an alignment writes, so an alignment's last launches (with frozen pairs: a chain of 16 us kernels on an idle
 * device) run under the next one's searching launches.  The context's stream waits for every such alignment as soon as it is
 * enqueued: a fetch, an upload or a map rebuild issued afterwards is ordered behind it exactly as before, and a changed input
 * makes the next alignment wait for everything before it.  A caller that fetches each result before the next alignment never
 * leaves the context's stream.  Results are those of the same alignment run alone (same kernels, same data; tested bitwise).
 * A source set FROM HOST MEMORY (sf_icp_set_source_batch / sf_icp_set_source) while an alignment is unfetched does not wait
 * for it either: the object keeps two source sets, the upload and its conversion take the one the alignment in flight does
 * not read, on the stream the next alignment will run on -- the streaming loop "set the next batch, enqueue its alignment,
 * sf_icp_fetch_previous" uploads batch k+1 beside the alignment of batch k (measured: +41 % over the same loop with the
 * upload behind the alignment; profiles/LADDER.md).  Sources handed over as DEVICE pointers or clouds stay on the context's
 * stream, behind whatever produced them.
 * on: 1 (default) / 0 = every alignment on the context's stream.  No reference counterpart (one scan at a time,
 * localization_node.cpp:337). */
int sf_icp_set_pipeline(sf_icp *icp, int on);
/* Tile search (O3D_P2P / P2PLANE launch list, scans above 131 072 points, whole map, unsharded, queries ordered): the
 * launches of an alignment in which nearly every query searches -- the first four with the neighbour reuse on, all of them
 * with it off -- run tile by tile: the scans' queries are sorted by map tile (a box of grid cells), one workgroup stages a
 * tile's points and cell table in LDS and serves every query of every scan that falls into it from there; the pairs go
 * through the neighbour cache and are summed in the usual order.  The exact search of icp_point_to_point.cpp:64-69 /
 * localization_node.py:233-237, the same pairs and bit-identical sums as without (tested); what changes is that a
 * candidate is an LDS read instead of a 16-byte access through the L1.  mode: 0 never, 1 (default) when the batch holds at
 * least 2 M queries, 2 whenever the conditions above hold. */
int sf_icp_set_tile_search(sf_icp *icp, int mode);
/* out[0] = the last alignment used tile search; [1..3] cells per tile (x, y, z); [4..6] tiles per axis; with
 * sf_icp_profile_enable: [7] queries that searched in the tile launches, [8] settled out of LDS, [9] walked the global
 * index because they had left the staged region, [10] went on to ring 2 and beyond, [11] tiles too dense to stage */
int sf_icp_tile_info(sf_icp *icp, int64_t out[12]);
/* Frozen pairs (P2PLANE launch list, scans above 131 072 points, neighbour reuse on, whole map, unsharded): once a scan's
 * pairs are certified to stay as they are while it moves by a guard distance more, one launch forms the 96 moments of
 * those pairs and the iterations after it evaluate the normal equations from the moments (a polynomial in the pose)
 * instead of streaming the scan; queries too close to a change stay "active" and are evaluated launch by launch.
 * Same pairs, same float64 sums up to summation rounding (~1e-13 of a pose).  on: 0 never, 1 (default) when the batch holds
 * at least 0.7 M queries -- a frozen launch costs a fixed latency whatever the batch, a small batch is faster
 * without --, 2 always.  No reference counterpart (the reference searches every point in every iteration,
 * icp_point_to_point.cpp:64-69).  While a robust kernel is set (sf_icp_set_robust_kernel) P2PLANE never freezes, whatever
 * `on` says: the moment polynomial assumes unit weights. */
int sf_icp_set_freeze(sf_icp *icp, int on);
/* guard = max(guard_scale x motion of the last pose update, guard_min) [m]; a freeze launch is asked for once that is at most
 * guard_max (a larger guard means long active lists), at most max_tries times per alignment, from launch index
 * from_launch (>= 4) on.  Defaults 8, 2e-5, 3e-4, 3, 5. */
int sf_icp_set_freeze_params(sf_icp *icp, float guard_scale, float guard_min, float guard_max, int max_tries, int from_launch);
/* of the last batched alignment, summed over its scans: {freeze launches that held, thaws (moved beyond the guard),
 * freeze launches that did not hold, active queries of the last freeze launch, scans frozen at the end} */
int sf_icp_freeze_stats(sf_icp *icp, int64_t out[5]);
/* Deferred search (frozen-pairs schedule only, unsharded): in the last verifying launch before the first chance to freeze
 * (from_launch >= 5) a wave in which up to 8 queries fail their certificate lists them instead of searching in place, and a
 * dense pass behind the launch searches the listed queries 64 per wave.  Same pairs; their terms enter the sums at another
 * place (the schedule's results agree with the switch off to summation rounding, as frozen pairs on / off do).  on: 0 / 1
 * (default 1), an A/B switch like sf_icp_set_freeze. */
int sf_icp_set_defer_search(sf_icp *icp, int on);
/* of the last batched alignment: {queries that went to the dense pass, waves with more failing queries than the cap, which
 * searched in place} -- zeros when the schedule did not run or the switch is off.  Whether it ran is recorded when the
 * alignment is enqueued: a later sf_icp_fetch_results that re-learns the freeze schedule does not change the answer.
 * An alignment that consults a neighbour table has several deferring launches (sf_icp_lookup_launch_stats): the two
 * numbers are then the sums over all of them. */
int sf_icp_defer_stats(sf_icp *icp, int64_t out[2]);
/* Look-up launches.  An alignment on the frozen-pairs schedule with the deferred search on that consults a neighbour table
 * (unsharded, whole map) runs every launch from the first that consults the table (sf_icp_set_neighbour_research) up to the
 * launch before from_launch (sf_icp_set_freeze_params) in the deferring form: two queries per lane, table and nearest gap
 * first, the few queries they leave to the dense pass.  Same pairs as the searching launches they replace; their terms enter
 * the float64 sums at another place.  Without a table the schedule is unchanged.  While from_launch is left to the library the
 * first look-up launch of the NEXT alignment is learnt like from_launch itself (sf_icp_fetch_results): a look-up launch in which
 * more than one wave in eight exceeded the cap moves it behind that launch; sf_icp_set_freeze_params and
 * sf_icp_set_neighbour_research start over.  Of the last batched alignment, as recorded
 * when it was enqueued: {launches that ran in look-up form, queries they deferred, their capped waves, the index of the first
 * of them (-1: none)}. */
int sf_icp_lookup_launch_stats(sf_icp *icp, int64_t out[4]);
/* The first launch index (>= 1; default 2, the third launch) of an alignment from which lanes consult the map's neighbour
 * table (sf_map_set_neighbour_table); negative: never.  Earlier launches move the pose too far for the table to serve many. */
int sf_icp_set_neighbour_research(sf_icp *icp, int from_launch);
/* of the last alignment enqueued, in profiled runs (sf_icp_profile_enable): {queries the table served, queries it was tried for
 * and did not serve, waves that still searched}.  A wave of the deferring launch that holds more failing queries than the cap
 * looks its unserved queries up a second time and counts them twice.  SF_ERR_STATE when profiling is off or its counters are
 * full (1024 launches since sf_icp_profile_enable; enabling again resets them). */
int sf_icp_neighbour_stats(sf_icp *icp, int64_t out[3]);
/* the same three and, fourth, how many of the served queries the nearest gap alone settled (sf_map_download_nearest_gap) */
int sf_icp_neighbour_gap_stats(sf_icp *icp, int64_t out[4]);
/* Robust M-estimator kernel of SF_ICP_P2PLANE (REF_CPP and O3D_P2P ignore it, as Open3D's point-to-point estimator takes no
 * kernel).  With r = (y - p) . n the float64 point-to-plane residual of a pair (y the transformed source point, p / n the
 * neighbour and its normal) and the scale k > 0 in metres, every pair enters the normal equations with the weight w(r):
 *   SF_ROBUST_NONE    1 (default: the unweighted path, unchanged)
 *   SF_ROBUST_HUBER   1 if |r| <= k, else k / |r|
 *   SF_ROBUST_CAUCHY  1 / (1 + (r/k)^2)
 *   SF_ROBUST_TUKEY   (1 - (r/k)^2)^2 if |r| <= k, else 0
 *   SF_ROBUST_GM      (k^2 / (k^2 + r^2))^2   (Geman-McClure with k in metres; Open3D's GMLoss takes k in m^2: not equal)
 * The Huber, Cauchy and Tukey forms are meant to be those of Open3D's TransformationEstimationPointToPlane(kernel); that
 * parity has not been checked against Open3D itself.  The JtJ and Jtr sums are weighted (sum w J J^T, sum w J r, w formed
 * in float64); the correspondence count, sum r^2 and sum d^2 are not, so fitness, rmse and n_corr keep their meaning.  A
 * weighted system that is not positive definite (Tukey zeroing too many pairs) sets SF_ICP_FLAG_SINGULAR and stops that
 * scan.  Correspondences do not depend on the kernel (the neighbour reuse is unaffected).  The setting is read when an
 * alignment is enqueued and travels with it (two unfetched alignments keep their own; a captured graph is re-captured when
 * it changes).  While a kind other than NONE is set, P2PLANE does not freeze (sf_icp_set_freeze) and does not take the tile
 * search (sf_icp_set_tile_search); the single-launch form and the sharded paths carry the weights.
 * SF_ERR_INVALID (setting unchanged) for an unknown kind, or for a k that is not finite or <= 0 while kind != NONE. */
#define SF_ROBUST_NONE 0
#define SF_ROBUST_HUBER 1
#define SF_ROBUST_CAUCHY 2
#define SF_ROBUST_TUKEY 3
#define SF_ROBUST_GM 4
int sf_icp_set_robust_kernel(sf_icp *icp, int kind, double k);

/* Pose covariance and degeneracy of an alignment.  With the switch on (sf_icp_set_covariance; default off) every alignment
 * enqueues, behind its last iteration and on the same stream / lane, ONE more evaluation of the objective it minimised, at
 * the pose it ended at (the T64 of its result), with its own source, target, max_correspondence_dist, mode and robust
 * kernel.  No solve changes; an object that never touches the switch computes what it always did.
 *   Pairs: for every source point s_i = T x_i (float64) its exact nearest map point q_i (normal n_i) -- a fresh search at
 *     the FINAL pose, on the float32 rounding of s_i like every search of this library, whole map or the attached window
 *     -- accepted by the mode's own predicate (REF_CPP: d2 < max_correspondence_dist un-squared, as the reference compares;
 *     O3D_P2P / P2PLANE: d2 < max_correspondence_dist^2).
 *   Perturbation: T' = Exp(w, t) T, vector order (wx wy wz tx ty tz), map frame -- the convention of the Gauss-Newton step.
 *   P2PLANE: r_i = n_i . (s_i - q_i), J_i = [s_i x n_i, n_i], w_i = the robust weight of r_i (1 without a kernel);
 *     H = sum w_i J_i^T J_i, chi2 = sum w_i r_i^2, W = sum w_i, dof = W - 6.
 *   REF_CPP / O3D_P2P: r_i = s_i - q_i, J_i = [-[s_i]x, I], unit weights; H = sum J_i^T J_i (formed in closed form from n,
 *     sum s, sum s s^T), chi2 = sum |r_i|^2, W = n_corr, dof = 3 n_corr - 6.
 *   sigma2_hat = chi2 / dof (0 when dof <= 0); sigma2 = sensor_sigma^2 when a sensor sigma > 0 was set, else sigma2_hat.
 *   H = V diag(lambda) V^T (cyclic Jacobi, float64); cov = sigma2 V diag(1 / max(lambda_k, SF_COV_EIG_EPS lambda_max)) V^T:
 *     always finite, symmetric, positive semi-definite.  Any lambda_k <= SF_COV_EIG_EPS lambda_max sets SF_COV_SINGULAR.
 *     Fewer than 10 pairs (the reference's own floor) set SF_COV_FEW_CORR; info, cov and the degeneracy fields are zero then.
 *   Degeneracy: the marginal information of the translation, S_t = H_tt - H_tr H_rr^-1 H_rt, and of the rotation,
 *     S_r = H_rr - H_rt H_tt^-1 H_tr (formed as the inverses of the diagonal blocks of cov / sigma2, so they stay finite
 *     when H is singular): eigenvalues ascending, DIVIDED BY W, with their eigenvectors as rows.  For P2PLANE
 *     trace(H_tt) = W, so the smallest normalised translation eigenvalue lies in [0, 1/3] whatever the scan size.
 *     sf_icp_set_degeneracy_thresholds(trans, rot, inflate_trans_var, inflate_rot_var) (defaults 0 = never) sets
 *     SF_COV_DEGENERATE_TRANS / _ROT when a normalised eigenvalue is below its threshold and adds, for EVERY flagged
 *     eigenvector v, inflate * u u^T to cov (u = v embedded in the 6-vector); info stays the pure H.
 * This is the Hessian (Gauss-Newton / Cramer-Rao style) covariance: it models sensor noise on CORRECT pairs.  It knows
 * nothing of wrong data association nor of the bias of a sampled map, and where the geometry barely constrains a direction
 * (a tunnel's axis) the noise of the map normals still leaves a little information per pair, which over thousands of pairs
 * claims millimetres where the pose is decimetres off.  That is the known weakness of Hessian covariances, and why
 * LOAM-style stacks threshold eigenvalues instead: let the FLAG (and the inflation), not the magnitude of cov, decide.
 * The settings are read when an alignment is enqueued and travel with it (part of a captured graph's key).
 * sf_icp_fetch_covariance: the covariances of the alignment sf_icp_fetch_results last returned (call it first; batch
 * entries); sf_icp_fetch_covariance_previous: of the alignment sf_icp_fetch_previous returns (callable before or after it,
 * once).  SF_ERR_STATE when that alignment ran with the switch off, or there is none.  Sharded / stepping alignments
 * (sf_icp_set_shard, sf_icp_step_*, sf_icp_align_sharded*, sf_icp_align_group) decline: SF_ERR_STATE while the switch is on.
 * SF_ERR_INVALID: NULL arguments, a negative or non-finite sigma, threshold or inflation. */
#define SF_COV_EIG_EPS 1e-12
#define SF_COV_FEW_CORR 1
#define SF_COV_SINGULAR 2
#define SF_COV_DEGENERATE_TRANS 4
#define SF_COV_DEGENERATE_ROT 8
typedef struct {
    double info[36];        /* H, row-major, order (wx wy wz tx ty tz) */
    double cov[36];
    double sigma2, sigma2_hat, weight_sum;
    double trans_info[3], trans_dir[9];   /* ascending, / weight_sum; eigenvectors as rows */
    double rot_info[3], rot_dir[9];
    int64_t n_corr;
    int32_t flags;          /* SF_COV_* */
} sf_icp_covariance;
int sf_icp_set_covariance(sf_icp *icp, int on, double sensor_sigma);
int sf_icp_set_degeneracy_thresholds(sf_icp *icp, double trans, double rot, double inflate_trans_var, double inflate_rot_var);
int sf_icp_fetch_covariance(sf_icp *icp, sf_icp_covariance *out);
int sf_icp_fetch_covariance_previous(sf_icp *icp, sf_icp_covariance *out);

/* multi-GPU (map tile-sharded along x with halo): this rank only
 * accumulates queries whose TRANSFORMED x lies in [x_lo, x_hi); per iteration
 *   sf_icp_step_begin  -> NN + partial normal equations into the exchange buffer
 *   (caller all-reduces sf_icp_exchange_ptr over RCCL on sf_ctx_stream)
 *   sf_icp_step_end    -> identical solve on every rank
 * first = 1 starts an alignment (state <- initial transforms; sharded: this rank's owned-query
 * candidates are compacted, cell-ordered and gathered -- one host synchronisation), first = 0 is
 * the next iteration.  Sharded: a scan whose points move close to the margin (1 m) of those arrays
 * stops with SF_ICP_FLAG_SHARD_STALE (same decision on every rank); after the loop the caller
 * fetches the results and, if any scan carries the flag, calls sf_icp_step_begin(first = 2) --
 * rebuild at the current poses, flag cleared -- and runs the remaining iterations. */
int sf_icp_set_shard(sf_icp *icp, float x_lo, float x_hi);
int sf_icp_set_shard_margin(sf_icp *icp, float margin_m); /* default 1 m: how far a scan may move before its owned-query arrays are rebuilt */
int sf_icp_set_exchange_buffer(sf_icp *icp, void *d_buf, int64_t nbytes); /* optional: caller-owned (torch tensor) */
void *sf_icp_exchange_ptr(sf_icp *icp, int64_t *nbytes);
int sf_icp_step_begin(sf_icp *icp, int mode, int first);
int sf_icp_step_end(sf_icp *icp, int mode, int last);

/* The same loop driven from the C side (no host work between iterations).  sf_comm is an RCCL communicator bound to a
 * context's stream; RCCL is resolved at run time (sf_comm_load_rccl: path of the library the process must share, NULL =
 * the already loaded one or librccl.so.1).  Rank 0 draws sf_comm_unique_id (128 bytes), the launcher (torch.distributed,
 * MPI, a file) hands it to every rank, each rank calls sf_comm_create. */
typedef struct sf_comm sf_comm;
int sf_comm_load_rccl(const char *library_path);
int sf_comm_unique_id(void *id128);
int sf_comm_create(sf_ctx *ctx, int nranks, int rank, const void *id128, sf_comm **out);
void sf_comm_destroy(sf_comm *c);
int sf_comm_size(const sf_comm *c, int *nranks, int *rank);
int sf_comm_allreduce_f64(sf_comm *c, void *d_buf, int64_t count); /* in place, on the context's stream (barriers, timing) */
/* The second transport (SURVEY.md §8e option ii): a hand-written P2P all-gather + fixed-rank-order sum.  Every rank keeps an
 * exchange region in its device memory, exports it (hipIpc) and maps its peers'; an all-reduce is ONE single-workgroup
 * kernel on the context's stream that stores the rank's doubles into every region, raises a flag there, waits for the
 * peers' flags (bounded) and adds the nranks slots in rank order -- bitwise identical on every rank and run to run, a few
 * microseconds over xGMI, and the only transport that runs 2-4 ranks as separate processes on ONE device.
 *   sf_comm_p2p_create     this rank's region; max_count = largest all-reduce in doubles (32 x scans in flight)
 *   sf_comm_p2p_handle     -> SF_COMM_P2P_HANDLE_BYTES the launcher hands to every rank (torch.distributed, MPI, a file)
 *   sf_comm_p2p_connect    <- the nranks handles in rank order
 *   sf_comm_p2p_rendezvous handle + connect through a POSIX shared-memory object `name` (ranks of one node, no launcher)
 * A rank whose wait runs out (sf_comm_set_timeout, default 20 s) or that meets an abort raises the abort word of every
 * region: all ranks leave their collectives and sf_comm_status / sf_icp_align_sharded return SF_ERR_COMM -- nobody is
 * left waiting in a collective.  sf_comm_abort does that from the host (RCCL: ncclCommAbort). */
#define SF_COMM_RCCL 0
#define SF_COMM_P2P 1
#define SF_COMM_P2P_HANDLE_BYTES 128
int sf_comm_p2p_create(sf_ctx *ctx, int nranks, int rank, int64_t max_count, sf_comm **out);
int sf_comm_p2p_handle(sf_comm *c, void *handle);
int sf_comm_p2p_connect(sf_comm *c, const void *handles);
int sf_comm_p2p_rendezvous(sf_comm *c, const char *name, double timeout_s);
int sf_comm_set_timeout(sf_comm *c, double seconds);
int sf_comm_abort(sf_comm *c);
int sf_comm_status(sf_comm *c);
int sf_comm_kind(const sf_comm *c);
/* one whole pass (every iteration) enqueued; first = 1 start, 2 resume the scans that stopped stale */
int sf_icp_align_sharded_async(sf_icp *icp, int mode, sf_comm *comm, int first);
/* blocking: passes until no scan is stale (identical decisions on every rank), results like sf_icp_align_batch */
int sf_icp_align_sharded(sf_icp *icp, int mode, sf_comm *comm, sf_icp_result *out, int *resumes /* or NULL */);
/* several slabs held by ONE process on one device and context (members[m]: slab m + halo indexed, sf_icp_set_shard given,
 * same source batch and initial transforms): lockstep on the stream, the all-reduce is a device sum in member order */
int sf_icp_align_group(sf_icp **members, int n_members, int mode, sf_icp_result *out, int *resumes /* or NULL */);
/* owned-query candidates of this rank per scan in the last sharded alignment */
int sf_icp_owned_counts(sf_icp *icp, int64_t *counts, int cap);
/* Routing ("all-reduce only when the submap spans tiles"): the slabs [lo[b], hi[b]] scan b can reach -- the x-extent of its
 * bounding box under its initial pose (inits: batch x 16 doubles or NULL) widened by margin, against the slab edges
 * (n_slabs + 1 ascending values, first -inf, last +inf).  lo == hi: one rank registers the scan alone, unsharded, no
 * collective; otherwise the ranks lo..hi do, on a communicator of just those ranks.  hi < lo: no finite point. */
int sf_shard_route(const float *xyz, int64_t n_per_scan, int batch, const double *inits, const double *edges, int n_slabs, double margin,
                   int32_t *lo, int32_t *hi);

/* profiling: wraps every NN kernel of the following aligns in hipEvents on the context
 * stream; sf_icp_profile_read returns launches and summed milliseconds since enabling. */
int sf_icp_profile_enable(sf_icp *icp, int on);
int sf_icp_profile_read(sf_icp *icp, int64_t *nn_launches, double *nn_ms_total);
/* every profiled NN launch in launch order: duration [ms] and, for the fused O3D_P2P / P2PLANE kernel, how many queries and
 * waves ran the search in it (the rest kept their certified neighbour); any output may be NULL, *n = launches recorded */
int sf_icp_profile_read_launches(sf_icp *icp, float *ms, uint32_t *searched_queries, uint32_t *searched_waves, int64_t cap, int64_t *n);
/* the sharded path's other phases while profiling is on: per-launch durations [ms] of one kind, in order (ms NULL: count only) */
#define SF_PROF_NN 0
#define SF_PROF_REDUCE 1      /* slab rows -> one exchange record per scan */
#define SF_PROF_COLLECTIVE 2  /* the all-reduce of the records (RCCL or P2P), as the stream saw it: waiting for peers included */
#define SF_PROF_SOLVE 3       /* the identical solve on every rank */
#define SF_PROF_SHARD_BUILD 4 /* owned-query compaction + ordering at the start / resume of an alignment (one host sync inside) */
#define SF_PROF_KINDS 5
int sf_icp_profile_read_phases(sf_icp *icp, int kind, float *ms, int64_t cap, int64_t *n);

/* ------------------------------------------------------------------ BruteForceAlignment (start-up coarse lock) */
/* localization/include/localization/brute_force_alignment.h:22-112 and
 * localization/src/brute_force_alignment.cpp: every candidate pose of the x,y,z,yaw grid is
 * scored by the mean SQUARED NN distance of the source points (all candidates of one x slice
 * in one launch); the first candidate under the threshold, in the reference's nesting
 * order, wins.  Same setters, same state (previous / best transformation, first-alignment
 * flag, the trace == 4 rule of setInitialGuess). */
typedef struct sf_bf sf_bf;
int sf_bf_create(sf_ctx *ctx, sf_bf **out);
void sf_bf_destroy(sf_bf *bf);
int sf_bf_set_xyz_step(sf_bf *bf, float x_step, float y_step, float z_step);
int sf_bf_set_xyz_range(sf_bf *bf, float x, float y, float z);
int sf_bf_set_rotation_step(sf_bf *bf, float yaw_step);
int sf_bf_set_rotation_range(sf_bf *bf, float yaw);
int sf_bf_set_mean_error_threshold(sf_bf *bf, float error_threshold);
int sf_bf_set_initial_guess(sf_bf *bf, const float T[16]);
int sf_bf_set_source(sf_bf *bf, const float *xyz, int64_t n);
int sf_bf_set_source_cloud(sf_bf *bf, sf_cloud *cloud);
int sf_bf_set_target(sf_bf *bf, const float *xyz, int64_t n);
int sf_bf_set_target_map(sf_bf *bf, sf_map *map);
int sf_bf_reset_first_alignment(sf_bf *bf, int value);
/* Refused with the handle's state untouched (previous / best transformation, first-alignment flag, last result):
 * SF_ERR_STATE without a source or a target, for a target with no point and for a map window that accepts none;
 * SF_ERR_INVALID for a step that is not finite and > 0, a range that is not finite and >= 0, a sequence of more
 * than 4 096 entries, more than 2^20 candidates in all or more than 65 535 in one x slice.  A source point with a
 * non-finite coordinate adds 0 to every score and still counts in its divisor. */
int sf_bf_align_clouds(sf_bf *bf, int *found);
int sf_bf_first_alignment_completed(sf_bf *bf);
int sf_bf_get_best_transformation(sf_bf *bf, float T[16]);
/* diagnostics of the last alignClouds: chosen candidate (nesting-order index), its score,
 * and the float32 score of every candidate evaluated before the early exit (NaN after it) */
int sf_bf_last_result(sf_bf *bf, int32_t *index, float *score, int32_t *n_candidates, float *scores, int64_t cap);

/* ------------------------------------------------------------------ GlobalMapFramesManager (start-up I/O) */
/* localization/src/global_map_frames_manager.cpp: map.pcd cache or merge of the recorded
 * cloud_<n>.pcd tiles + PCL voxel grid (on the device) + save (:93-151); map_T_global from
 * odometry_positions.txt / gps_imu_poses.txt with the bad-reading filter (:153-248);
 * altitude look-up table (:60-63, :69-91). */
typedef struct sf_frames sf_frames;
sf_frames *sf_frames_create(const char *data_folder, const char *map_name, int64_t num_poses_max);
void sf_frames_destroy(sf_frames *fr);
int sf_frames_get_map_cloud(sf_frames *fr, sf_cloud *out, float voxel_size, int *loaded_cached);
int sf_frames_get_map_T_global(sf_frames *fr, double T[16]);
float sf_frames_get_closest_altitude(sf_frames *fr, double lat, double lon);
int sf_frames_altitude_table(sf_frames *fr, double *table_lat_lon_alt, int64_t cap_rows, int64_t *rows);

/* ------------------------------------------------------------------ MapDataSaver file writers (recorder side of f-3) */
/* mapping/src/map_data_save_node.cpp:12-29 (folder wiped and re-created, "tx ty tz" / "lat lon alt y" headers),
 * :61-98 (per synchronized cloud/GPS/odometry triple: cloud appended to the open tile, cloud_<counter>.pcd written
 * with savePCDFileBinary every 10 clouds -- map_data_save_node.h:72 --, one line per log: odometry with default
 * ostream formatting, GPS with std::fixed << std::setprecision(8)), :100-112 (open tile flushed on shutdown).
 * compass_yaw is the recorder's own double conversion of the heading (:38-49): sf_recorder_compass_yaw. */
typedef struct sf_recorder sf_recorder;
int sf_recorder_create(const char *map_data_path, sf_recorder **out);
int sf_recorder_add(sf_recorder *r, const float *xyz, int64_t n, const double odom_xyz[3], double lat, double lon, double alt, double compass_yaw);
int sf_recorder_shutdown(sf_recorder *r);
void sf_recorder_destroy(sf_recorder *r);
double sf_recorder_compass_yaw(double compass_hdg_deg);

/* ------------------------------------------------------------------ pose fusion (host, float32 like the reference) */
/* a14: computePosePredictionFromOdometry — localization_node.cpp:89-110 */
void sf_fusion_quat_to_pose(const double q_wxyz[4], const double t[3], float T[16]);
void sf_fusion_odom_prediction(const float map_T_sensor[16], const float odom_T_prev[16],
                               const float odom_T_cur[16], float out[16]);
/* a15: compass callback :64-76, UTM::LLtoUTM geo_lib.hpp:38-83, getClosestAltitude
 * global_map_frames_manager.cpp:69-91, computeGpsCoarsePoseInMapFrame :112-128 */
float sf_fusion_compass_to_yaw(double compass_deg);
void sf_fusion_ll_to_utm(double lat, double lon, double *northing, double *easting);
float sf_fusion_closest_altitude(const double *table_lat_lon_alt, int rows, double lat, double lon);
void sf_fusion_gps_pose(const double map_T_global[16], float yaw, double lat, double lon,
                        float table_alt, float out[16]);
/* a16: computePoseGainsFromCovarianceMatrices — localization_node.cpp:151-179 */
void sf_fusion_pose_gains(const double gps_cov[9], const double odom_cov[36], int fixed,
                          float *odom_gain, float *gps_gain);
/* a17: prior blend — localization_node.cpp:329 */
void sf_fusion_blend(float g_odom, const float T_odom[16], float g_gps, const float T_gps[16],
                     float out[16]);
/* computeMapTGlobal — global_map_frames_manager.cpp:209-248 */
void sf_fusion_map_T_global(const double *latlonalt, const float *yaw, int n, double out[16]);
void sf_fusion_mat4f_inverse(const float A[16], float out[16]);
void sf_fusion_mat4f_mul(const float A[16], const float B[16], float out[16]);
/* a18: StochasticFilter — stochastic_filter.cpp:3-27,44-113 */
typedef struct sf_sfilter sf_sfilter;
sf_sfilter *sf_sfilter_create(int queue_size, float n_std_dev_threshold);
void sf_sfilter_destroy(sf_sfilter *f);
void sf_sfilter_set_maximum_linear_velocity(sf_sfilter *f, float v);
void sf_sfilter_weights(const sf_sfilter *f, float *w);
void sf_sfilter_add_pose_to_queue(sf_sfilter *f, const float pose[16]);
float sf_sfilter_pose_zscore(const sf_sfilter *f, const float prev[16], const float cur[16]);
void sf_sfilter_apply_gaussian_filter(const sf_sfilter *f, const float prev[16],
                                      const float cur[16], float out[16]);

/* ------------------------------------------------------------------ the node's per-scan callback as one call
 * LocalizationNode::localizationCallback and its helpers -- localization/src/localization_node.cpp:263-344 (callback),
 * :62-77 (compass), :112-128 (GPS pose), :181-261 (coarse alignment), constructor constants :19-43 -- over the entry
 * points above: same order, same constants, same state, everything device-side on the context's stream.  The ROS 2 shell
 * (subscriptions, synchroniser, publishers) stays with the caller. */
typedef struct sf_node sf_node;
typedef struct {
    float ref_frame_distance; /* 3 m: re-crop distance, localization_node.h:142                                     */
    float cloud_crop_radius;  /* 10 m: scan and map crop radius, localization_node.h:145                            */
    float index_cell;         /* grid cell of the whole-map index (0.5 m; 0 = automatic)                              */
    int32_t pcl_crop_order;   /* 1: the scan crop keeps PCL's ascending-distance order (point_cloud_processing.hpp:40-52) */
    int32_t icp_mode;         /* SF_ICP_REF_CPP (the node's ICPPointToPoint)                                          */
    int32_t map_is_downsampled; /* 0: apply getMapCloud's 0.1 m voxel grid (:19) before the stride-3 subsample (:20) */
} sf_node_params;
typedef struct { /* the sensor_msgs/NavSatFix fields the node reads */
    double latitude, longitude, altitude;
    double position_covariance[9];
} sf_gps_fix;
typedef struct { /* the nav_msgs/Odometry fields the node reads */
    double q_wxyz[4];
    double t[3];
    double covariance[36];
} sf_odom;
#define SF_NODE_OK 0              /* map_T_sensor is the new pose                                           */
#define SF_NODE_GATED_ALTITUDE 1  /* negative GPS altitude: message dropped (:269-276)                       */
#define SF_NODE_FIRST_MESSAGE 2   /* first message: pose initialised from GPS + compass, no alignment (:278-283) */
#define SF_NODE_COARSE_FAILED 3   /* the start-up lock was not found on this scan (:307-315)                 */
typedef struct {
    int32_t status;          /* SF_NODE_*                                                                     */
    int32_t recropped;       /* the map window moved on this scan (:299-305)                                  */
    int32_t coarse_ran;      /* 0 no, 1 brute force only, 2 brute force + the "strong" ICP                    */
    int32_t pad_;
    int64_t n_scan;          /* scan points after the stride-2 subsample and the radius crop                  */
    float map_T_sensor[16];  /* the node's pose after this message                                            */
    float prior[16];         /* the filtered prior handed to the ICP (:318-332)                               */
    float odom_pose[16], gps_pose[16];
    float odometry_gain, gps_compass_gain;
    sf_icp_result icp;       /* the fine alignment                                                            */
    sf_icp_result coarse_icp; /* the "strong" ICP of the coarse phase when coarse_ran == 2                    */
} sf_node_output;
void sf_node_default_params(sf_node_params *p);
/* map_xyz: the map cloud (getMapCloud's output when map_is_downsampled); altitude table rows = (lat, lon, alt) */
int sf_node_create(sf_ctx *ctx, const float *map_xyz, int64_t n_map, const double map_T_global[16], const double *altitude_table_lat_lon_alt, int rows,
                   const sf_node_params *params /* or NULL */, sf_node **out);
void sf_node_destroy(sf_node *n);
int sf_node_compass(sf_node *n, double compass_deg); /* compassCallback :62-77 */
int sf_node_callback_xyz(sf_node *n, const float *xyz, int64_t n_points, const sf_gps_fix *gps, const sf_odom *odom, sf_node_output *out);
int sf_node_callback_pointcloud2(sf_node *n, const void *data, int64_t data_bytes, int64_t width, int64_t height, int point_step, int64_t row_step, int off_x, int off_y,
                                 int off_z, int datatype, int is_bigendian, const sf_gps_fix *gps, const sf_odom *odom, sf_node_output *out);
#define SF_NODE_POSE_MAP_T_SENSOR 0
#define SF_NODE_POSE_MAP_T_REF 1
#define SF_NODE_POSE_ODOM_PREVIOUS 2
int sf_node_set_pose(sf_node *n, int which, const float T[16]); /* callers that already hold a lock */
int sf_node_get_pose(sf_node *n, int which, float T[16]);
int sf_node_set_coarse_alignment_complete(sf_node *n, int complete);
int sf_node_coarse_alignment_complete(sf_node *n);
sf_icp *sf_node_icp(sf_node *n); /* the node's icp_ (parameters, counters) */
struct sf_bf;
struct sf_bf *sf_node_bf(sf_node *n); /* the node's brute_force_alignment_ (pose grid, threshold) */

/* f-4 (EXTENSION, no reference counterpart): error-state EKF pose prior with IMU pre-integration.
 * The reference has no EKF and never reads the IMU (SURVEY.md "Read this first"); its prior is the
 * blend + StochasticFilter above.  Nominal state: position, velocity (map frame), attitude R (map <- sensor),
 * gyro bias, accelerometer bias; 15x15 covariance over (dp, dv, dtheta, dbg, dba), attitude error on the right.
 * Host code, float64, row-major.  After sf_ekf_reset the bias states carry zero variance and zero random walk, i.e.
 * the filter is the 9-state (p, v, theta) one until sf_ekf_set_bias / sf_ekf_set_bias_noise give them room. */
typedef struct sf_ekf sf_ekf;
int sf_ekf_create(sf_ekf **out);
void sf_ekf_destroy(sf_ekf *e);
int sf_ekf_reset(sf_ekf *e, const double T[16], const double v[3] /* or NULL */, const double P_diag[9] /* or NULL: identity */);
int sf_ekf_set_noise(sf_ekf *e, double gyro_sigma, double accel_sigma, const double gravity[3] /* or NULL: (0, 0, -9.80665) */);
/* bias estimates and their variances (any argument may be NULL = unchanged); bias random walks per sqrt(second) */
int sf_ekf_set_bias(sf_ekf *e, const double gyro_bias[3], const double accel_bias[3], const double gyro_bias_var[3], const double accel_bias_var[3]);
int sf_ekf_set_bias_noise(sf_ekf *e, double gyro_bias_walk, double accel_bias_walk);
/* n IMU samples (rad/s, specific force m/s^2 in the sensor frame) of period dt, integrated one by one */
int sf_ekf_predict_imu(sf_ekf *e, const double *gyro, const double *accel, int64_t n, double dt);
/* the reference's prediction (localization_node.cpp:89-110) as an EKF step: pose <- pose * (prev^-1 cur), covariance
 * through the step's Jacobian (dp <- -R [d_t]x dtheta, dtheta <- d_R^T dtheta) plus the odometry noise */
int sf_ekf_predict_odometry(sf_ekf *e, const double odom_T_prev[16], const double odom_T_cur[16], const double cov_pos[3], const double cov_rot[3]);
int sf_ekf_update_position(sf_ekf *e, const double p_map[3], const double cov[9]);   /* GPS, already in the map frame (sf_fusion_gps_pose) */
int sf_ekf_update_yaw(sf_ekf *e, double yaw, double var);                            /* compass (sf_fusion_compass_to_yaw) */
int sf_ekf_update_pose(sf_ekf *e, const double T[16], const double cov_pos[3], const double cov_rot[3]);  /* ICP result */
/* The same update with the ICP's own 6x6 covariance (sf_icp_covariance::cov, order (wx wy wz tx ty tz), left perturbation
 * T' = Exp(w, t) T of the measured pose).  Innovation as above: y = (p_meas - p, Log(R^T R_meas)).  To first order the
 * perturbed measurement is p' = p_meas + w x p_meas + t and R' = (I + [w]x) R_meas = R_meas Exp(R_meas^T w), so the filter's
 * measurement error is (dp, dtheta) = A (w, t) with A = [[-[p_meas]x, I], [R_meas^T, 0]] and the measurement noise A cov A^T. */
int sf_ekf_update_pose_cov(sf_ekf *e, const double T[16], const double cov[36]);
int sf_ekf_get(const sf_ekf *e, double T[16], double v[3], double P[81]);            /* any output may be NULL; P = the (dp, dv, dtheta) block */
int sf_ekf_get_full(const sf_ekf *e, double gyro_bias[3], double accel_bias[3], double P[225]); /* biases and the whole 15x15 covariance */

/* ------------------------------------------------------------------ test hooks (NOT part of the drop-in boundary)
 * The stable radix sort and the device scans every indexed structure stands on (voxel grids, grid index, sorted crop,
 * cluster labels), run directly on host arrays so that the suite can compare them with a plain reference.  No reference
 * counterpart; nothing in an integration calls them.  Both run the library's own kernels on the context's stream,
 * synchronise and copy the result back.  Every device array is carved from one allocation as
 * [guard | lead | n elements | guard] with guards of 4096 elements holding a fixed pattern; *guard_damage = the 32-bit
 * guard words that no longer hold it afterwards (0 unless a kernel wrote outside its array).
 * sf_test_radix_sort: stable sort of n (key, value) pairs by the low passes x bits bits of the key, passes =
 *   ceil(end_bit / 8), bits = ceil(end_bit / passes) (end_bit rounded up to equally wide passes; every key arrives whole).
 *   vals == vals_out == NULL: keys only.  lead / lead_alt: elements by which the first element of the primary /
 *   ping-pong arrays is displaced from a 16-byte boundary.
 * sf_test_scan_u32: op 0: out[i] = carry0 + in[0] + ... + in[i-1] (uint32 arithmetic); op 1: out[i] = max(carry0, in[0..i]).
 *   in_place != 0 scans the device array onto itself.
 * n = 0 and n = 1 succeed.  SF_ERR_INVALID, nothing touched: key_bytes not 4 or 8; end_bit = 0 with n > 1 or
 * end_bit > 8 key_bytes; a lead outside 0..3; op not 0 or 1; n < 0 or n > 2^26; a NULL array that is needed (vals and
 * vals_out go together). */
int sf_test_radix_sort(sf_ctx *ctx, int key_bytes /* 4 | 8 */, const void *keys, const uint32_t *vals /* or NULL: keys only */, int64_t n, unsigned end_bit,
                       int lead /* 0..3 */, int lead_alt /* 0..3 */, void *keys_out, uint32_t *vals_out /* or NULL */, int64_t *guard_damage);
int sf_test_scan_u32(sf_ctx *ctx, int op /* 0: exclusive sum, 1: inclusive max */, const uint32_t *in, int64_t n, uint32_t carry0, int in_place, uint32_t *out,
                     int64_t *guard_damage);

/* The float64 numerical core, run directly on host float64 arrays: the hooks launch kernels that CALL
 * the production device functions of csrc/sf_icp.hip, csrc/sf_cov.hpp and csrc/sf_map.hip -- no copy, no second
 * implementation -- on the context's stream, synchronise and copy the result back.
 * sf_test_linalg: `cases` independent cases, one per thread in workgroups of 64 (one working lane per case, as in
 *   production).  Case i reads in[i * in_stride ..] and writes out[i * out_stride ..]; doubles read / written by op:
 *     SF_TEST_OP_RSQRT    x                        ->  rsqrt_nr(x), recip_nr(x)                          1 / 2
 *     SF_TEST_OP_SVD3     A (3x3 row-major)        ->  U (9), S (3, descending), V (9):  A = U S V^T      9 / 21
 *     SF_TEST_OP_KABSCH   record (32: n, sum s, sum t, sum s t^T row-major, rest ignored) -> T (4x4)      32 / 16
 *     SF_TEST_OP_LDLT6    A (6x6), b (6)           ->  rc (0 | -1 as a double), x (6; zeros when rc = -1) 42 / 7
 *     SF_TEST_OP_VEC6     v = (rx, ry, rz, t)      ->  T (4x4) = [Rz Ry Rx | t]                           6 / 16
 *     SF_TEST_OP_JACOBI3  A (3x3 symmetric)        ->  eigenvalues (unsorted), V (9), sweeps that rotated 9 / 13
 *     SF_TEST_OP_JACOBI6  A (6x6 symmetric)        ->  eigenvalues (unsorted), V (36), sweeps             36 / 43
 *     SF_TEST_OP_ROBUST   kind, k, r               ->  w(r) of SF_ROBUST_<kind>                           3 / 1
 *     SF_TEST_OP_EIGVEC   C (3x3 symmetric)        ->  the unit normal smallest_eigvec(C) of the map normals  9 / 3
 *   Doubles of out beyond what the op writes come back as they went in.
 * sf_test_wave_reduce: one workgroup of 256; lane l of it holds in[l * width .. + width]; out[l] = what
 *   wave_reduce_<width> returned on lane l (width 32: the wave's total of component (l % 64) >> 1; 16: of component
 *   ((l % 64) >> 2) & 15; 1: of the one value).
 * sf_test_block_reduce: block_reduce_store<nrec> of one workgroup of 256 (lane l contributes in[l * nrec .. + nrec]) into
 *   a device copy of out[32]: out[c < nrec] = the workgroup's total of component c, out[c >= nrec] as it went in.
 * sf_test_reduce_partials: reduce_partials<nrec, nt> over part[nblocks][32] by one workgroup of nt threads -> out[32]
 *   (out[c >= nrec] = 0).  Only the instantiations the library uses: nt = 256 with nrec 11 | 17 | 24 | 30, nt = 1024 with
 *   nrec 17 | 30.
 * SF_ERR_INVALID, nothing touched: an unknown op / width / nrec / (nrec, nt); a stride below what the op reads or writes or
 *   above 64; cases outside [0, 2^20]; nblocks outside [0, 65536]; a NULL array that is needed (none for cases = 0 or
 *   nblocks = 0). */
#define SF_TEST_OP_RSQRT 0
#define SF_TEST_OP_SVD3 1
#define SF_TEST_OP_KABSCH 2
#define SF_TEST_OP_LDLT6 3
#define SF_TEST_OP_VEC6 4
#define SF_TEST_OP_JACOBI3 5
#define SF_TEST_OP_JACOBI6 6
#define SF_TEST_OP_ROBUST 7
#define SF_TEST_OP_EIGVEC 8
int sf_test_linalg(sf_ctx *ctx, int op, const double *in, int in_stride, int64_t cases, double *out, int out_stride);
int sf_test_wave_reduce(sf_ctx *ctx, int width /* 1 | 16 | 32 */, const double *in /* [256][width] */, double *out /* [256] */);
int sf_test_block_reduce(sf_ctx *ctx, int nrec /* 17 | 30 */, const double *in /* [256][nrec] */, double *out /* [32], in and out */);
int sf_test_reduce_partials(sf_ctx *ctx, int nrec /* 11 | 17 | 24 | 30 */, int nt /* 256 | 1024 */, const double *part /* [nblocks][32] */, int nblocks, double *out /* [32] */);

/* sf_cloud_score_planes with the grid of its scoring kernel capped at max_blocks workgroups (0: the production choice, at most
 * 65536), so that a small cloud exercises the path where one workgroup takes several tiles. */
int sf_test_plane_score(sf_cloud *c, const float *planes, int64_t n_planes, double t, int max_blocks, int64_t *counts);

/* sf_cloud_score_poses with the first grid dimension of its scoring kernel capped at max_blocks workgroups (0: the production
 * choice; a lane then takes several transforms) and the pairs split into slices of pair_chunk (0: the production choice; the
 * slices of a transform meet in one integer atomic each), so that a small case runs on 1 and 3 workgroups and through the path
 * that splits the pairs.  SF_ERR_INVALID: max_blocks outside 0 .. 65536, pair_chunk < 0. */
int sf_test_score_poses(sf_cloud *src, sf_cloud *dst, const int32_t *pairs, int64_t m, const float *T12, int64_t n_poses,
                        double distance_threshold, int max_blocks, int64_t pair_chunk, int64_t *counts);

/* sf_cloud_label_boxes with the grid of its three segmented passes capped at max_blocks workgroups (0: the production choice, at
 * most 1024), so that a small cloud exercises the path where one workgroup walks several tiles and carries the open segment
 * from tile to tile.  The summation order depends on the grid, so the moments differ from the production
 * call's within their rounding bound (and the axes with them); count, lo, hi, valid and the stats are equal. */
int sf_test_label_boxes(sf_cloud *c, const int32_t *labels, int64_t n_labels, const sf_box_params *p, int max_blocks,
                        sf_label_box *boxes, sf_box_stats *stats);

/* The launch schedule of an O3D_P2P / P2PLANE alignment (csrc/sf_schedule.hpp): the form launch k takes under
 * each of `rows` configurations.  Host code alone -- make_schedule, launches and step_of, the functions every driver of the library
 * dispatches on -- so it needs no context and no device.
 *   in [rows][SF_TEST_SCHEDULE_IN]:   mode (SF_ICP_O3D_P2P | SF_ICP_P2PLANE), iterations K, queries per lane (1 | 2), sharded,
 *     enqueued whole (1) or stepped (0), neighbour reuse, window kind of the map, robust kernel on, frozen pairs wanted,
 *     from_launch, deferred search, neighbour table consulted, first launch that consults it, learnt first look-up launch, queries
 *     sorted by tile
 *   out[rows][SF_TEST_SCHEDULE_OUT]:  launches of the alignment; of launch k: its form (0 search, 1 tile search, 2 deferring,
 *     3 freeze launch, 4 frozen, few workgroups), one query per lane, the solve takes the freeze state, the solve may ask for a
 *     freeze launch, the deferred rows are added, the launch index from which k_nn_red_df first tries to verify a whole wave; of the
 *     schedule: frozen pairs on, first look-up launch, first deferring launch (both from_launch: none)
 * k is not checked against the launch count.  SF_ERR_INVALID: rows < 0, or a NULL array with rows > 0. */
#define SF_TEST_SCHEDULE_IN 15
#define SF_TEST_SCHEDULE_OUT 10
int sf_test_launch_schedule(const int32_t *in, int64_t rows, int k, int32_t *out);

/* The stream compaction every crop and filter ends in, and the bounds reduction every voxel grid and grid index starts from
 * (csrc/sf_cloud.hip), run directly on a cloud.  Both CALL the production functions -- no copy.
 * sf_test_compact: uploads flags[n] (n = the cloud's size, host memory) into the cloud's own flag buffer, takes a new stamp as
 *   the crops do and runs sf::compact_cloud: the points whose flag is not 0 stay, in order; read them with sf_cloud_download and
 *   their indices with sf_cloud_last_indices.  n = 0 succeeds (flags may be NULL then).
 * sf_test_cloud_minmax: bounds of the points whose three coordinates are finite and their number (zeros when there is none).
 *   enqueue_form = 0: sf::cloud_minmax (the voxel grids, sf_map_build); otherwise sf::cloud_minmax_enqueue into a device buffer
 *   of the hook's own, copied back after a stream synchronise (sf_cloud_voxel_merge, sf_map_patch).  n = 0 succeeds in both.
 * SF_ERR_INVALID: a NULL argument that is needed. */
int sf_test_compact(sf_cloud *c, const uint8_t *flags); /* flags: host, [n] */
int sf_test_cloud_minmax(sf_cloud *c, int enqueue_form, float mn[3], float mx[3], int64_t *n_finite);

/* The query ordering that runs in front of an alignment (csrc/sf_order.hpp), run directly on host points with
 * buffers of the hook's own: k_order_hist -> k_order_scan -> form 0: k_order_scatter + k_order_gather (ids, then the records
 * gathered), form 1: k_order_move (ranked and moved in one pass; what an alignment's plain path runs).  The library's own path is
 * not altered.
 *   points [batch][n][3]: the scans; poses [batch][16]: one row-major 4x4 pose per scan (the key is the map cell of the posed
 *   point); table != 0: the density-equalised buckets of the map's index (what an alignment uses), 0: the plain cell key.
 *   keys [batch][n]: the 10-bit bucket of every point, in element order (1023: a non-finite posed point);
 *   ordered [batch][n][3]: every scan stably ordered by key, the coordinates bit for bit those of `points`.
 * SF_ERR_INVALID: a NULL argument, a map without an index, batch outside [1, 64], n outside [1, 2^20], form not 0 or 1. */
int sf_test_query_order(sf_map *map, const float *points, int batch, int64_t n, const double *poses, int form, int table, uint16_t *keys, float *ordered);

/* The neighbour cache that the launch list of the latest sf_icp_align_batch_async / sf_icp_align_batch left behind, read back
 * (csrc/sf_icp_testhooks.hpp).  Host code alone: the context's stream is synchronised and the arrays are
 * copied out; no kernel is launched, nothing is written on the device and no member of the object changes, so the alignment's
 * results and every later alignment are what they would have been without the call.
 * For scan b, per cache entry in cache order (entry i of the scan is slot b * n + i of the lane's arrays):
 *   x0 [n][3]   the source point the entry belongs to, as the kernels read it (the ordered copy when the queries were ordered)
 *   orig [n]    its index in the scan as given: i without ordering, the id the tile sort kept, -1 under the plain cell order
 *               (its move kernel keeps no ids).  May be NULL.
 *   nbr [n][3], j [n]   the cached neighbour and its position in the index (negative: none within the acceptance radius)
 *   e [n]       E = D + M_then of the reuse certificate (<= 0: no search behind the entry)
 * and in *info the scan's pose, its motion bound (IcpState::motion) and counters as the last launch left them.
 * cap: entries the arrays hold.  cap = 0 with every array NULL is the size query: *info alone (info->n = entries per scan).
 * SF_ERR_STATE, touching nothing: no alignment yet, or the latest one was REF_CPP, the single launch (its cache lives in registers),
 * sharded, stepped or ran with the neighbour reuse off.  SF_ERR_INVALID, touching nothing: b outside the batch, cap below n, a
 * NULL array that is needed. */
typedef struct sf_icp_cache_info {
    double T[16];
    double motion;
    int64_t n;
    int32_t batch, mode;
    int32_t cache_live, n_research, iterations;
    int32_t ordered; /* 0: as given, 1: cell order (no ids kept), 2: tile order (ids kept) */
} sf_icp_cache_info;
int sf_icp_test_download_cache(sf_icp *icp, int b, int64_t cap, float *x0, int32_t *orig, float *nbr, int32_t *j, float *e, sf_icp_cache_info *info);

#ifdef __cplusplus
}
#endif
#endif

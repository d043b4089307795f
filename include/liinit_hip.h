/* liinit_hip.h — C-ABI of the MI355X-native LI-Init hot path (libliinit_hip.so).
 *
 * The reference (hku-mars/LiDAR_IMU_Init) has NO plugin / FFI seam: its hot path is inline C++ over
 * globals in one ROS executable.  This header therefore DEFINES the boundary a
 * maintainer would bind to; every entry point names the reference code it replaces (file:line relative
 * to the reference root).  Conventions:
 *   - plain C, opaque handle, `int` status (0 = LII_OK, negative = error; lii_strerror / lii_last_error);
 *   - caller-owned host buffers, library-owned device buffers; no exceptions cross the boundary;
 *   - one handle is used from one host thread; all device work of a handle runs on ONE HIP stream;
 *   - the library FAILS (LII_ERR_NO_DEVICE) when no gfx950 device is usable — there is no CPU fallback.
 */
#ifndef LIINIT_HIP_H
#define LIINIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LII_ABI_VERSION 9 /* 2: lii_scan_job::scan_dev / n_scan_dev, lii_comm_init_ex, lii_comm_transport
                             3: lii_params_*, lii_comm_set_partition (library-side split of the down-sampled cloud)
                             4: lii_scan_upload_next / lii_scan_advance (the next scan travels while the current one registers)
                             5: LII_COMM_MAILBOX = the peer-mapped HBM mailbox (HIP IPC), LII_COMM_MAILBOX_HOST, lii_comm_rccl_ranks
                             6: lii_scan_job::scan_sorted (struct_size 56; a job of size 48 - ABI 5 - is still accepted), lii_last_kernel_profile,
                                lii_comm_describe, lii_comm_set_partition(h, 2) (split by voxel), lii_scan_job::map_update (the reserved field)
                             7: lii_ingest_opts::cut_frame_num = 0 (the whole message as one frame: Preprocess::process), lii_last_solve_info,
                                lii_selftest_list_exchange
                             8: lii_last_unfinished_queries, lii_scan_job::next_scan_dev / next_n_scan (struct_size 72: the pre-armed prologue)
                             9: lii_ingest_pcl2_begin / lii_ingest_livox_begin / lii_ingest_end (driver messages queue on the device: message k + 1 is
                                transferred and decoded while the sub-frames of message k are registered), lii_scan_job::while_waiting (struct_size 88) */

enum lii_status {
  LII_OK = 0,
  LII_ERR_INVALID = -1,   /* bad argument / NULL / size */
  LII_ERR_NO_DEVICE = -2, /* no HIP device (the library never falls back to the CPU) */
  LII_ERR_HIP = -3,       /* a HIP runtime call failed; see lii_last_error */
  LII_ERR_CAPACITY = -4,  /* more points than the handle was created for */
  LII_ERR_STATE = -5,     /* call order violated (e.g. registration without a map) */
  LII_ERR_COMM = -6       /* RCCL failure */
};

typedef struct lii_context* lii_handle;

/* Replaces the file-scope configuration of the reference: NUM_MATCH_POINTS 5 (include/common_lib.h:28),
 * Nearest_Search max_dist 5 (src/laserMapping.cpp:980), esti_plane threshold 0.1 (:997),
 * LASER_POINT_COV 0.001 (:59), the fixed 100000-point arrays (:108-109,117-119 — lifted to a capacity). */
typedef struct lii_config {
  int32_t struct_size;       /* = sizeof(lii_config) */
  int32_t device;            /* HIP device ordinal */
  int32_t max_scan_points;   /* capacity of one (sub-)scan, N */
  int32_t max_map_points;    /* capacity of the local map, M */
  float map_cell_size;       /* edge of the device k-NN grid cell [m]; <= 0: 3 x map_downsample_size */
  float map_downsample_size; /* ikd-Tree downsample box = mapping/filter_size_map (set_downsample_param) */
  float max_match_dist2;     /* accept neighbours with d^2 <= this (5.0) */
  float reserved0;
  double plane_threshold;     /* 0.1 */
  double laser_point_cov_inv; /* 1000 */
} lii_config;

/* IMU pose-table record: msg/Pose6D.msg:1-7 as filled by set_pose6d (include/common_lib.h:183-199). */
typedef struct lii_pose6d {
  double offset_time; /* [s] from scan start */
  double acc[3], gyr[3], vel[3], pos[3];
  double rot[9]; /* row-major */
} lii_pose6d;

/* StatesGroup (include/common_lib.h:68-169) as POD; rotation matrices row-major; cov 24x24 row-major.
 * State order: theta, p, theta_LI, T_LI, v, b_g, b_a, g (Appendix B of SURVEY.md). */
typedef struct lii_state {
  double rot_end[9];
  double pos_end[3];
  double offset_R_L_I[9];
  double offset_T_L_I[3];
  double vel_end[3];
  double bias_g[3];
  double bias_a[3];
  double gravity[3];
  double cov[24 * 24];
} lii_state;

/* Options of one scan registration — the loop constants of src/laserMapping.cpp:957-1134. */
typedef struct lii_iekf_opts {
  int32_t max_iterations; /* NUM_MAX_ITERATIONS (param max_iteration; launch files: 5) */
  int32_t imu_en;         /* 0: LiDAR-only odometry (H cols 6..11 = 0), 1: LIO with extrinsic in state */
} lii_iekf_opts;

typedef struct lii_iekf_report {
  int32_t iterations;    /* executed */
  int32_t searches;      /* k-NN passes executed (S) */
  int32_t effect_num;    /* effect_feat_num of the last iteration */
  int32_t converged;     /* flg_EKF_converged of the last iteration */
  double normal_eq[91];  /* last iteration: upper 78 of H^T R^-1 H, 12 of H^T R^-1 z, count */
} lii_iekf_report;

/* ---------------------------------------------------------------- lifecycle */
int lii_abi_version(void);
const char* lii_strerror(int status);
const char* lii_last_error(lii_handle h);
int lii_device_count(int* count);
/* Replaces the global KD_TREE / buffers of src/laserMapping.cpp:102-150. */
int lii_create(const lii_config* cfg, lii_handle* out);
int lii_destroy(lii_handle h);
int lii_synchronize(lii_handle h);

/* ---------------------------------------------------------------- local map (device mirror of the ikd-Tree)
 * lii_map_build      <- ikdtree.Build(feats_down_world->points)           src/laserMapping.cpp:921-931
 * lii_map_add_points <- ikdtree.Add_Points(PointToAdd, true|false)        src/laserMapping.cpp:556-557,
 *                       with the per-voxel keep-closest-to-centre semantics of include/ikd-Tree/ikd_Tree.cpp:381-456
 * lii_map_size       <- ikdtree.validnum()                                src/laserMapping.cpp:933
 * Points are float xyz with `stride_bytes` between records (12 for packed xyz, 48 for PointXYZINormal).
 * The map is a point SET kept on the device and updated in place: lii_map_download returns it in no particular order;
 * an update is enqueued, not waited for (lii_map_size / lii_map_download / lii_map_add_points' counter read the device).
 * LII_ERR_CAPACITY: n_valid + batch would exceed lii_config::max_map_points - tested BEFORE the batch is applied, counting
 * every point of it; the map is left as it was.  The in-place layout keeps slack behind every cell (count + max(2, count / 4)
 * slots) and moves a cell that outgrows it to the tail of a point array of 3 * max_map_points + 65 536 slots: a SPARSE map (many
 * one-point cells: 3 slots each) close to max_map_points can need a rebuild on almost every update, and a batch of b inserts asks
 * for 8 b + 4 096 free tail slots after a rebuild - if even the rebuilt map cannot offer them the call fails with
 * LII_ERR_CAPACITY ("no room left behind the cells") although n_valid + b <= max_map_points.  Size max_map_points with ~25 %
 * headroom over the largest map expected.  An update that runs out of provisioned room while it executes loses nothing: the
 * inserts it could not place are parked and re-inserted by a rebuild before the next search or update uses the map. */
int lii_map_reset(lii_handle h);
int lii_map_build(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes);
int lii_map_add_points(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes, int32_t downsample_on,
                       int32_t* n_added);
/* lii_map_delete_boxes <- ikdtree.Delete_Point_Boxes(cub_needrm)  (include/ikd-Tree/ikd_Tree.cpp:500-516; the call the reference
 *                       prepares in lasermap_fov_segment, src/laserMapping.cpp:260-305, and never makes - quirk A6: its map only
 *                       grows).  boxes = n x 6 floats (min xyz, max xyz); a point goes when min <= p < max on every axis. */
int lii_map_delete_boxes(lii_handle h, const float* boxes, int32_t n_boxes, int32_t* n_deleted);
/* ---- the moving local map: lasermap_fov_segment (src/laserMapping.cpp:260-305, called at :914 between p_imu->Process and the voxel
 * filter) FOLLOWED BY Delete_Point_Boxes(cub_needrm) - the call upstream prepared and never made (quirk A6).  A cube of edge cube_len
 * follows the sensor; when state.pos_end (the IMU's position, as upstream - not the LiDAR's) comes within 1.5 * det_range of a face the
 * cube moves by mov_dist along that axis, and the slab it leaves behind - one box per axis, x, y, z, the low side tested before the high
 * side - is deleted from the map (min <= p < max, the rule of lii_map_delete_boxes).  Without it nothing ever makes room in the map and a
 * sensor that keeps travelling ends in LII_ERR_CAPACITY.  The arithmetic is the reference's: MOV_THRESHOLD = 1.5f, det_range a float,
 * cube_len a double, the cube six floats; mov_dist = (float)max((cube_len - 2.0 * 1.5f * det_range) * 0.5 * 0.9, det_range * (1.5f - 1)).
 *
 * The setting is durable handle state (like lii_publish_set) and OFF until asked for; lii_scan_job is unchanged.
 *   lii_local_map_set      installs cube_len / det_range and sets Localmap_Initialized = false (every call of it does: the next segment
 *                          initialises the cube around its position).  enabled = 1: every lii_scan_register, lii_scan_register_imu and
 *                          lii_scan_register_cv makes one lii_local_map_segment call itself, on the device, with the PROPAGATED state - the
 *                          `state` argument of lii_scan_register, what the in-call propagation produced for the other two - behind any
 *                          map update still in flight and in front of the call's first search: three launches of fixed size, whatever
 *                          the map holds (lii_set_profiling(h, 3) counts them as LII_KP_VOXEL).  Calls that do not register are not
 *                          touched (lii_iekf_update, the separate lii_undistort_* path, lii_map_build_from_scan): their hosts call
 *                          lii_local_map_segment.  enabled = 0: only lii_local_map_segment segments.
 *   lii_local_map_segment  one such call at pos_end; works without a map (the first scan: the cube is initialised, or moved with nothing
 *                          to delete).  out == NULL: enqueued only - and, since nobody knows yet whether the cube moved, the neighbour
 *                          lists and planes of an earlier search are not used again (call it where the reference does: in front of the
 *                          scan's search); out != NULL: waits and reports (the lists are dropped when points were deleted).
 *   lii_local_map_get      waits for the stream and reports the state after the last call that ran, in-job calls included.
 * Refusals (nothing changed, an earlier setting stays in force).  LII_ERR_INVALID: NaN / infinite pos_end, cube_len or det_range;
 * det_range <= 0; cube_len <= 3 * det_range - a sensor at the centre of a fresh cube is then inside the threshold of BOTH faces of every
 * axis, the reference's arithmetic would move the cube on every scan and delete around the sensor; this includes the reference's own
 * parameter defaults (cube_side_length 200, det_range 300: lii_params_defaults), which upstream survives only because it never deletes.
 * The library refuses instead of inventing a rule.  LII_ERR_STATE: a communicator is attached (single rank for now; a registration call
 * on a handle with enabled = 1 refuses likewise), lii_local_map_segment / _get before lii_local_map_set, a call from inside
 * lii_scan_job::while_waiting.  Under LII_TEST=host_solve a registration call with enabled = 1 returns LII_ERR_STATE (the decision reads
 * the device-resident control block the host-driven loop does not have); lii_local_map_segment works there.  A job on a handle with
 * enabled = 1 neither uses nor arms the pre-armed prologue: next_scan_dev is ignored. */
typedef struct lii_local_map_opts {
  uint32_t struct_size; /* sizeof(lii_local_map_opts) */
  int32_t enabled;      /* 1: the registration calls segment by themselves */
  double cube_len;      /* cube_side_length */
  float det_range;      /* mapping/det_range */
  int32_t reserved;
} lii_local_map_opts;
typedef struct lii_local_map_info {
  uint32_t struct_size; /* sizeof(lii_local_map_info); set by the call */
  int32_t initialized;  /* Localmap_Initialized */
  float cube[6];        /* LocalMap_Points: min xyz, max xyz */
  int32_t last_n_boxes; /* cub_needrm of the last call that ran: 0 .. 3 boxes of 6 floats */
  float last_boxes[18];
  int32_t last_n_deleted; /* points those boxes removed */
  int32_t moves;          /* calls that moved the cube since lii_local_map_set */
  int64_t deleted_total;
} lii_local_map_info;
int lii_local_map_set(lii_handle h, const lii_local_map_opts* opts);
int lii_local_map_get(lii_handle h, lii_local_map_info* out);
int lii_local_map_segment(lii_handle h, const double pos_end[3], lii_local_map_info* out /* may be NULL */);
/* ---- the history of what leaves the local map: points_cache_collect() (src/laserMapping.cpp:249-254, the last statement of
 * lasermap_fov_segment, :304), which drains KD_TREE::acquire_removed_points (include/ikd-Tree/ikd_Tree.cpp:522-534) into _featsArray - the
 * reference's store for everything that has left the map.  Upstream never deletes, so it loses nothing; the library does delete (quirk A6),
 * and without this order what it deletes is gone: lii_local_map_info only counts it.  A buffer on the device, OFF until asked for: while the
 * order is in force every point a DELETE removes - by box: lii_map_delete_boxes, lii_local_map_segment, the segment call a registration
 * makes itself; by point: lii_map_delete_points, lii_map_delete_points_dev - is appended to it, by the launch that squeezes the point out of
 * its cell (no launch is added: the moving local map stays at three launches of fixed size, lii_set_profiling(h, 3) counts the same with
 * and without the order).
 *   What is collected: exactly what the delete removes - the reference's `point_deleted && !point_downsample_deleted`
 *   (ikd_Tree.cpp:1242-1249), which holds for the victims of Delete_by_range and of Delete_by_point alike; a point inside several boxes
 *   of one call once, a stored point that a list of points names once for every copy it takes.  NOT collected: the points Add_Points replaces while it
 *   down-samples (lii_map_add_points, lii_map_incremental, a registration's own map update); lii_map_reset / lii_map_build /
 *   lii_map_build_from_scan and a rebuild of the index neither collect nor touch the buffer.
 *   When: as the delete runs.  The reference hands the same points over LATER - when a rebuild happens to flatten the sub-tree that holds
 *   them (ikd_Tree.cpp:1242-1249 sits in flatten) - so its timing depends on the shape of its tree; the multiset over a run is the same.
 *   Order: unspecified - the buffer is a multiset of the map's stored float bits of x, y, z (16-byte records on the device, the fourth
 *   float the point's intensity: what lii_map_build_xyzi / lii_map_add_points_xyzi stored with it, 0.0f for every other point).
 *   Overflow: the delete always completes, the map never depends on the buffer.  Points that find no room are not stored and are counted in
 *   lost_total; nothing already held is overwritten.  From then on lii_map_removed_acquire / _view deliver what the buffer holds AND return
 *   LII_ERR_CAPACITY, until an acquire with clear != 0 has emptied it (the rule of lii_publish_saved).
 *   lii_map_removed_set      capacity in points.  0: collecting off, the contents stay readable.  The capacity the buffer already has: on
 *                            (again), the contents and totals stay.  Any other: a new, empty buffer, totals zero.  The first order that asks
 *                            for a buffer creates it (16 bytes a point).
 *   lii_map_removed_get      waits for the stream and reports (as lii_local_map_get does).
 *   lii_map_removed_acquire  packed xyz as lii_map_download delivers it; xyz_out == NULL: *n only (nothing is cleared then; LII_ERR_CAPACITY
 *                            all the same behind an overflow).  clear != 0:
 *                            the buffer is empty behind the call - acquire returns and clears; the totals go on counting.
 *   lii_map_removed_view     the records where they lie: *dev_float4 is valid until the next call that deletes or clears.
 * Refusals.  LII_ERR_INVALID: negative capacity, NULL arguments (xyz_out excepted), a bad struct_size.  LII_ERR_CAPACITY with nothing
 * cleared: capacity < *n.  LII_ERR_STATE: _get / _acquire / _view before any lii_map_removed_set; a call from inside
 * lii_scan_job::while_waiting (these calls use the handle's stream; like every entry point they end a pre-armed launch first).  Of
 * everything else the calls are observers: neighbour lists, IMU carry and publish order stay as they are.  With a communicator attached the
 * order works wherever lii_map_delete_boxes does: the maps are replicated, every rank collects the same multiset (lii_local_map_* stays
 * single rank). */
typedef struct lii_map_removed_info {
  uint32_t struct_size; /* sizeof(lii_map_removed_info): set by the caller, checked */
  int32_t capacity;     /* points; 0: off */
  int32_t held;         /* points in the buffer */
  int32_t reserved;
  int64_t collected_total; /* stored since the lii_map_removed_set that made the buffer */
  int64_t lost_total;      /* not stored for lack of room since then */
} lii_map_removed_info;
int lii_map_removed_set(lii_handle h, int32_t capacity);
int lii_map_removed_get(lii_handle h, lii_map_removed_info* out);
int lii_map_removed_acquire(lii_handle h, float* xyz_out, int32_t capacity, int32_t* n, int32_t clear);
int lii_map_removed_view(lii_handle h, const void** dev_float4, int32_t* n);
int lii_map_size(lii_handle h, int32_t* n_valid);
int lii_map_download(lii_handle h, float* xyz_out, int32_t capacity, int32_t* n);
/* Kept for callers of ABI 1: the device map is always current (updates are applied in place); waits for the stream. */
int lii_map_commit(lii_handle h);
/* lii_map_nearest <- ikdtree.Nearest_Search(point, k_nearest, Nearest_Points, Point_Distance, max_dist) for arbitrary points, k and
 *                  max_dist  (include/ikd-Tree/ikd_Tree.cpp:349-379, :825-968; the registration pass searches the handle's own
 *                  down-sampled cloud with k = 5 and max_match_dist2 and needs none of this).
 * Query i (float xyz every stride_bytes, as for lii_map_build) receives the min(k, m) nearest of the m map points with
 * d2 <= max_dist - inclusive, and the SQUARED distance against max_dist itself, as the reference compares (quirk A5) - ascending in
 * d2, where d2 is the reference's float32 calc_dist (dx*dx + dy*dy + dz*dz, left to right, no FMA): rows i*k .. i*k + count[i] - 1 of
 * pts (3 floats a row) and d2; the rows from count[i] on are written as zeros.  Among EQUAL d2 the order - and, at the end of a full
 * list, which of them is kept - is the library's own visiting order: deterministic for a given map state, otherwise unspecified (the
 * reference keeps whichever its tree visits first).  The distances are never ambiguous.  pts / d2 may be NULL (that output is not
 * wanted); count is required.
 * LII_ERR_INVALID, nothing written: k < 1 or k > 64; max_dist NaN, infinite or < 1 (the reference prunes sub-trees at
 * box_d2 > max_dist^2, which is tighter than its acceptance test below 1: its answer then depends on the shape of its tree, and the
 * library refuses instead of inventing a rule); sqrt(max_dist) > 32 map_cell_size (the ball would span more cells than a query
 * should walk - create the handle with a larger lii_config::map_cell_size); a bad stride; NULL queries with n > 0.  No map:
 * LII_ERR_STATE.  n == 0: LII_OK.  A query with a NaN coordinate gets count 0; one whose ball leaves the addressable grid is
 * searched over the cells that exist (no map point lies outside them).
 * The call is an OBSERVER: scan, down-sampled cloud, neighbour lists, IMU carry and publish order of the handle stay as they are, and
 * a registration behind it behaves as if it had not been made.  It ends a pre-armed launch and joins a map update in flight first
 * (never a map with a pending update or parked inserts); it works with a communicator attached (the map is replicated, the query
 * local) and under LII_TEST=host_solve.
 *   lii_map_nearest      host queries, host results, synchronous.  n is processed in chunks of at most 65 536 queries and 2^20 rows
 *                        (queries x k) through staging buffers of the handle - created by the first call, grown geometrically, never
 *                        more than 17 MiB of device and 17 MiB of pinned host memory, released with the handle.
 *   lii_map_nearest_dev  queries and results in device memory of the caller (lii_dev_alloc, a tensor's data_ptr): enqueued on the
 *                        handle's stream, returns without waiting - lii_synchronize or any later synchronous call orders it. */
int lii_map_nearest(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes, int32_t k, double max_dist,
                    float* pts_out /* n*k*3 */, float* d2_out /* n*k */, int32_t* count_out /* n */);
int lii_map_nearest_dev(lii_handle h, const void* xyz_dev, int32_t n, int32_t stride_bytes, int32_t k, double max_dist,
                        float* pts_dev, float* d2_dev, int32_t* count_dev);
/* lii_map_radius <- the ball query: upstream ikd-Tree's Radius_Search; in the reference's copy of the tree the idiom
 *                  Nearest_Search(point, k, Nearest_Points, Point_Distance, max_dist) with k above the ball's population, which
 *                  lii_map_nearest cannot serve (k <= 64, max_dist >= 1).
 * Query i (float xyz every stride_bytes, as for lii_map_nearest) receives EVERY live map point with d2 <= max_dist, however many there
 * are: d2 is the reference's float32 calc_dist (left to right, no FMA), compared as a float against the double max_dist, inclusive -
 * the rule of lii_map_nearest and of Search (quirk A5); max_dist is a SQUARED distance.  The points stand in rows
 * offsets[i] .. offsets[i + 1] - 1 of pts (3 floats a row) and d2; offsets[0] = 0, offsets[n] = *total, and *total is ALWAYS the full
 * count.  The rows of one query come in the library's visiting order - deterministic for a given map state, otherwise unspecified -
 * or, with LII_RADIUS_SORTED in flags, ascending in d2 (equal d2 in unspecified order).
 * Any finite max_dist >= 0 is accepted: 0 returns the points at d2 == 0, and there is no lower bound of 1 - a ball query has none of
 * Nearest_Search's dependence on the shape of the tree, the ball itself is the definition.
 * LII_ERR_INVALID, nothing written: max_dist NaN, infinite or negative; sqrt(max_dist) > 32 map_cell_size (the ball would span more
 * cells than a query should walk - create the handle with a larger lii_config::map_cell_size); a bad stride; NULL queries with n > 0;
 * n < 0; unknown flag bits; NULL offsets or total; a negative capacity (where capacity is read).  No map: LII_ERR_STATE.  n == 0:
 * LII_OK, offsets[0] = 0, total 0.  A query with a NaN coordinate gets an empty segment; one whose ball leaves the addressable grid
 * is searched over the cells that exist.  From inside lii_scan_job::while_waiting: LII_ERR_STATE.
 * Both calls are OBSERVERS in the sense of lii_map_nearest: they end a pre-armed launch and join a map update in flight first; scan,
 * neighbour lists, cached planes, IMU carry and publish order stay as they are; they work with a communicator attached and under
 * LII_TEST=host_solve.
 *   lii_map_radius      host queries, host results, synchronous.  With pts_out == NULL && d2_out == NULL offsets and total only are
 *                       returned and capacity is ignored.  Otherwise capacity (in rows) < *total is LII_ERR_CAPACITY: offsets and
 *                       total are written and nothing else is (the rule of lii_map_box_search).  The queries are counted 65 536 at a
 *                       time and filled in chunks of at most 2^20 rows through the staging of lii_map_nearest, grown geometrically; a
 *                       single query whose ball holds more rows than a chunk gets a chunk to itself, and the staging grows to hold it
 *                       (16 bytes a row, device and pinned: never more than 16 bytes x the live map points beyond the 17 MiB).
 *   lii_map_radius_dev  queries and results in device memory of the caller: enqueued on the handle's stream, returns without waiting.
 *                       offsets_dev (n + 1 words) and total_dev[0] are always complete; rows with index >= capacity are not written -
 *                       the caller compares the total with its capacity behind lii_synchronize.  pts_dev / d2_dev may be NULL (both:
 *                       offsets and total only, capacity ignored).
 * LII_RADIUS_SORTED sorts (query, d2 bits) per row - a non-negative float orders as its uint32 bits - and gathers the points: 24 bytes
 * a row of temporary device memory that belongs to the handle and is created by the first sorted call (the device form sorts
 * `capacity` rows, whatever the total turns out to be: give it the capacity it needs, not a generous bound). */
enum { LII_RADIUS_SORTED = 1 };
int lii_map_radius(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes, double max_dist, int32_t flags,
                   int64_t* offsets_out /* n + 1, required */, float* pts_out /* capacity x 3, may be NULL */,
                   float* d2_out /* capacity, may be NULL */, int64_t capacity, int64_t* total /* required */);
int lii_map_radius_dev(lii_handle h, const void* xyz_dev, int32_t n, int32_t stride_bytes, double max_dist, int32_t flags,
                       int64_t* offsets_dev /* n + 1 */, float* pts_dev, float* d2_dev, int64_t capacity,
                       int64_t* total_dev /* one word */);
/* ---- the surface the map holds at a point: normal, curvature, covariance spectrum of a ball (no counterpart in the reference: PCL's
 * NormalEstimation - computePointNormal, flipNormalTowardsViewpoint, curvature = "surface variation" - and the mean map entropy / mean
 * plane variance of the LiDAR calibration literature are the models).  LII_ABI_VERSION stays 9: everything below is new.
 * Query i (float xyz every stride_bytes, as for lii_map_radius) is answered from EXACTLY the points of its lii_map_radius segment at the
 * same max_dist (a SQUARED distance; float32 calc_dist against it, inclusive): `count` is that segment's length.  The ball is reduced on
 * the device, one wavefront per query, in double and relative to the query:
 *   d = (double)m - (double)q per axis,  s1 = sum d,  s2_ab = sum d_a d_b,
 *   mean_rel = s1 / n,   C_ab = s2_ab / n - mean_rel_a * mean_rel_b          (formed exactly so, no FMA)
 * and C is decomposed by lii_sym3_eigen's routine.  A query's record is the SAME BITS alone or in any batch, in the host or the device
 * form, on every call, for a given map state (fixed-order sums, no atomics).
 * Sign of the normal: viewpoint == NULL - the component of largest magnitude is positive (on a tie the lowest index decides); viewpoint
 * (3 doubles, map coordinates; a HOST pointer in both forms) - normal . (viewpoint - mean) >= 0.
 * The contract is lii_map_radius's: any finite max_dist >= 0; LII_ERR_INVALID with nothing written for max_dist NaN, infinite or negative,
 * sqrt(max_dist) > 32 map_cell_size, a bad stride, n < 0, NULL queries or out with n > 0; no map: LII_ERR_STATE; from inside
 * lii_scan_job::while_waiting: LII_ERR_STATE; n == 0: LII_OK.  A query with a NaN coordinate, or one whose ball reaches no addressable
 * cell, gets count 0, valid 0.  OBSERVERS in the sense of lii_map_nearest: they end a pre-armed launch and join a map update in flight
 * first, write nothing of the registration state, work with a communicator attached and under LII_TEST=host_solve.
 *   lii_map_surface      host queries, host records, synchronous: chunks of 65 536 queries through the staging of lii_map_nearest.
 *   lii_map_surface_dev  queries and records in device memory of the caller: enqueued on the handle's stream, returns without waiting. */
struct lii_surface {  /* 88 bytes, no padding */
  int32_t count;      /* live map points with d2 <= max_dist: lii_map_radius's count, exactly */
  int32_t valid;      /* 1 when count >= 3, else 0: eig, normal and curvature are zeros then */
  double  mean[3];    /* centroid of the ball in map coordinates (q + s1/n); zeros when count == 0 */
  double  eig[3];     /* eigenvalues of C, ascending, negative rounding residue clamped to 0 */
  double  normal[3];  /* unit eigenvector of eig[0] */
  double  curvature;  /* eig[0] / (eig[0] + eig[1] + eig[2]) (PCL's surface variation); 0 when the sum is 0 */
};
int lii_map_surface(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes, double max_dist,
                    const double* viewpoint /* NULL or 3 */, struct lii_surface* out /* n */);
int lii_map_surface_dev(lii_handle h, const void* xyz_dev, int32_t n, int32_t stride_bytes, double max_dist,
                        const double* viewpoint /* NULL or 3, host */, struct lii_surface* out_dev);
/* lii_map_crispness: the whole map's figures - how crisp is the map a calibration produced?  The queries are the map's own live points,
 * enumerated on the device as lii_map_download enumerates them (nothing is downloaded); a point is SELECTED when mix(x, y, z) % every == 0
 * with, over the points' float bits in uint32 arithmetic,
 *   h = bx * 0x9E3779B1u ^ by * 0x85EBCA77u ^ bz * 0xC2B2AE3Du;  h ^= h >> 15
 * - a property of the point, not of where it is stored: two handles that hold the same multiset of points select the same points.  Each
 * point's ball contains the point itself.  A selected point is SPARSE when count < min_count, else DEGENERATE when
 * eig[0] <= 1e-12 * eig[2], else USED: n_selected = n_used + n_sparse + n_degenerate.
 * The surface kernel writes one 24-byte term per selected point into scratch of the handle (created by the first call, grown geometrically,
 * released with the handle; the selection runs through scratch of the map build), and a second launch adds the terms in a fixed order,
 * in double, without atomics: the figures are the same bits on every call for a given map state.
 * LII_ERR_INVALID: min_count < 4, every < 1, NULL out, max_dist as for lii_map_surface.  No map / while_waiting: LII_ERR_STATE.  Observer
 * as lii_map_surface.  An empty selection or n_used == 0: mme = mpv = mean_count = 0. */
struct lii_map_crispness {  /* 56 bytes */
  int64_t n_selected, n_used, n_sparse /* count < min_count */, n_degenerate /* eig[0] <= 1e-12 * eig[2] */;
  double  mme;        /* mean over the used points of 0.5 * (3 ln(2 pi e) + ln eig0 + ln eig1 + ln eig2) */
  double  mpv;        /* mean over the used points of eig[0] */
  double  mean_count; /* mean ball population of the used points */
};
int lii_map_crispness(lii_handle h, double max_dist, int32_t min_count /* >= 4 */, int32_t every /* >= 1 */,
                      struct lii_map_crispness* out);
/* The eigen-solver of the surface statistics, handle-free and on the host (lii_eig3.h: the same source runs on the device): cyclic Jacobi
 * in double, a fixed number of sweeps.  m: xx, xy, xz, yy, yz, zz.  LII_ERR_INVALID: a NULL argument or a non-finite entry. */
int lii_sym3_eigen(const double m[6], double eig[3] /* ascending */, double vec[9] /* row k = eigenvector of eig[k] */);
/* ---- candidate poses scored against the map in one call: the ranking step of a re-localisation (restart in a saved map, flg_reset -
 * src/laserMapping.cpp:895-900 -, recovery after drift), where the caller holds no pose inside the update's convergence basin.
 * For pose k the figures of ONE pass of src/laserMapping.cpp:957-1020, run with nearest_search_en on an all-true selection at the state
 * `base` with rot_end / pos_end replaced by pose k (the extrinsic is base's; cov and the rest are not read): pointBodyToWorld with the
 * registration path's rounding, the exact 5-NN with d2 <= max_match_dist2 inclusive, esti_plane at plane_threshold, pd2 and the gate
 * s > 0.9 (:1001).  total_residual is what :961 / :1022 meant and the reference never accumulates (quirk A13).
 *   res (optional, n_poses x n_down): res[k * n_down + i] = res_last[i] - fabs(pd2) as a float for a selected point, -1000.0f otherwise
 *   (:987).  The cloud is the handle's current down-sampled cloud, the one lii_iekf_iterate would use; the host form's rows are in the
 *   order of lii_scan_download(1), the device form's in the device's order of that cloud.
 * Reads the map and the down-sampled cloud, writes NOTHING of the registration state: neighbour lists, sticky selection, cached planes,
 * point-noise weights, lii_last_unfinished_queries and the publish buffers stay as they were.  Ends a pre-armed launch and joins a map
 * update in flight first.  The host form waits; the _dev form only enqueues on the handle's stream (it waits only where the size of the
 * down-sampled cloud is still on the device, and where the call needs more scratch than any call before it: growing it frees device
 * memory, which waits for the device).  Scratch of the handle's, created by the first call and kept until lii_destroy: the _dev form holds
 * 16 bytes per 64 (pose, point) pairs of its largest call - 128 KiB at 256 poses x 2 048 points, 512 MiB at the limit of 2^31 pairs -,
 * the host form stages chunks of 2^22 pairs (about 50 MiB, device and pinned, with res).
 * DETERMINISTIC: pose k's score and res row are the same bits scored alone or as any member of any batch, in one call or another
 * (fixed-order sums in double, no atomics).
 * LII_ERR_STATE: no map, no down-sampled cloud, inside lii_scan_job::while_waiting, a communicator of more than one rank attached.
 * LII_ERR_INVALID: NULL arguments, n_poses < 1 or > 65 536, n_poses * n_down >= 2^31.
 * A pose with a NaN or Inf entry, or one that puts every point outside the addressable grid, scores {0, 0, 0.0} with every res at -1000;
 * its neighbours in the batch are not disturbed. */
/* (a struct TAG only, no typedef: the record and the call that fills it share their name, which C and C++ allow for a tag and a function
 * and for nothing else - write `struct lii_pose_score`) */
struct lii_pose_score {   /* 16 bytes */
  int32_t n_full;         /* points whose Nearest_Search returned NUM_MATCH_POINTS neighbours (d2 <= max_match_dist2) */
  int32_t effect_num;     /* effect_feat_num of a search pass at this pose (:1013-1020) */
  double  total_residual; /* sum of res_last[i] = |pd2| over the selected points (what :961/:1022 meant); 0 when none */
};
int lii_pose_score(lii_handle h, const lii_state* base, const double* poses /* n_poses x 12: rot_end row-major, pos_end */,
                   int32_t n_poses, struct lii_pose_score* scores, float* res /* NULL, or n_poses x n_down */);
int lii_pose_score_dev(lii_handle h, const lii_state* base, const double* poses_dev, int32_t n_poses,
                       struct lii_pose_score* scores_dev, float* res_dev /* 0 or device */);
/* ---- candidate poses refined against the map in one call: the step behind the ranking.  For pose k the iterated update of
 * src/laserMapping.cpp:957-1134 in LO mode (imu_en = false, :1063-1066) on the six pose states, `updates` times in a row, at the state
 * `base` with rot_end / pos_end replaced by pose k (the extrinsic is base's).  ONE UPDATE starts with state_propagat = the pose it finds,
 * P = the 6 x 6 pose covariance it finds, nearest_search_en = true, rematch_num = 0, and runs up to max_iterations iterations:
 *   pass      every point of the handle's current down-sampled cloud.  Searching: pointBodyToWorld with the registration path's rounding, the
 *             exact 5-NN with d2 <= max_match_dist2 inclusive, the test of :981-984, an all-true selection.  Not searching: the lists and the
 *             sticky selection of this pose's last pass.  Then esti_plane at plane_threshold, pd2 and the gate s > 0.9,
 *             h = [[p_I]x R^T n, n] with p_I = R_LI p + T_LI, z = -pd2, R^-1 = lii_config::laser_point_cov_inv for every point.
 *   solve     G = R^-1 sum h^T h, g = R^-1 sum h^T z, K_1 = (G + P^-1)^-1, v = state_propagat [-] state (Log(R^T R_prop), p_prop - p),
 *             delta = K_1 g + v - K_1 G v, R <- R Exp(delta_rot), p += delta_p  (:1081-1087)
 *   schedule  converged iff |delta_rot| 57.3 < 0.01 and |delta_p| 100 < 0.015; the next pass searches iff converged or (rematch_num == 0 and
 *             iterCount == max_iterations - 2), and rematch_num counts those; with rematch_num >= 2 or iterCount == max_iterations - 1 the
 *             update ends with P <- (I - K_1 G) P  (:1093-1133), stored as its symmetric part 0.5 (P + P^T) - as lii_iekf_update stores
 *             its posterior: the next update's gain relies on P = P^T, and the cov of a record is exactly symmetric, so it is a prior
 *             this call accepts again (a coarse grid, then a fine one around the winner).
 * prior_cov: the 6 x 6 covariance (row-major) every pose starts from; NULL: the pose block cov[0:6, 0:6] of base.  Where that block is
 * uncorrelated with the rest of base->cov (lii_state's initial covariance is the identity) this IS lii_iekf_update(imu_en = 0) on the
 * pose, `updates` times with state_propagat = the state each call finds - and that update leaves the other 18 states alone.  The same
 * definition, the symmetric posterior included; not the same arithmetic (a 6 x 6 elimination here, a 24-state solve there): the two
 * agree in every iteration count and to rounding in the pose (below 1e-9 m on the suite's cases), not bit for bit.
 * An observer, like lii_pose_score: it reads the map and the down-sampled cloud and writes NOTHING of the registration state - neighbour
 * lists, sticky selection, cached planes, point-noise weights, lii_last_unfinished_queries and the publish buffers stay as they were.
 * Ends a pre-armed launch and joins a map update in flight first.  updates x max_iterations rounds of two launches are enqueued at
 * once on the handle's stream - no wait in between; a pose whose last update has ended costs a round one load per workgroup.  The host
 * form stages poses and records through pinned memory and waits once; the _dev form only enqueues (it waits only where the size of the
 * down-sampled cloud is still on the device, and where the call needs more scratch than any call before it).  Scratch of the handle's,
 * created by the first call and kept until lii_destroy: 33 bytes per (pose, point) pair of the largest call (a plane and a selection
 * flag), 232 bytes per 64 pairs, 512 bytes per pose - 18.4 MiB at 256 poses x 2 048 points, 147 MiB at the limit of 2^22 pairs.
 * DETERMINISTIC: pose k's record is the same bits refined alone or as any member of any batch, in one call or another, through either
 * form (fixed-order sums in double, no atomics; a pose reads and writes only its own records).
 * LII_ERR_STATE: no map, no down-sampled cloud, inside lii_scan_job::while_waiting, a communicator of more than one rank attached,
 * lii_point_noise_set's model on (the refinement weighs every point alike; it does not silently differ from the update the caller
 * would otherwise run).
 * LII_ERR_INVALID: NULL arguments (prior_cov excepted), n_poses < 1 or > 65 536, max_iterations outside 1 .. 16, updates outside 1 .. 8,
 * n_poses * n_down > 2^22, a prior - prior_cov, or base's pose block - that is not finite, not symmetric or not positive definite.
 * Nothing is written to `out` by a refused call.
 * A pose with a NaN or Inf entry is returned as given - pose, the prior as cov, the counts 0 - with LII_REFINE_BAD_POSE.  One that puts
 * every point outside the grid selects nothing: each update ends after two iterations exactly where it started, P unchanged.  Neither
 * disturbs its neighbours in the batch. */
enum { LII_REFINE_CONVERGED = 1, LII_REFINE_BAD_POSE = 2 };
/* (a struct tag only, as lii_pose_score) */
struct lii_pose_refined {      /* 408 bytes */
  double  pose[12];            /* rot_end row-major, pos_end - after the last update */
  double  cov[36];             /* the 6x6 pose covariance after the last update, row-major */
  double  total_residual;      /* of the last pass executed: sum of |pd2| over its selected points */
  int32_t effect_num;          /* of the last pass executed */
  int32_t iterations;          /* executed, summed over the updates */
  int32_t searches;            /* search passes executed, summed */
  int32_t flags;               /* LII_REFINE_CONVERGED: the last update ended on rematch_num >= 2, not on the iteration limit;
                                  LII_REFINE_BAD_POSE: a NaN / Inf entry - pose and cov returned as given, the counts 0 */
};
int lii_pose_refine(lii_handle h, const lii_state* base, const double* prior_cov /* NULL or 36 */, const double* poses /* n_poses x 12 */,
                    int32_t n_poses, int32_t max_iterations, int32_t updates, struct lii_pose_refined* out);
int lii_pose_refine_dev(lii_handle h, const lii_state* base, const double* prior_cov /* NULL or 36, host memory */, const double* poses_dev,
                        int32_t n_poses, int32_t max_iterations, int32_t updates, struct lii_pose_refined* out_dev);
/* ---- edits and queries by point and box: the rest of what a holder of the tree can do (include/ikd-Tree/ikd_Tree.h:165-187).
 * lii_map_delete_points <- ikdtree.Delete_Points(PointToDel)  (include/ikd-Tree/ikd_Tree.cpp:479-498, Delete_by_point :672-719,
 *                       same_point :1269-1271).  Every listed point (float xyz every stride_bytes, as for lii_map_build) takes ONE live
 *                       stored point out of the map: one that same_point accepts - per axis the float difference, its fabs compared in
 *                       double against 1e-6.  The map can hold bit-equal twins (lii_map_add_points with downsample_on = 0 stores what it
 *                       is given): a list that holds a point c times removes min(c, stored copies) of them, wherever in the list the
 *                       copies stand; *n_deleted is the number actually removed.  The work follows the LIST, not the map: a listed point
 *                       looks at the one to eight cells it can match in.
 *                       Unspecified: among stored points that are not bit-equal but lie within 2e-6 of each other on every axis, which of
 *                       them a listed point takes - and, when several listed points compete for them, how many go (the reference takes the
 *                       first on its descent: its answer depends on the shape of its tree).  A listed point with a NaN or infinite
 *                       coordinate matches nothing.  A listed point that is not in the map is not an error; n == 0 or an empty map: LII_OK,
 *                       count 0.  LII_ERR_INVALID, nothing changed: a bad stride, NULL with n > 0, n < 0.  n is unbounded: the list goes
 *                       through the handle's staging in chunks of at most 65 536 points, the chunks in order.
 *                       Everything else is as lii_map_delete_boxes: the call ends a pre-armed launch and joins a map update in flight
 *                       (never a map with parked inserts), drops the neighbour lists and cached planes when something went, works with a
 *                       communicator attached (the maps are replicated: give every rank the same list) and under LII_TEST=host_solve.
 *                       While lii_map_removed_set is in force the points it removes go into the history buffer (see there).
 * lii_map_delete_points_dev  the list lies in device memory of the caller (lii_dev_alloc, a tensor's data_ptr): enqueued on the handle's
 *                       stream, returns without waiting.  Nobody knows yet whether anything went, so the neighbour lists and planes of an
 *                       earlier search are not used again (the rule of lii_local_map_segment(out == NULL)); lii_map_size behind it reads
 *                       the result.
 * lii_map_range       <- ikdtree.tree_range()  (ikd_Tree.cpp:90-118): the exact float minimum and maximum of the live points per axis -
 *                       min xyz, max xyz; the same bits on every run (-0 counts as below +0).  An empty map: six zeros and LII_OK, as the
 *                       reference's memset on a null root.  Waits for the stream.
 * lii_map_box_search  <- ikdtree.Search_by_range  (ikd_Tree.cpp:970-998; the tree's own box query, the one Add_Points down-samples with)
 *                       for n_boxes <= 4096 boxes of 6 floats (min xyz, max xyz): the live points with min <= p < max on every axis in
 *                       at least one box - the rule of lii_map_delete_boxes -, a point that lies in several boxes once.  Packed xyz in
 *                       unspecified order.  Capacity as for lii_map_download: *n is ALWAYS the full count; xyz_out == NULL returns the
 *                       count only; capacity < *n is LII_ERR_CAPACITY and nothing is written.  Zero boxes or an empty map: *n = 0.
 * lii_map_range and lii_map_box_search are OBSERVERS in the sense of lii_map_nearest: neighbour lists, IMU carry and publish order stay;
 * they end a pre-armed launch and join a map update in flight first.
 * NOT offered: Add_Point_Boxes (ikd_Tree.cpp:458-477, Add_by_range :721-767).  In the reference it un-deletes only those lazily deleted
 * nodes that no rebuild has flattened away yet: its answer depends on the shape of the tree, and the device map squeezes deleted points
 * out at once.  The library refuses rather than invent a rule; re-insert the points (lii_map_removed_acquire keeps them) with
 * lii_map_add_points. */
int lii_map_delete_points(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes, int32_t* n_deleted /* may be NULL */);
int lii_map_delete_points_dev(lii_handle h, const void* xyz_dev, int32_t n, int32_t stride_bytes);
int lii_map_range(lii_handle h, float range6[6] /* min xyz, max xyz */);
int lii_map_box_search(lii_handle h, const float* boxes, int32_t n_boxes, float* xyz_out, int32_t capacity, int32_t* n);
/* ---- map points keep their intensity.  The reference's tree stores whole PointType values: map_incremental pushes feats_down_world[i]
 * (src/laserMapping.cpp:516-559), into which pointBodyToWorld has copied the intensity (:219); Add_Points keeps downsample_result, a whole
 * point - the new one or a stored one (include/ikd-Tree/ikd_Tree.cpp:381-456); Nearest_Search (:349-379), Search_by_range (:970-998),
 * flatten (:1229-1251) and acquire_removed_points (:522-534) hand whole points back.  The device map's records are float4: the fourth
 * word is the point's intensity.
 * RULE.  A stored point's intensity is the intensity of the input point that the existing rules keep - through every layer that moves,
 * chooses, squeezes, parks, rebuilds or returns a map point.  No rule that decides which xyz survives changes; where such a choice is
 * unspecified (bit-equal twins, equal d2) the intensity that goes with it is unspecified in the same way.  Points stored through
 * lii_map_build and lii_map_add_points - and, while lii_map_intensity_set is off, through lii_map_build_from_scan, lii_map_incremental and
 * a registration's own map update - carry 0.0f: lii_publish_saved_pcd's convention for "none kept".  LII_ABI_VERSION stays 9: every
 * entry point below is new.
 * Scan-driven updates:
 *   lii_map_intensity_set / lii_map_intensity_get  durable handle state, OFF by default.  ON: the updates a scan feeds - lii_map_incremental
 *                            (src/laserMapping.cpp:516-559), a registration's own lii_scan_job::map_update, lii_map_build_from_scan (:921-931)
 *                            - take each inserted point's intensity from the down-sampled cloud's (what pointBodyToWorld copies, :219; the
 *                            values lii_scan_intensity_download(h, 1) returns): one more load per inserted point, no launch added.  A cloud
 *                            that carried none (nothing attached when the voxel filter ran; a job that adopted scan_dev) stores 0.0f.  The
 *                            world points of lii_scan_download(h, 2) keep their fourth float 0.  OFF: those calls enqueue exactly the launches
 *                            and instantiations they did before the switch existed.
 *                            Refusals.  LII_ERR_STATE: a communicator is attached (single rank for now; lii_comm_init / lii_comm_init_ex on
 *                            a handle with the switch on refuse likewise); from inside lii_scan_job::while_waiting.  LII_ERR_INVALID: on
 *                            not 0 / 1, NULL arguments.  It works under LII_TEST=host_solve (where no intensities can be attached: zeros).
 *                            A job on such a handle keeps its pre-armed prologue: the map update is not part of it.
 *   A handle whose map may hold intensities - an _xyzi input, or the switch, since the last lii_map_reset / lii_map_build - runs the
 *   carrying instantiations of the fold and insert kernels in every later update, 3-float batches and recoveries included (same results:
 *   their fourth word is 0), until lii_map_reset or lii_map_build starts an empty or plain map.
 * Inputs:
 *   lii_map_build_xyzi       <- ikdtree.Build(feats_down_world->points), src/laserMapping.cpp:921-931: lii_map_build, plus a float read
 *                            at intensity_offset bytes into each record (12 with stride 16 for packed xyzi, 32 with stride 48 for
 *                            pcl::PointXYZINormal, include/common_lib.h:37).
 *   lii_map_add_points_xyzi  <- ikdtree.Add_Points(PointToAdd, downsample_on), ikd_Tree.cpp:381-456: lii_map_add_points likewise.  With
 *                            down-sampling the voxel keeps its closest-to-centre point WITH that point's intensity (downsample_result,
 *                            :400-420); a stored point that wins keeps its own.
 *   LII_ERR_INVALID, nothing changed: an intensity_offset that is negative, not a multiple of 4, overlaps x / y / z (< 12) or has
 *   offset + 4 > stride_bytes; everything lii_map_build / lii_map_add_points refuse.  A NaN intensity is stored as given, bit for bit: only
 *   coordinates decide anything.
 * Outputs - each is its sibling with 4 floats a row (x, y, z, intensity) where the sibling has 3: the same counts, order rules,
 * capacities (in rows), errors and observer guarantees; they return the stored word whatever entry point stored it:
 *   lii_map_download_xyzi         <- flatten / PCL_Storage (ikd_Tree.cpp:1229-1251)
 *   lii_map_nearest_xyzi, lii_map_nearest_xyzi_dev  <- Nearest_Points[i].intensity of Nearest_Search (ikd_Tree.cpp:349-379); the rows from
 *                                 count[i] on are zeros
 *   lii_map_radius_xyzi, lii_map_radius_xyzi_dev    <- the ball query, LII_RADIUS_SORTED included
 *   lii_map_box_search_xyzi       <- Search_by_range (ikd_Tree.cpp:970-998)
 *   lii_map_removed_acquire_xyzi  <- acquire_removed_points (ikd_Tree.cpp:522-534) / _featsArray (src/laserMapping.cpp:249-254)
 *   The host forms of nearest and radius stage 20 bytes a row through the buffers of their siblings (16 a row there): their chunks are cut
 *   at four fifths of the siblings' rows, the buffers keep their bound.
 * lii_map_pcd <- publish_map / featsFromMap (src/laserMapping.cpp:638-645: the save of the down-sampled map the reference meant and never
 *               fills) as pcd_writer.writeBinary (:609) would write it: the live map as the 32-byte rows lii_pcd_header describes - x y z,
 *               normals 0, intensity the stored word, curvature 0 - in lii_map_download's order rule (none).  Gathered and repacked on the
 *               device, brought over through the staging of lii_publish_saved_pcd, 65 536 rows at a time.  *n_points is ALWAYS the live
 *               count; rows_out == NULL returns the count only; capacity_bytes < 32 x *n_points is LII_ERR_CAPACITY and nothing is
 *               written.  An OBSERVER in the sense of lii_map_nearest; from inside lii_scan_job::while_waiting: LII_ERR_STATE. */
int lii_map_build_xyzi(lii_handle h, const void* pts, int32_t n, int32_t stride_bytes, int32_t intensity_offset);
int lii_map_add_points_xyzi(lii_handle h, const void* pts, int32_t n, int32_t stride_bytes, int32_t intensity_offset,
                            int32_t downsample_on, int32_t* n_added);
int lii_map_download_xyzi(lii_handle h, float* xyzi_out, int32_t capacity, int32_t* n);
int lii_map_nearest_xyzi(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes, int32_t k, double max_dist,
                         float* pts_out /* n*k*4 */, float* d2_out /* n*k */, int32_t* count_out /* n */);
int lii_map_nearest_xyzi_dev(lii_handle h, const void* xyz_dev, int32_t n, int32_t stride_bytes, int32_t k, double max_dist,
                             float* pts_dev, float* d2_dev, int32_t* count_dev);
int lii_map_radius_xyzi(lii_handle h, const void* xyz, int32_t n, int32_t stride_bytes, double max_dist, int32_t flags,
                        int64_t* offsets_out /* n + 1, required */, float* pts_out /* capacity x 4, may be NULL */,
                        float* d2_out /* capacity, may be NULL */, int64_t capacity, int64_t* total /* required */);
int lii_map_radius_xyzi_dev(lii_handle h, const void* xyz_dev, int32_t n, int32_t stride_bytes, double max_dist, int32_t flags,
                            int64_t* offsets_dev /* n + 1 */, float* pts_dev, float* d2_dev, int64_t capacity,
                            int64_t* total_dev /* one word */);
int lii_map_box_search_xyzi(lii_handle h, const float* boxes, int32_t n_boxes, float* xyzi_out, int32_t capacity, int32_t* n);
int lii_map_removed_acquire_xyzi(lii_handle h, float* xyzi_out, int32_t capacity, int32_t* n, int32_t clear);
int lii_map_pcd(lii_handle h, void* rows_out, int64_t capacity_bytes, int32_t* n_points);
int lii_map_intensity_set(lii_handle h, int32_t on);
int lii_map_intensity_get(lii_handle h, int32_t* on);

/* ---------------------------------------------------------------- scan in / undistortion / down-sampling
 * lii_scan_upload: host AoS -> device float4 (x,y,z,t_ms).  For pcl::PointXYZINormal use stride 48,
 *                  time_offset_bytes 36 (`curvature`, include/common_lib.h:37).  Replaces the hand-over of
 *                  Measures.lidar to ImuProcess::Process (src/laserMapping.cpp:909).
 * lii_scan_set_device: same, from a device-resident float4 buffer (copied on the handle's stream by the kernel that also
 *                  reduces the scan's time extent; the caller's buffer is only read and free again once a later call on
 *                  the handle has returned).
 * ORDER OF THE POINTS.  The reference sorts every scan by time before it de-skews it (std::sort by curvature,
 *                  src/IMU_Processing.hpp:209, :287; its preprocess hands the scan over sorted as well,
 *                  src/preprocess.cpp:296-302) and everything downstream sees that order.  The library sorts ONLY WHEN ASKED: the
 *                  de-skew itself does not need it (the time-earliest point is found by a reduction), but the voxel-grid
 *                  centroids are float sums in input order, so results are bit-identical to the reference's only for a
 *                  scan in ascending time order (equal stamps in the reference's order) - which is what the cutting
 *                  lii_ingest_* / lii_frame_select deliver.  An unsorted scan registered as it is comes out correct up to the
 *                  rounding of those sums (~1e-6 m per centroid).  To get the reference's bits for it, have the library sort it
 *                  on the device: lii_scan_job::scan_sorted = 2 inside a registration, or lii_scan_sort as a call of its own.
 * lii_scan_sort:   puts the handle's current scan (lii_scan_upload / lii_scan_set_device / lii_scan_advance / lii_frame_select)
 *                  into ascending time order, on the device: one key launch, a stable radix sort of (key, index), one gather
 *                  launch into another buffer of the handle (a selected ingest frame is only read).  The order is ascending t,
 *                  compared as floats, STABLE: equal stamps keep their input order (the reference's std::sort leaves it
 *                  unspecified; the ingest fixes it the same way), and -0.0f and +0.0f are equal stamps - they are not
 *                  reordered.  All four floats of a point travel unchanged.  A NaN stamp is outside the contract: any order,
 *                  but every point still appears exactly once.  Afterwards lii_scan_download(h, 0, ...) returns the sorted
 *                  scan and a registration may state scan_sorted = 1.  For callers of lii_undistort_* + lii_downsample +
 *                  lii_iekf_update.  No scan: LII_ERR_STATE; one point: LII_OK, nothing to do; a communicator attached:
 *                  LII_ERR_STATE (a sharded job cannot sort for now).  The buffers of the sort (36 bytes per point of
 *                  max_scan_points + the radix sort's temporary storage) are allocated by the handle's first sort, not by
 *                  lii_create.  The voxel filter emits the down-sampled cloud in the order of the
 *                  voxels' first points; lii_scan_download(1 / 2) and lii_neighbors_download return the reference's order
 *                  (ascending PCL voxel index).
 * lii_undistort_imu <- back-propagation loop of ImuProcess::propagation_and_undist, src/IMU_Processing.hpp:390-414
 * lii_undistort_cv  <- CV de-skew of Forward_propagation_without_imu,            src/IMU_Processing.hpp:246-266
 * lii_downsample    <- downSizeFilterSurf.filter(*feats_down_body),              src/laserMapping.cpp:917-919
 *                      (n_down == NULL && filtered == NULL: fully asynchronous — the result size stays on the device)
 * lii_downsample_skip: use the (undistorted) scan as feats_down_body unchanged (PCL's overflow-identity path).
 * lii_scan_download: which = 0 undistorted scan, 1 down-sampled body points, 2 world points of the last iteration.
 * lii_scan_upload_next / lii_scan_advance: the scan queue of the reference (lidar_buffer, src/laserMapping.cpp:331-366 ->
 *                  sync_packages :432-480) one element deep, on the device.  lii_scan_upload_next starts the NEXT scan on its
 *                  way (same arguments as lii_scan_upload) into a second device buffer on the library's copy stream and returns
 *                  at once: the transfer overlaps the registration / map update of the current scan.  A source in pinned host
 *                  memory with stride 16 / time offset 12 is read by the copy engine directly and must stay untouched until
 *                  lii_scan_advance has returned; any other source is staged (copied before the call returns).
 *                  lii_scan_advance makes that scan the current one (as lii_scan_upload would have): waits for its transfer,
 *                  swaps the buffers.  LII_ERR_STATE without a pending lii_scan_upload_next. */
int lii_scan_upload(lii_handle h, const void* points, int32_t n, int32_t stride_bytes, int32_t time_offset_bytes);
int lii_scan_upload_next(lii_handle h, const void* points, int32_t n, int32_t stride_bytes, int32_t time_offset_bytes);
int lii_scan_advance(lii_handle h);
int lii_scan_set_device(lii_handle h, const void* dev_float4, int32_t n);
int lii_scan_sort(lii_handle h);
int lii_undistort_imu(lii_handle h, const lii_pose6d* poses, int32_t n_poses, const double end_R[9],
                      const double end_p[3], const double R_LI[9], const double T_LI[3]);
int lii_undistort_cv(lii_handle h, const double omega[3], const double vel[3], const double end_R[9]);
int lii_downsample(lii_handle h, float leaf, int32_t* n_down, int32_t* filtered);
int lii_downsample_skip(lii_handle h, int32_t* n_down);
int lii_scan_download(lii_handle h, int32_t which, float* out_float4, int32_t capacity, int32_t* n);

/* ---------------------------------------------------------------- the intensity channel (optional, off until asked for)
 * What the reference hands on with every point (pointBodyToWorld copies it, src/laserMapping.cpp:219; PCL's VoxelGrid averages it with
 * every other field) travels BESIDE the float4 clouds: one float per point in buffers of the handle's own, created by the first call that
 * attaches intensities.  Every stage that reorders, drops, merges or republishes points carries it: the ingest's filters, sort and cut,
 * the time sort (lii_scan_sort, scan_sorted = 2), the voxel filter in all its forms (per output voxel PCL's centroid: the members'
 * intensities added in input order from 0.f, divided by the count - the arithmetic of x, y, z, t; the unfiltered pass-through and
 * lii_downsample_skip copy), and lii_publish_* (LII_PUB_INTENSITY).  A scan without intensities enqueues the launches and gives the bits it
 * did before the channel existed.
 *   lii_scan_intensity_upload      attaches intensities to the CURRENT scan from the caller's AoS (pcl::PointXYZINormal: stride 48, offset 32).
 *                                  n must be the current scan's point count (else LII_ERR_INVALID); no scan: LII_ERR_STATE.
 *   lii_scan_intensity_set_device  the same from device memory (n floats, copied on the handle's stream; the caller's buffer is only read).
 *   lii_ingest_set_intensity       a STANDING ORDER on the ingest (off by default): every lii_ingest_pcl2 / lii_ingest_livox / *_begin call
 *                                  from then on also forms the intensity of every frame point (one launch behind the cut), and
 *                                  lii_frame_select makes the frame's intensities those of the current scan.  VELO, OUSTER and PANDAR hold a
 *                                  float, copied bit for bit; ROBOSENSE `intensity` and Livox `reflectivity` are uint8, converted to float
 *                                  (src/preprocess.cpp:69,149,198,222,262); L515 has no such field: 0.0f.
 *   lii_scan_intensity_download    which = 0: the current scan's intensities in the scan's current order; which = 1: the down-sampled
 *                                  cloud's, in the order lii_scan_download(h, 1) returns its points (PCL's).  Nothing attached (for 1: not
 *                                  attached when the voxel filter ran): LII_ERR_STATE.  out may be NULL (*n only).
 * LIFETIME.  Intensities belong to the current scan, and whatever REPLACES the current scan detaches them: lii_scan_upload,
 * lii_scan_set_device, lii_scan_advance (a scan that arrived through lii_scan_upload_next has none), lii_frame_select of a frame ingested
 * without the order, and a job that adopts lii_scan_job::scan_dev.  A caller registering a device-resident scan WITH intensity hands it over
 * with lii_scan_set_device + lii_scan_intensity_set_device and leaves job->scan_dev NULL; jobs with scan_dev / next_scan_dev - and with them
 * the pre-armed prologue - know nothing of the channel.  De-skew and sort keep them (the same points, moved).
 * With a communicator attached, or under LII_TEST=host_solve, the attaching calls (and lii_ingest_set_intensity(h, 1)) return LII_ERR_STATE.
 * Like every entry point they end a pre-armed launch first. */
int lii_scan_intensity_upload(lii_handle h, const void* points, int32_t n, int32_t stride_bytes, int32_t intensity_offset_bytes);
int lii_scan_intensity_set_device(lii_handle h, const void* dev_float, int32_t n);
int lii_ingest_set_intensity(lii_handle h, int32_t on);
int lii_scan_intensity_download(lii_handle h, int32_t which, float* out, int32_t capacity, int32_t* n);

/* ---------------------------------------------------------------- ingest: driver message -> device-resident scan frames
 * lii_ingest_pcl2  <- Preprocess::process_cut_frame_pcl2  (src/preprocess.cpp:115-335; callers laserMapping.cpp:363-372)
 * lii_ingest_livox <- Preprocess::process_cut_frame_livox (src/preprocess.cpp:50-113;  callers laserMapping.cpp:326-336)
 * ... and, with lii_ingest_opts::cut_frame_num = 0, the callbacks' branch for `initialization/cut_frame: false`
 *                     (laserMapping.cpp:337-342, :374-379): Preprocess::process - oust_handler / velodyne_handler / l515_handler
 *                     (PointCloud2; any other lidar_type is "Error LiDAR Type" there, LII_ERR_INVALID here) and avia_handler
 *                     (CustomMsg), src/preprocess.cpp:337-713 - with feature extraction disabled unless lii_ingest_set_features
 *                     (below) turned it on: the handler's filters (they are not
 *                     the cutting functions' in every detail: velodyne_handler has no ring test), no time sort, no cut - ONE frame
 *                     holding pl_surf in input order, its first point included, begin_time_s = header.stamp; hand such a frame to
 *                     lii_scan_register with scan_sorted = 2 (sorted on the device first: the reference's bits - its
 *                     ImuProcess::Process sorts the frame, src/IMU_Processing.hpp:209, :287) or with scan_sorted = 0 (registered
 *                     in input order: no sort, the centroids' rounding differs).  An empty cloud yields no frame (the node skips it, laserMapping.cpp:909-914).
 * `data` is sensor_msgs/PointCloud2::data (or the CustomPoint array) as received; the field offsets are what
 * pcl::fromROSMsg derives from msg->fields for the point structs of src/preprocess.h:35-116 (types per lidar_type:
 * VELO time f32 [s] / ring u16; OUSTER t u32 [ns] / ring u8; PANDAR timestamp f64 / ring u16; ROBOSENSE timestamp f64 /
 * ring u16 / intensity u8; intensity is not part of the float4 records — nothing on the path reads it — and is carried beside them only
 * under lii_ingest_set_intensity, below).  Decode, blind / NaN / ring /
 * point_filter_num filters, azimuth time synthesis for clouds without per-point time (:163-185), time sort and the
 * sub-frame cut (:296-334) run on the device; the frames stay there.  frames[k].begin_time_s is the value the caller
 * pushes to time_buffer (time_lidar / 1000), offset/count index the handle's frame buffer.
 * Equal time stamps keep their input order (the reference's std::sort leaves that order unspecified).
 * lii_frame_select: frame k becomes the current scan (what lidar_buffer.front() -> meas.lidar -> lii_scan_upload did). */
enum { LII_LIDAR_AVIA = 1, LII_LIDAR_VELO = 2, LII_LIDAR_OUSTER = 3, LII_LIDAR_L515 = 4, LII_LIDAR_PANDAR = 5,
       LII_LIDAR_ROBOSENSE = 6 }; /* LID_TYPE, include/common_lib.h:55 */
typedef struct lii_pc2_fields {
  int32_t point_step; /* bytes per point record */
  int32_t x, y, z, intensity, time, ring; /* byte offsets */
} lii_pc2_fields;
typedef struct lii_livox_fields {
  int32_t point_step;
  int32_t offset_time, x, y, z, reflectivity, tag, line; /* byte offsets (livox_ros_driver/CustomPoint.msg) */
} lii_livox_fields;
typedef struct lii_ingest_opts {
  uint32_t struct_size;     /* sizeof(lii_ingest_opts) */
  int32_t lidar_type;       /* LII_LIDAR_* (preprocess/lidar_type) */
  int32_t n_scans;          /* N_SCANS (preprocess/scan_line) */
  int32_t point_filter_num; /* point_filter_num */
  double blind;             /* preprocess/blind [m] */
  double stamp_s;           /* msg->header.stamp.toSec() */
  int32_t cut_frame_num;    /* required_frame_num (initialization/cut_frame_num), <= 64; 0: do not cut (initialization/cut_frame: false) */
  int32_t scan_count;       /* the caller's scan_count: the first 20 (PointCloud2) / 5 (Livox) messages are not cut */
} lii_ingest_opts;
typedef struct lii_frame_info {
  double begin_time_s;   /* time_lidar / 1000 */
  double last_offset_ms; /* curvature of the frame's last point: lidar_end_time = begin + this / 1000 (laserMapping.cpp:452-456) */
  int32_t offset, count;
} lii_frame_info;
int lii_ingest_pcl2(lii_handle h, const void* data, int32_t n_points, const lii_pc2_fields* fields, const lii_ingest_opts* opts,
                    lii_frame_info* frames, int32_t max_frames, int32_t* n_frames);
int lii_ingest_livox(lii_handle h, const void* points, int32_t n_points, const lii_livox_fields* fields,
                     const lii_ingest_opts* opts, lii_frame_info* frames, int32_t max_frames, int32_t* n_frames);
int lii_frame_select(lii_handle h, int32_t frame);
/* The overlapped forms (ABI 9) - the reference's message queue (lidar_buffer / time_buffer filled by the callbacks, src/laserMapping.cpp:326-379,
 * drained by sync_packages, :432-480) kept ON THE DEVICE: lii_ingest_*_begin puts a message under way (H2D of the raw bytes on a copy stream,
 * decode ... cut on a stream of its own) and returns without waiting; lii_ingest_end waits for the OLDEST message under way (long
 * done when it overlapped a registration), makes its frames the ones lii_frame_select serves and returns its frame table exactly as the
 * one-call form does.  Up to two messages may be under way (LII_ERR_STATE for a third); the frames of the message before stay selectable until
 * lii_ingest_end.  Call order of a single-threaded host: lii_ingest_end(m) -> register the sub-frames of m -> lii_ingest_*_begin(m + 2): the
 * begin's launches are then enqueued while the device still runs the map update of m's last sub-frame.  `data` must stay valid until the matching lii_ingest_end; from page-locked memory the transfer is asynchronous, from pageable
 * memory the call returns once the runtime has staged the bytes (the launches still overlap).  Results are the one-call forms' bits. */
int lii_ingest_pcl2_begin(lii_handle h, const void* data, int32_t n_points, const lii_pc2_fields* fields, const lii_ingest_opts* opts);
int lii_ingest_livox_begin(lii_handle h, const void* points, int32_t n_points, const lii_livox_fields* fields, const lii_ingest_opts* opts);
int lii_ingest_end(lii_handle h, lii_frame_info* frames, int32_t max_frames, int32_t* n_frames);
/* Feature extraction (preprocess/feature_extract_en): Preprocess::give_feature :715-965, plane_judge :976-1071, edge_jump_judge :1073-1102
 * and the feature branches of avia_handler :373-418, oust_handler :487-536 and velodyne_handler :585-652, on the device.
 *   lii_ingest_set_features      a STANDING ORDER like lii_ingest_set_intensity, off by default.  With it on, a whole-message ingest
 *                                (cut_frame_num == 0) of AVIA, VELO or OUSTER - one-call or overlapped form - returns ONE frame holding
 *                                pl_surf of the feature branch: lines ascending, positions ascending within a line; begin_time_s = stamp_s,
 *                                last_offset_ms = the curvature of its last point; an empty pl_surf yields no frame.  point_filter_num
 *                                acts in the emission only (every point_filter_num-th point of a plane run, the float mean of an
 *                                unfinished remainder); 1 <= n_scans <= 128 (else LII_ERR_INVALID).  Every other ingest is unaffected:
 *                                any cut_frame_num > 0, and L515.  Under lii_ingest_set_intensity such a frame's intensities are all
 *                                0.0f (the emitted surface points carry x, y, z and curvature only).  Messages under way keep what
 *                                they were enqueued with.  The buffers the extraction needs are created by the first message that is
 *                                ingested under the order; a handle that never hears of it holds what it held before.
 *   lii_ingest_corners_download  pl_corn of the message whose frames are current (Edge_Jump / Edge_Plane points, whole): x, y, z,
 *                                curvature per point into xyzt, the points' intensities into `intensity`; either may be NULL, both NULL
 *                                return *n only.  With the order off, or before any such message: *n = 0, LII_OK.
 *   lii_ingest_features_get      the order, and of the message whose frames are current: pl_surf.size(), pl_corn.size() and the number of
 *                                lines the passes ran on (0 for a message that did not go through the feature branch).
 * Every decision is an IEEE add / mul / div / sqrt in the reference's types and order; results are the reference's bits wherever the
 * reference defines them.  It does NOT define them in these places, and the library does:
 *   - Preprocess::disB is never initialised (src/preprocess.cpp:15-16 sets disA twice), yet plane_judge adds it: it is 0 here.
 *   - types[plsize - 1].dista is never written, yet plane_judge pushes it into disarr whenever a group runs to the end of its line
 *     (:1008): it is 0 here.  (What a node's first message sees when its heap is fresh; later messages there see recycled memory.)
 *   - `while (types[head].range < blind) head++` (:724) runs off a line that is blind throughout: nothing is emitted for that line.
 *   - an empty OUSTER line indexes types[-1] (:534): it yields nothing.
 *   - in the edge-jump pass vecs[j] stays unset beside a blind neighbour (:846-853) and `intersect` is formed from it (:866): it is the
 *     zero vector here - the quotient is NaN and every comparison with it is false.
 *   - a plane group that runs to the end of its line marks types[plsize] (:750-756): only the points the line has are marked here.
 * NULL handle / bad arguments: LII_ERR_INVALID; from inside lii_scan_job::while_waiting: LII_ERR_STATE.  Like every entry point they end a
 * pre-armed launch first. */
int lii_ingest_set_features(lii_handle h, int32_t on);
int lii_ingest_corners_download(lii_handle h, float* xyzt, float* intensity, int32_t capacity, int32_t* n);
int lii_ingest_features_get(lii_handle h, int32_t* on, int32_t* n_surf, int32_t* n_corn, int32_t* n_lines);

/* ---------------------------------------------------------------- scan-to-map registration
 * lii_iekf_iterate: ONE pass of the per-point loop + Jacobian + normal-equation reduction at a fixed state —
 *   pointBodyToWorld :209-220, Nearest_Search :980, esti_plane :997, residual/selection :987-1011,
 *   Jacobian rows :1035-1071, H^T R^-1 H / H^T R^-1 z :1073-1080 (src/laserMapping.cpp).
 *   out91 = upper triangle (78) of the 12x12, then 12, then effect_feat_num.  With a communicator attached
 *   (lii_comm_init) out91 is the all-reduced sum over ranks.
 * lii_iekf_update: the whole loop :957-1134 including the 24-state solve (:1081-1087), convergence / rematch
 *   logic (:1093-1106) and covariance update (:1109-1131).  The loop is device resident: every pass is enqueued up
 *   front, the kernels consult a control block in HBM and skip the passes the reference's schedule does not run, the
 *   final state lands in mapped host memory followed by a sequence word the call waits for — one host round trip per
 *   call, and the call returns as soon as the result exists: passes still queued behind the stopping one (they read a flag
 *   and return) drain in stream order while the caller goes on; every later call on the handle is ordered behind them.
 *   (LII_TEST=sync_result waits for the whole stream instead.  LII_TEST=host_solve drives the loop from the host
 *   around lii_iekf_iterate with the literal two-inversion algebra.)
 * lii_neighbors_download: Nearest_Points of the last search (for map_incremental, :525-549);
 *   pts = n_down x 5 x 3 floats, counts = n_down. */
int lii_iekf_iterate(lii_handle h, const lii_state* state, int32_t search, int32_t imu_en, double out91[91]);
int lii_iekf_update(lii_handle h, lii_state* state, const lii_state* state_propagated, const lii_iekf_opts* opts,
                    lii_iekf_report* report);
int lii_neighbors_download(lii_handle h, float* pts, int32_t* counts, uint8_t* selected, int32_t capacity);
/* How the last device-resident update solved its passes: *pivoted_passes = the passes (of the first 16) whose 12 x 12 elimination left the
 * pivot-free form for the routine with row exchanges (its element growth exceeded 2^8, or a pivot was zero).  The reference inverts
 * with Eigen's partial-pivoting LU every time (src/laserMapping.cpp:1081-1085); the result is held to the same tolerance either way -
 * the count exists so that tests can tell which routine they exercised. */
int lii_last_solve_info(lii_handle h, int32_t* pivoted_passes);
/* How many queries the most recent search pass could not finish inside its own launch - their 5th neighbour lies beyond what the
 * 3 x 3 x 3 cells around the query can prove: the reference's tree walks on into farther boxes for them (include/ikd-Tree/
 * ikd_Tree.cpp:827-842) - and left to the fit launch behind it (ABI 8).  Up to 256 per launch are finished by completion workgroups of
 * their own; beyond that a launch of its own finishes the listed ones (up to 4096, one wavefront each) when the scan before was in that
 * regime too, and every workgroup finishes its own points' otherwise.  ABI 9: behind lii_iekf_update / lii_scan_register on one rank the value
 * is the LARGEST count among the update's search passes and comes with the result (no device read); otherwise the most recent search
 * launch's (one small device read, synchronises the handle's stream). */
int lii_last_unfinished_queries(lii_handle h, int32_t* n_last);

/* ---- per-point measurement noise from range and bearing.  src/laserMapping.cpp:1039-1042 forms a 3 x 3 covariance for every selected
 * point - calcBodyVar(point_this, 0.02, 0.05, var) (:158-181): range_var along the ray plus a bearing term across it, rotated into the world
 * frame by rot_end - and :1050 discards it: R_inv(i) = 1000 for every point, whose square root :1051 stores as the effect cloud's intensity.
 * This is the model its authors meant, switched on by choice.  LII_ABI_VERSION stays 9: everything below is new.
 * THE DEFECT.  calcBodyVar builds the basis of the ray's tangent plane as base_vector1 = (1, 1, -(dx + dy) / dz) (:170-171): NaN for any
 * point with z = 0 in the IMU frame - a spinning LiDAR's horizontal ring - so the literal form cannot be switched on.
 * THE CLOSED FORM.  The update needs only n^T (R_end var R_end^T) n.  With p_I = R_LI p_L + T_LI (:1039), t = R_end^T n (n: the float-cast
 * normal the Jacobian reads back, :1047-1048), A = p_I x t (the row's first three columns), u = t . p_I, r^2 = |p_I|^2:
 *     sigma^2_i = 1 / laser_point_cov_inv + sr2 u^2 / r^2 + s2 |A|^2        (the radial term 0 when r^2 == 0)
 *     R_inv_i   = 1 / sigma^2_i
 * because N = [base_vector1, base_vector2] (:170-177) is an orthonormal basis of the tangent plane, so A diag(s2) A^T = s2 r^2 (I - d d^T)
 * (:178-180) whatever basis is chosen.  Finite everywhere; all arithmetic in double.  The two constants are formed once per
 * lii_point_noise_set:  sr2 = (double)((float)range_inc * (float)range_inc) - range_inc and range_var are floats in calcBodyVar (:158-161) - and
 * s2 = sin((double)(float)degree_inc * 0.017453293)^2 (:163-164), the constant being PCL's DEG2RAD macro as the reference compiles it (restated
 * from knowledge of PCL, not pinned by a build).
 *   lii_point_noise           <- the arguments of calcBodyVar at :1041.  model 0 (default): R_inv = lii_config::laser_point_cov_inv for every
 *                             point, :1050 - every launch, instantiation and result as before the setting existed.  model 1: the above.
 *   lii_point_noise_set       a standing setting of the handle, like lii_map_intensity_set; m == NULL: model 0.  Honoured by every fit pass,
 *                             search or cached-plane, of lii_iekf_iterate, lii_iekf_update, lii_scan_register, lii_scan_register_imu,
 *                             lii_scan_register_cv and LII_TEST=host_solve (<- :1039-1050 inside the loop :957-1134: the weights are a function
 *                             of the current state, recomputed by every pass).  The two gates (:987-1011) and effect_feat_num do not look at them.
 *                             The buffer behind lii_point_noise_download is created by the first call with model 1.  Ends a pre-armed launch first.
 *                             LII_ERR_INVALID: NULL handle, struct_size != sizeof(lii_point_noise), a model other than 0 / 1, a negative or
 *                             non-finite constant.  LII_ERR_STATE: a communicator is attached (single rank only for now; lii_comm_init /
 *                             lii_comm_init_ex on a handle with model 1 refuse likewise); from inside lii_scan_job::while_waiting.
 *   lii_point_noise_get       the setting as the handle holds it (struct_size is checked on the way in).
 *   lii_point_noise_download  <- feats_down_body->points[i].intensity = sqrt(R_inv(i)) (:1051): the buffer of the last fit pass, one float per
 *                             point of the down-sampled cloud in the device's order (the rows of lii_scan_download(h, 2)) - (float)sqrt(R_inv_i)
 *                             of a selected point, 0.0f otherwise.  *n: the number of rows (always set); capacity < *n: LII_ERR_CAPACITY.
 *                             LII_ERR_STATE: model 0, or no fit pass since the model was set.
 *   The wire form of LII_PUB_EFFECT (lii_publish_wire_*) carries these values as the records' intensity under model 1 - what :1051 plus
 *   publish_effect_world (:625-636) would publish - and the constant (float)sqrt(1000.0) under model 0. */
typedef struct lii_point_noise {
  uint32_t struct_size;
  int32_t model;     /* 0: R_inv = laser_point_cov_inv for every point (default, :1050); 1: range / bearing (:1039-1042) */
  double range_inc;  /* [m]   calcBodyVar's range_inc  (0.02 at :1041) */
  double degree_inc; /* [deg] calcBodyVar's degree_inc (0.05 at :1041) */
} lii_point_noise;
int lii_point_noise_set(lii_handle h, const lii_point_noise* m);
int lii_point_noise_get(lii_handle h, lii_point_noise* m);
int lii_point_noise_download(lii_handle h, float* sqrt_rinv, int32_t capacity, int32_t* n);

/* The per-scan sequence of main() (src/laserMapping.cpp:909-1134) in ONE call, enqueued back to back on the handle's
 * stream with a single host round trip at the end: p_imu->Process' undistortion (:909; the scan is the one handed over by
 * lii_scan_upload / lii_scan_set_device, or job->scan_dev), downSizeFilterSurf.filter (:917-919) and the iterated update
 * (:957-1134).  The undistortion takes its end pose and extrinsic from `state` (the propagated state, as the reference
 * does: IMU_Processing.hpp:404-407 reads state_inout).  Equivalent to lii_undistort_* + lii_downsample(_skip) +
 * lii_iekf_update; it exists because every separate call costs the caller a host round trip. */
typedef struct lii_scan_job {
  uint32_t struct_size;            /* sizeof(lii_scan_job) */
  int32_t undistort;               /* 0 none, 1 IMU back-propagation, 2 constant-velocity model (LO mode) */
  const lii_pose6d* imu_poses;     /* undistort == 1: IMUpose table */
  int32_t n_imu_poses;
  float leaf;                      /* voxel-grid leaf size; <= 0: use the scan unfiltered */
  lii_iekf_opts opts;
  const void* scan_dev;            /* optional: adopt this device-resident scan first (as lii_scan_set_device would: float4
                                      x, y, z, t_ms; caller-owned, only read) - saves the separate call and a launch */
  int32_t n_scan_dev;
  int32_t scan_sorted;             /* 1: the scan's points are in ascending time order - the order the reference's preprocess hands
                                      every scan over in (src/preprocess.cpp:296-302) and lii_ingest_* / lii_frame_select deliver.
                                      The time-earliest point is then the first and the sweep ends with the last: the library
                                      skips the reduction that finds them (one launch per scan) and de-skews scan_dev in place of
                                      copying it first.  0: nothing is assumed.  A job that claims an order the scan does not have
                                      gets the A3 quirk / the CV sweep end applied to the wrong point - nothing else depends on it.
                                      2: sort this scan by time on the device first (what lii_scan_sort does: ascending t, stable, -0.0f
                                      and +0.0f equal) and go on as for 1 - no time-extent launch, the time-earliest point is the first,
                                      the sweep ends with the last (also pcl_end_time of lii_scan_register_imu).  It buys the reference's
                                      bits for a scan in any order (a driver cloud, a whole-message ingest frame) without a host sort.
                                      scan_dev and a selected ingest frame are only read: the sorted scan is written to the handle's own
                                      scan buffer.  Honoured by lii_scan_register, lii_scan_register_imu and lii_scan_register_cv.  Such a
                                      job neither uses nor arms the pre-armed prologue (next_scan_dev is ignored); with a communicator
                                      attached it returns LII_ERR_STATE (single rank only for now).  lii_set_profiling(h, 3) counts the
                                      sort's launches where it counts the time-extent launch of a scan_sorted = 0 job.  A job of
                                      struct_size 48 has no such field. */
  int32_t map_update;              /* 1: lii_map_incremental(h, state, NULL, NULL) with the update's final state follows the update inside
                                      this call (src/laserMapping.cpp:1146 behind :1134) - its launches are enqueued behind the update's passes
                                      while the device still works on them, instead of after the result has come back.  The caller does NOT
                                      call lii_map_incremental for this scan.  0 (the value of the formerly reserved field): nothing follows. */
  /* ABI 8 (struct_size 72; jobs of size 56 and 48 are still accepted): THE NEXT SCAN, if the caller already holds it in device memory.
   * The library then enqueues the next call's first launch - IMU de-skew + the voxel filter's insert over next_scan_dev - behind this
   * call's passes, where it waits ON THE DEVICE for what only the next call can know (the propagated state and the IMU pose table:
   * they depend on this call's result; src/laserMapping.cpp:905-915 - p_imu->Process runs on the state the update left).  The next
   * lii_scan_register hands them over with a store to mapped memory instead of a launch: the round trip result -> host -> first
   * kernel of the next scan loses the launch path (~5 us of ~10 per scan on an MI355X).  Only used when the next call asks for the
   * same thing (scan_dev == next_scan_dev, n_scan_dev == next_n_scan, undistort 1, scan_sorted 1, the same leaf, up to 64 poses);
   * anything else - another scan, any other entry point of the handle - ends the waiting launch first (it has touched nothing), and
   * a launch nobody comes for ends itself after 2 s (LII_PREARM_TIMEOUT_MS).  NULL / 0: no announcement (the forms of ABI <= 7). */
  const void* next_scan_dev;
  int32_t next_n_scan;
  int32_t reserved1;
  /* ABI 9 (struct_size 88; jobs of size 72, 56 and 48 are still accepted): THE HOST'S TIME INSIDE THE CALL.  Once every launch of the job is
   * enqueued the calling thread has nothing to do but wait for the result (~ 130 us per scan): while_waiting(while_waiting_arg) is called
   * exactly then, once, before the wait - the place for what the reference does between two scans (ros::spinOnce, src/laserMapping.cpp:893:
   * the callbacks that queue the next driver message - here lii_ingest_pcl2_begin / lii_ingest_livox_begin, whose ~ 50 us of enqueueing
   * then cost the loop nothing).  The hook may call the overlapped ingest's begin functions of this handle and anything that does not take the
   * handle; it must NOT call entry points that use the handle's stream (they would wait for, or disturb, the update under way).  A hook that
   * runs longer than the device delays the result by the difference.  Called once by every call that gets as far as its update, not by a
   * call that fails before.  NULL: nothing is called. */
  void (*while_waiting)(void* arg);
  void* while_waiting_arg;
} lii_scan_job;
int lii_scan_register(lii_handle h, const lii_scan_job* job, lii_state* state, const lii_state* state_propagated,
                      lii_iekf_report* report);

/* map_incremental (src/laserMapping.cpp:516-559): decides PointToAdd / PointNoNeedDownsample from the last
 * search's neighbour lists and applies both to the map.  n_add / n_no_downsample (the sizes of the two lists) may be NULL: then
 * the call returns without waiting for anything - the update is enqueued for predicted list sizes (those of the previous call
 * + 25 %) on a stream of its own, the next scan's arrival, de-skew and voxel filter overlap it, and whatever touches the map
 * next (a search, any lii_map_* call) waits for it first; an update whose lists outgrew the prediction is repeated there with
 * the exact sizes.  The map that results is the same either way.
 * Deferred errors: such a repeat can itself fail (LII_ERR_CAPACITY when the exact lists no longer fit max_map_points or the work
 * list - the padded predicted bounds passed the checks, the exact sizes are larger); the status then comes back from the call
 * that joined the update - the next lii_scan_register / lii_iekf_update / lii_map_* / lii_synchronize - not from this one; the
 * map is unchanged by the failed update and the handle stays usable. */
int lii_map_incremental(lii_handle h, const lii_state* state, int32_t* n_add, int32_t* n_no_downsample);

/* ---------------------------------------------------------------- IMU processing (ImuProcess::Process on the device)
 * The FORWARD half of ImuProcess::Process (src/IMU_Processing.hpp:419-461) - what lii_undistort_imu / lii_scan_register leave to the
 * caller: the state, the 24 x 24 covariance and the IMUpose table propagated over the scan's IMU samples (propagation_and_undist,
 * :292-382) or by the constant-velocity model (Forward_propagation_without_imu, :212-244).  One launch per scan (k_imu_propagate /
 * k_cv_propagate, lii_imu.hip).  What stays on the host: IMU_init (:161-200, a running mean over the first scans), the setters
 * (:127-159 - they become lii_imu_set_noise), sync_packages, and the hand-over scans of Process() that only re-arm the processor
 * (:426-453 - they become lii_imu_set_carry).  The L515 branch (:278-282) is not served: these entry points take no lidar type.
 *   lii_imu_sample          one sensor_msgs/Imu as the loop reads it (:304-319): header.stamp.toSec(), angular_velocity, linear_acceleration
 *   lii_imu_noise           cov_gyr ... cov_T_LI and IMU_mean_acc_norm, the members the setters write (:127-159).  lii_imu_noise_defaults:
 *                           the values of ImuProcess::ImuProcess() (:97-102); mean_acc_norm - which the constructor leaves unset and main()
 *                           installs from the parameter file - that of lii_params_defaults.  Host only, no handle.
 *   lii_imu_carry           what ImuProcess keeps between two scans: last_imu_, acc_s_last, angvel_last, last_lidar_end_time_
 *   lii_imu_set_noise       the setters; lii_imu_set_carry: what Process() sets on the init / switch-to-LIO scan (:432, :448: last_imu_ =
 *                           meas.imu.back()) - or any other carry a host wants to go on from; lii_imu_get_carry: the members after Process
 *                           (reads the device: waits for the handle's stream).
 *   lii_imu_propagate       the forward part of propagation_and_undist alone (:292-382): `state` in = after the previous update, out =
 *                           propagated; poses_out = IMUpose (capacity >= n_imu + 1 records, else LII_ERR_CAPACITY; *n_poses of them are
 *                           written); the handle's carry is advanced.  A synchronous call (tests, hosts that keep their own de-skew).
 *   lii_cv_propagate        Forward_propagation_without_imu without its de-skew (:212-244): dt as the caller's b_first_frame_ /
 *                           time_last_scan logic gives it (:215-221), cov_gyr_scale / cov_acc_scale of :234-235; `state` in / out.
 *   lii_scan_register_imu   Process() + the per-scan sequence in ONE call: propagate -> de-skew -> voxel filter -> iterated update
 *                           (-> map update).  The job is lii_scan_register's with undistort == 1, imu_poses == NULL, n_imu_poses == 0
 *                           (anything else: LII_ERR_INVALID).  `state` in is the state after the PREVIOUS update, NOT propagated; the
 *                           propagated state, the pose table and the update's state_propagated go from k_imu_propagate to the de-skew
 *                           and the solve in device memory.  pcl_end_time is formed on the device from the scan (pcl_beg_time + largest
 *                           t_ms / 1000, :288: the last point of a scan_sorted job, the time-extent reduction otherwise).  The carry lives
 *                           in the handle and is advanced by the call.  The samples are copied before the call returns (they ride in the
 *                           pinned block that carries the update's control block; k_imu_propagate pulls both).  leaf, scan_dev,
 *                           scan_sorted, map_update, while_waiting mean what they mean to lii_scan_register.  state_propagated_out (may
 *                           be NULL): the propagated state, covariance included.
 * Rules: n_imu < 1 -> LII_ERR_INVALID (the reference returns untouched when meas.imu.empty(), :423); n_imu > 63 (more than 64 poses, the
 * limit of the fused de-skew) -> LII_ERR_CAPACITY; no noise block or no carry set -> LII_ERR_STATE.  A pre-armed launch of the handle is
 * ended first, as by every other entry point, and job->next_scan_dev is IGNORED by lii_scan_register_imu (nothing is armed).  With a
 * communicator attached: LII_ERR_STATE (single rank only for now).  LII_TEST=host_solve: lii_scan_register_imu returns LII_ERR_STATE
 * (the host-driven loop has no device-resident control block to propagate into); lii_imu_propagate / lii_cv_propagate work.
 * The carry is advanced as soon as the propagation launch is on the stream: a call that fails BEHIND it (e.g. LII_ERR_STATE "no map",
 * a singular solve) has still consumed its samples, as Process() has when the update behind it fails; a call refused by the rules above,
 * or whose propagation launch itself fails, leaves the carry as it was.
 * lii_set_profiling(h, 3) attributes the new launch (and, for a scan that is not scan_sorted, the time-extent launch in front of it)
 * to LII_KP_PROPAGATE.
 *   lii_scan_register_cv    Process() with imu_en == false (src/IMU_Processing.hpp:212-266) + the per-scan sequence in ONE call, the LO
 *                           phase's counterpart of lii_scan_register_imu: propagate -> de-skew -> voxel filter -> iterated update
 *                           (-> map update), WITHOUT a launch for the propagation - it rides in the CV de-skew launch (k_deskew_cv_prop,
 *                           lii_scan.hip: every scan workgroup forms rot_end * Exp(bias_g, dt) for itself, one extra workgroup propagates
 *                           the state and its covariance and writes the update's state / state_propagated in device memory).  `state`
 *                           in is the state after the PREVIOUS update, NOT propagated; out: the updated state.  dt, cov_gyr_scale,
 *                           cov_acc_scale as for lii_cv_propagate (:215-221, :234-235).  state_propagated_out (may be NULL): the
 *                           propagated state, covariance included.  leaf, scan_dev, scan_sorted, map_update, while_waiting mean what
 *                           they mean to lii_scan_register.
 * Rules of lii_scan_register_cv: job->undistort != 2, imu_poses != NULL, n_imu_poses != 0, a NULL scale or a dt that is not finite ->
 * LII_ERR_INVALID; a communicator attached -> LII_ERR_STATE; LII_TEST=host_solve -> LII_ERR_STATE; no scan -> LII_ERR_STATE; no map ->
 * what lii_scan_register returns.  A refused call leaves `state` as it was.  A pre-armed launch is ended first and job->next_scan_dev is
 * IGNORED.  lii_set_profiling(h, 3) counts the launch as LII_KP_DESKEW: there is no propagate launch.  Under LII_TEST=no_fast the call is
 * lii_cv_propagate followed by lii_scan_register's general path - the same device code on the same numbers, the same results. */
typedef struct lii_imu_sample { double t; double gyr[3]; double acc[3]; } lii_imu_sample; /* 56 bytes */
typedef struct lii_imu_noise {
  uint32_t struct_size; /* sizeof(lii_imu_noise) */
  int32_t reserved0;
  double cov_gyr[3], cov_acc[3], cov_bias_gyr[3], cov_bias_acc[3], cov_R_LI[3], cov_T_LI[3];
  double mean_acc_norm;
} lii_imu_noise;
typedef struct lii_imu_carry {
  lii_imu_sample last_imu;
  double acc_s_last[3], angvel_last[3];
  double last_lidar_end_time;
} lii_imu_carry;
int lii_imu_noise_defaults(lii_imu_noise* out);
int lii_imu_set_noise(lii_handle h, const lii_imu_noise* noise);
int lii_imu_set_carry(lii_handle h, const lii_imu_carry* carry);
int lii_imu_get_carry(lii_handle h, lii_imu_carry* out);
int lii_imu_propagate(lii_handle h, const lii_imu_sample* imu, int32_t n_imu, double pcl_beg_time, double pcl_end_time, lii_state* state,
                      lii_pose6d* poses_out, int32_t capacity, int32_t* n_poses);
int lii_cv_propagate(lii_handle h, double dt, const double cov_gyr_scale[3], const double cov_acc_scale[3], lii_state* state);
int lii_scan_register_imu(lii_handle h, const lii_scan_job* job, const lii_imu_sample* imu, int32_t n_imu, double pcl_beg_time,
                          lii_state* state, lii_state* state_propagated_out, lii_iekf_report* report);
int lii_scan_register_cv(lii_handle h, const lii_scan_job* job, double dt, const double cov_gyr_scale[3], const double cov_acc_scale[3],
                         lii_state* state, lii_state* state_propagated_out, lii_iekf_report* report);

/* The first scan seeds the map (src/laserMapping.cpp:921-929) on the device: pointBodyToWorld (:209-220) at `state` over the current
 * down-sampled cloud - feats_down_body, which lii_downsample / lii_downsample_skip must have left (else LII_ERR_STATE) - becomes the map,
 * and the index is built; nothing visits the host.  *n_map: the points of the new map.  feats_down_size <= 5 (:922): nothing is built,
 * *n_map = 0, LII_OK - the map the handle had, if any, stays.  More points than max_map_points: LII_ERR_CAPACITY.  Like lii_map_build it
 * joins a pending map update first and the next pass searches again. */
int lii_map_build_from_scan(lii_handle h, const lii_state* state, int32_t* n_map);

/* ---------------------------------------------------------------- the registered clouds of a scan (publish_frame_world / pcd_save)
 * What laserMapping's loop hands out BEHIND the update, every scan (src/laserMapping.cpp:1152-1156), formed on the device at the
 * UPDATED state - pointBodyToWorld (:209-220; fp64 arithmetic, float result, the same bits) - without a host round trip:
 *   LII_PUB_DENSE   publish_frame_world with dense_publish_en (:561-614): the whole de-skewed scan (feats_undistort) in the world frame;
 *   LII_PUB_DOWN    publish_frame_world without it: feats_down_body in the world frame, in the device's order (that of the voxels'
 *                   first points; lii_scan_download(h, 1) restores PCL's);
 *   LII_PUB_EFFECT  publish_effect_world (:625-636): the points whose selection stands after the last pass (laserCloudOri), in the
 *                   world frame, compacted in ascending index of the device's down-sampled order - the same bits on every run; their
 *                   number is lii_iekf_report::effect_num;
 *   LII_PUB_BODY    publish_frame_body (:616-623): the de-skewed scan as it is (a copy).
 * Every cloud is float4 (x, y, z, t_ms), t_ms carried through unchanged.  The float4 records have no intensity: with LII_PUB_INTENSITY the
 * intensities of the registered scan (lii_scan_intensity_*, lii_ingest_set_intensity) are published beside the clouds, point for point.
 * lii_publish_set places a STANDING ORDER on the handle (off by default): from then on every call that reaches its update -
 * lii_scan_register, lii_scan_register_imu, lii_scan_register_cv, lii_iekf_update - enqueues one more launch behind its passes (behind
 * the map update of lii_scan_job::map_update, in front of a pre-armed prologue of lii_scan_job::next_scan_dev), which reads the final
 * state from device memory; a loop the host had to continue gets the launch again behind the passes that ended it.  The clouds are
 * always those of the state the call returns.  With save_capacity > 0 the dense world cloud of every scan is also appended to a save
 * buffer on the device (pcl_wait_save, :594-613; created by the first order that asks for it; another capacity: a new, empty buffer):
 * a scan that does not fit is not appended at all and raises a sticky flag - what the buffer holds is never lost.  With to_host the
 * clouds are copied to pinned host memory on the handle's copy stream, behind an event.  The clouds live in buffers of their own, two
 * deep.  NULL, or clouds == 0 && save_capacity == 0: the order is off (the buffers stay for a later order).  A communicator attached,
 * or LII_TEST=host_solve: LII_ERR_STATE (single rank only for now).  Bad struct_size, unknown bits in clouds, to_host other than
 * 0 / 1, save_capacity < 0: LII_ERR_INVALID.  lii_set_profiling(h, 3) attributes the launch to LII_KP_PUBLISH.
 *   lii_publish_now    the same outputs at the CALLER's state from the handle's current scan / down-sampled cloud / selection, for
 *                      hosts that call lii_undistort_* / lii_downsample / lii_iekf_iterate themselves (:1152-1156 behind their own loop).
 *   lii_publish_fetch  one cloud (ONE of the LII_PUB_* bits) of the LAST FINISHED registration (or lii_publish_now): *host_float4
 *                      (NULL without to_host) and *dev_float4 point into the library's buffers and stay valid until the registration
 *                      AFTER THE NEXT ONE BEGINS (that call's launch and copies overwrite them while it runs, its while_waiting
 *                      included); *n points.  Either pointer argument may be NULL.  The call waits for that cloud's copy
 *                      event only (without to_host: the launch's event): it neither uses the handle's stream nor ends a pre-armed launch,
 *                      so it MAY BE CALLED FROM lii_scan_job::while_waiting of the next call - scan m's clouds are consumed while scan
 *                      m + 1 is registered.  A cloud that was not ordered, or no registration since the order: LII_ERR_STATE; an unknown
 *                      cloud: LII_ERR_INVALID.
 *   lii_publish_saved  the save buffer's points so far -> out_float4 (may be NULL: *n only), and, with clear != 0, an empty buffer
 *                      (:603-612, the flush every pcd_save_interval scans; writing the PCD file is the caller's).  capacity < *n:
 *                      LII_ERR_CAPACITY, nothing is cleared.  A scan that did not fit since the last clear: the points are returned
 *                      and the call reports LII_ERR_CAPACITY.  Uses the handle's stream (not from while_waiting).
 *   LII_PUB_INTENSITY  a bit of lii_publish_opts::clouds, valid only together with at least one of DENSE / DOWN / BODY (alone:
 *                      LII_ERR_INVALID): the launch also hands on the intensities of the ordered clouds - dense and body: the scan's, in
 *                      the scan's order (sorted when the job sorts); down: the voxel filter's per-voxel means, row for row with the DOWN
 *                      cloud - into buffers of their own, two deep like the clouds, to_host honoured.
 *   lii_publish_fetch_intensity  cloud = LII_PUB_DENSE, LII_PUB_DOWN or LII_PUB_BODY: order, *n and lifetime are those of the cloud
 *                      lii_publish_fetch returns; it waits for the intensities' event only and MAY BE CALLED FROM while_waiting.
 *                      LII_PUB_EFFECT is NOT SERVED (LII_ERR_INVALID): the reference overwrites that cloud's intensity with sqrt(R_inv) =
 *                      sqrt(1000) (src/laserMapping.cpp:1051) - nothing of the sensor's is left to deliver.  The bit not ordered, the cloud not
 *                      ordered, or the registered scan had no intensities: LII_ERR_STATE.
 *   lii_publish_saved_intensity  with the bit set and save_capacity > 0 an intensity buffer of the same capacity is appended to in lock-step
 *                      with the save buffer - the same offset, the same fits / does-not-fit decision, by the same launch; a scan registered
 *                      without intensities appends 0.0f, so the two stay aligned.  This call reads it (out may be NULL: *n only; errors as
 *                      lii_publish_saved); the clearing call stays lii_publish_saved(..., clear = 1), which empties both. */
enum { LII_PUB_DENSE = 1, LII_PUB_DOWN = 2, LII_PUB_EFFECT = 4, LII_PUB_BODY = 8, LII_PUB_INTENSITY = 16 };
typedef struct lii_publish_opts {
  uint32_t struct_size;   /* sizeof(lii_publish_opts) */
  int32_t clouds;         /* LII_PUB_DENSE 1 | LII_PUB_DOWN 2 | LII_PUB_EFFECT 4 | LII_PUB_BODY 8 | LII_PUB_INTENSITY 16 */
  int32_t to_host;        /* 1: also copy each cloud to pinned host memory on the copy stream */
  int32_t save_capacity;  /* > 0: append the dense world cloud of every scan to a save buffer of that many points */
} lii_publish_opts;
int lii_publish_set(lii_handle h, const lii_publish_opts* opts);
int lii_publish_now(lii_handle h, const lii_state* state);
int lii_publish_fetch(lii_handle h, int32_t cloud, const float** host_float4, const void** dev_float4, int32_t* n);
int lii_publish_saved(lii_handle h, float* out_float4, int32_t capacity, int32_t* n, int32_t clear);
int lii_publish_fetch_intensity(lii_handle h, int32_t cloud, const float** host_float, const void** dev_float, int32_t* n);
int lii_publish_saved_intensity(lii_handle h, float* out, int32_t capacity, int32_t* n);

/* ---------------------------------------------------------------- the registered clouds as message bytes (pcl::toROSMsg / writeBinary)
 * The reference ends every scan with pcl::toROSMsg(*laserCloudWorld, msg) (src/laserMapping.cpp:578-586, :619, :632) and, every
 * pcd_save/interval scans, pcd_writer.writeBinary (:609).  lii_publish_wire_set places a SECOND STANDING ORDER beside lii_publish_set: the
 * same publish launch also forms each ordered cloud as the bytes of sensor_msgs/PointCloud2::data - records of pcl::PointXYZINormal,
 * point_step 48, little endian, twelve 32-bit words:
 *   word   0 1 2     3             4 5 6                         7     8          9          10 11
 *   field  x y z     pad data[3]   normal_x normal_y normal_z    pad   intensity  curvature  pad
 * msg.fields as pcl::toROSMsg writes them: x 0, y 4, z 8, normal_x 16, normal_y 20, normal_z 24, intensity 32, curvature 36 - all
 * FLOAT32 (datatype 7), count 1 (lii_publish_wire_layout hands the table out).  Contents, restating publish_frame_world :561-586 with
 * pointBodyToWorld :209-220, publish_frame_body :616-623 and publish_effect_world :625-636:
 *   LII_PUB_DENSE, LII_PUB_DOWN  laserCloudWorld is a cloud of default-constructed points of which pointBodyToWorld sets x, y, z and the
 *                   intensity only: x, y, z the world coordinates (the bits lii_publish_fetch gives), word 3 = 1.0f, words 4 - 7 = +0.0f,
 *                   intensity that of the scan (DENSE) or the voxel's mean (DOWN) where the registered scan carries intensities,
 *                   +0.0f where it does not; CURVATURE +0.0f - the time is NOT copied: the float4 clouds remain the place to get
 *                   t_ms; words 10 - 11 = 0.
 *   LII_PUB_EFFECT  as DOWN over the selected points, in the order of the float4 effect cloud; the intensity of every point is
 *                   (float)sqrt(1000.0) (:1050-1051: sqrt(R_inv)), whatever the scan carries - this form delivers the channel
 *                   lii_publish_fetch_intensity refuses.
 *   LII_PUB_BODY    feats_undistort as it is: x, y, z the de-skewed coordinates, word 3 = 1.0f, normals 0, intensity as for DENSE,
 *                   CURVATURE = t_ms, words 10 - 11 = 0.
 * The normals are 0 because every handler the library serves writes 0 there (src/preprocess.cpp:143-145 and siblings); the colours
 * the L515 handler puts into them (:470-472) are not carried, as everywhere else in the library.  Every zero word is 0x00000000.
 * NOT PINNED BY A BUILD: the pad values (1.0f in word 3 - PCL's PCL_ADD_POINT4D constructor -, zeros elsewhere) and the binary PCD
 * layout below are restated from knowledge of PCL's point_types.hpp and pcd_io.hpp; no PCL was available to run against (as
 * SURVEY.md Appendix B says of VoxelGrid).
 *   lii_publish_wire_set    clouds: a set of LII_PUB_DENSE | DOWN | EFFECT | BODY; off by default; NULL or clouds == 0: off.
 *                      INDEPENDENT of lii_publish_set - either order may be on alone, or both: an update enqueues ONE publish launch
 *                      either way (LII_KP_PUBLISH counts as before).  Buffers: two deep, 48 * max_scan_points bytes each, for the
 *                      ordered clouds only; with to_host they travel to pinned memory on the copy stream behind events of their own.
 *                      Bad struct_size, unknown bits (LII_PUB_INTENSITY is one here: the records always have the field), to_host
 *                      other than 0 / 1, reserved != 0: LII_ERR_INVALID.  A communicator attached, LII_TEST=host_solve, or a call from
 *                      while_waiting: LII_ERR_STATE.  PLACING OR CHANGING EITHER ORDER (lii_publish_set, lii_publish_wire_set) FORGETS THE
 *                      CLOUDS OF EARLIER REGISTRATIONS FOR BOTH: the fetches answer LII_ERR_STATE until the next registration.
 *   lii_publish_wire_fetch  the counterpart of lii_publish_fetch: *host_bytes (NULL without to_host) / *dev_bytes, 48 * *n_points
 *                      bytes, of the last finished registration (or lii_publish_now, which honours this order as the other); the same
 *                      lifetime (until the registration after the next one begins), waits for that cloud's event only, MAY BE CALLED
 *                      FROM while_waiting; the same errors.
 *   lii_publish_wire_layout  host only: point_step, the eight fields and the PCD row size - what fills msg.fields / point_step / row_step.
 *                      out->struct_size is the caller's sizeof(lii_wire_layout) (another value: LII_ERR_INVALID).
 *   lii_publish_saved_pcd  the save buffer (lii_publish_opts::save_capacity) as the rows of a binary PCD, as PCDWriter::writeBinary packs
 *                      the registered fields without padding - 32 bytes: x y z normal_x normal_y normal_z intensity curvature -, repacked
 *                      ON THE DEVICE from the buffer and its intensities (none kept: 0.0f; normals 0, curvature 0) and brought over
 *                      through a fixed staging area in chunks of at most 65 536 rows.  *n_points, capacity (here in BYTES: 32 * *n_points
 *                      needed), clear and the sticky overflow report are those of lii_publish_saved; rows_out == NULL: the count only.
 *   lii_pcd_header     host only: the text in front of the rows -
 *                        # .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z intensity curvature\n
 *                        SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH n\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n
 *                        POINTS n\nDATA binary\n
 *                      - into out (no terminating 0 is counted; one is written if it fits); *len: its length; capacity < *len:
 *                      LII_ERR_CAPACITY (*len is set); out == NULL: the length only. */
enum { LII_WIRE_POINT_STEP = 48, LII_WIRE_PCD_ROW = 32, LII_WIRE_FIELDS = 8, LII_WIRE_FLOAT32 = 7 };
typedef struct lii_wire_opts {
  uint32_t struct_size;   /* sizeof(lii_wire_opts) */
  int32_t clouds;         /* LII_PUB_DENSE 1 | LII_PUB_DOWN 2 | LII_PUB_EFFECT 4 | LII_PUB_BODY 8 */
  int32_t to_host;        /* 1: also copy each cloud's bytes to pinned host memory on the copy stream */
  int32_t reserved;       /* 0 */
} lii_wire_opts;
typedef struct lii_wire_field {
  char name[16];          /* 0-terminated */
  int32_t offset;         /* bytes from the start of the record */
  int32_t datatype;       /* sensor_msgs/PointField: 7 = FLOAT32 */
  int32_t count;
  int32_t pcd_offset;     /* bytes from the start of the binary PCD row */
} lii_wire_field;
typedef struct lii_wire_layout {
  uint32_t struct_size;   /* sizeof(lii_wire_layout), set by the caller */
  int32_t point_step;     /* 48 */
  int32_t n_fields;       /* 8 */
  int32_t pcd_row_bytes;  /* 32 */
  lii_wire_field fields[8];
} lii_wire_layout;
int lii_publish_wire_set(lii_handle h, const lii_wire_opts* opts);
int lii_publish_wire_fetch(lii_handle h, int32_t cloud, const void** host_bytes, const void** dev_bytes, int32_t* n_points);
int lii_publish_wire_layout(lii_wire_layout* out);
int lii_publish_saved_pcd(lii_handle h, void* rows_out, int64_t capacity_bytes, int32_t* n_points, int32_t clear);
int lii_pcd_header(int32_t n_points, char* out, int32_t capacity, int32_t* len);

/* ---------------------------------------------------------------- LI-Init batch calibration evaluators
 * CalibState record (include/LI_init/LI_init.h:31-89). */
typedef struct lii_calib_state {
  double rot_end[9];
  double ang_vel[3];
  double linear_vel[3];
  double ang_acc[3];
  double linear_acc[3];
  double timestamp;
} lii_calib_state;

/* Uploads the aligned IMU / LiDAR-odometry state sequences (IMU_state_group / Lidar_state_group). */
int lii_calib_set_buffers(lii_handle h, const lii_calib_state* imu, const lii_calib_state* lidar, int32_t n);
/* Residual + analytic Jacobian + J^T J / J^T r / cost for one stage at the given parameters:
 *  stage 1: Angular_Vel_Cost_only_Rot (LI_init.h:91-117)   params = R_LI[9]                      -> 3 dof
 *  stage 2: Angular_Vel_Cost          (LI_init.h:119-159)  params = R_LI[9], b_g[3], t_d         -> 7 dof
 *  stage 3: Linear_acc_Cost           (LI_init.h:161-205)  params = R_GL0[9], b_a[3], T_IL[3], R_LI[9] -> 9 dof
 * Tangent convention: R <- Exp(delta) R.  JtJ is dof x dof row-major, Jtr is dof, cost = 0.5 sum r^2. */
int lii_calib_eval(lii_handle h, int32_t stage, const double* params, double* JtJ, double* Jtr, double* cost);

typedef struct lii_calib_result {
  double R_LI[9];
  double T_LI[3];
  double gyro_bias[3];
  double acc_bias[3];
  double grav_L0[3];
  double time_lag_2;
  int32_t iterations[3];
  double final_cost[3];
} lii_calib_result;
/* solve_Rotation_only / solve_Rot_bias_gyro / solve_trans_biasacc_grav (LI_init.cpp:317-492): the three
 * least-squares problems, host Levenberg-Marquardt around lii_calib_eval. stage 3 expects the buffers AFTER
 * the second time compensation + acc_interpolate (caller re-uploads, as LI_Initialization does at :619-623). */
int lii_calib_solve_stage(lii_handle h, int32_t stage, lii_calib_result* inout);

/* LI_Init::LI_Initialization as a whole (include/LI_init/LI_init.cpp:586-632): the signal-conditioning chain on the host
 * (mean filter + interpolation :82-125, zero-phase Butterworth :260-315, cross-correlation :160-193, time compensation
 * :195-238, central differences :127-158, acc interpolation :240-258) around the three GPU-evaluated solves.
 * lii_li_init_interpolate = downsample_interpolate_IMU; lii_li_init_run = everything after it. */
/* LI_Init::data_sufficiency_assess (include/LI_init/LI_init.cpp:506-556; caller src/laserMapping.cpp:1169-1177) without the
 * progress bars: omg = the LiDAR angular velocity of every LO frame so far (n_frames x 3, frame order),
 * data_accum_length = initialization/data_accum_length.  eigenvalues: of sum [w]x^T [w]x, ascending; rot_percent: the
 * pairwise products of the scaled eigenvalues (the reference's Rot_percent up to its axis order); sufficient: all > 0.99. */
int lii_data_sufficiency(const double* omg, int32_t n_frames, double data_accum_length, double eigenvalues[3],
                         double rot_percent[3], int32_t* sufficient);
int lii_li_init_interpolate(const lii_calib_state* imu_all, int32_t n_imu, const lii_calib_state* lidar, int32_t n_lidar,
                            double move_start_time, lii_calib_state* imu_out, lii_calib_state* lidar_out, int32_t* n_out);
int lii_li_init_run(lii_handle h, const lii_calib_state* imu, const lii_calib_state* lidar, int32_t n, int32_t orig_odom_freq,
                    int32_t cut_frame_num, lii_calib_result* out, double* time_lag_1, double* total_time_lag);
/* The two pieces of that chain with real arithmetic volume, on the device, bit-identical to the host
 * path of lii_li_init_run:
 *   lii_zero_phase_filter  LI_Init::zero_phase_filt (include/LI_init/LI_init.cpp:260-315; Butterworth coefficients
 *                          LI_init.h:218-224) on n_seq sequences of n CalibStates laid back to back: the four 3-vectors are
 *                          filtered, rot_end / timestamp pass through (CalibState::operator= copies only the vectors);
 *   lii_xcorr_lag          LI_Init::xcorr_temporal_init (:160-193): lag_IMU_wtr_Lidar of the |ang_vel| series, one lane per lag;
 *   lii_li_init_set_device lii_li_init_run uses them (1) or the host functions (0, default: on the reference's committed run - 1 369 states -
 *                          the call takes 2.4 ms with the host chain and 7.4 ms with the device chain, a recursive filter being serial in time;
 *                          same bits either way). */
int lii_zero_phase_filter(lii_handle h, const lii_calib_state* in, int32_t n_seq, int32_t n, lii_calib_state* out);
int lii_xcorr_lag(lii_handle h, const lii_calib_state* imu, const lii_calib_state* lidar, int32_t n, int32_t* lag_imu_wrt_lidar);
int lii_li_init_set_device(lii_handle h, int32_t on_device);

/* LI_Init::LI_Initialization resident on the device (include/LI_init/LI_init.cpp:586-632): one upload of the accumulated states, then
 * a fixed sequence of launches on the handle's stream - downsample_interpolate_IMU (:82-125), IMU_time_compensate (:195-221), both
 * zero_phase_filt (:260-315), normalize_acc (:494-504), cut_sequence_tail (:223-238), xcorr_temporal_init (:160-193), central_diff
 * (:127-158), acc_interpolate (:240-258) and the three least-squares solves (:317-492), each a whole Levenberg-Marquardt in one launch -
 * and ONE wait of the host, at the end.  The sequences stay in place: what the host chain erases is a start index and a length in a
 * control block in device memory that the later launches read; no length visits the host before the end.  The conditioning is the
 * host chain's arithmetic operation for operation (same bits); the solves evaluate with lii_calib_eval's device function (same bits at
 * the same parameters) and restate lii_calib_solve_stage's trust-region loop on the device, where sin / cos / pow come from the device
 * library: the path of a solve can differ from the host LM's in the last bits.
 *   interpolate = 1: imu = every raw IMU CalibState (ang_vel, linear_acc in m/s^2, timestamp), lidar = every LiDAR-odometry CalibState;
 *                    downsample_interpolate_IMU runs first (what lii_li_init_interpolate does on the host).
 *   interpolate = 0: the aligned sequences lii_li_init_run takes (n_imu == n_lidar).
 * Refused on the host before anything is enqueued, LII_ERR_INVALID: NULL handle / job / out / sequences, a wrong struct_size,
 * interpolate other than 0 or 1, orig_odom_freq < 1 or cut_frame_num < 1, n < 200 or n_imu != n_lidar (aligned form), n_imu < 6 or
 * n_lidar < 1 (raw form).  What only the data decides is found on the device, which then skips the rest of the sequence; the call
 * returns LII_ERR_INVALID (fewer than 6 raw IMU states or fewer than 200 aligned states after interpolation; "fewer than 61 aligned
 * states left to filter", the text of lii_li_init_run) and the handle stays usable.  From inside lii_scan_job::while_waiting:
 * LII_ERR_STATE.  Like every entry point it ends a pre-armed launch of the handle first.
 * After a successful call the stage-3 sequences are the handle's calibration buffers, as after lii_li_init_run: lii_calib_eval may follow.
 * The call allocates only when its inputs are longer than any before (the buffers grow geometrically). */
typedef struct lii_li_init_job {
  uint32_t struct_size;
  int32_t interpolate;
  const lii_calib_state* imu;
  int32_t n_imu;
  const lii_calib_state* lidar;
  int32_t n_lidar;
  double move_start_time; /* interpolate == 1 only */
  int32_t orig_odom_freq, cut_frame_num;
} lii_li_init_job;
/* lii_li_init_report::termination - the exits of the trust-region loop (Ceres' order of tests) */
enum lii_lm_termination {
  LII_LM_GRADIENT_AT_START = 0, /* gradient tolerance at the projected start point: no iteration */
  LII_LM_MAX_ITERATIONS = 1,
  LII_LM_MIN_RADIUS = 2,
  LII_LM_INVALID_STEPS = 3,     /* five steps in a row without a positive model decrease */
  LII_LM_PARAMETER_TOLERANCE = 4,
  LII_LM_FUNCTION_TOLERANCE = 5,
  LII_LM_GRADIENT_TOLERANCE = 6 /* after an accepted step */
};
typedef struct lii_li_init_report {
  uint32_t struct_size;
  int32_t n_aligned, n_stage12, n_stage3; /* states after interpolation / entering stages 1-2 / entering stage 3 */
  int32_t lag_samples;                    /* lag_IMU_wtr_Lidar of the cross-correlation */
  int32_t launches, host_waits;           /* kernel launches enqueued by the call (a constant of the build); stream waits made by it (1) */
  int32_t termination[3];                 /* enum lii_lm_termination per stage */
  double time_lag_1, total_time_lag;
  double params[3][24];                   /* the final point of each stage in lii_calib_eval's parameter layout */
} lii_li_init_report;
int lii_li_init_resident(lii_handle h, const lii_li_init_job* job, lii_calib_result* out, lii_li_init_report* rep /* may be NULL */);
/* The sequences the last successful resident run solved on - what the reference dumps into Log/IMU_meas.txt, Log/LiDAR_meas.txt and
 * Log/acc_cost.txt (LI_init.cpp:606-623).  which = 1: entering stages 1 / 2; which = 2: entering stage 3.  Both pointers NULL: *n
 * only.  capacity < *n: LII_ERR_CAPACITY, nothing written.  No resident run yet: LII_ERR_STATE.  Any other `which`: LII_ERR_INVALID. */
int lii_li_init_resident_fetch(lii_handle h, int32_t which, lii_calib_state* imu, lii_calib_state* lidar, int32_t capacity, int32_t* n);
/* solve_Rotation_only / solve_Rot_bias_gyro / solve_trans_biasacc_grav (LI_init.cpp:317-492) with the contract of
 * lii_calib_solve_stage on the buffers of lii_calib_set_buffers, the whole Levenberg-Marquardt in one launch: `inout` goes up, the
 * launch runs, the result comes back.  No buffers uploaded: LII_ERR_STATE. */
int lii_calib_solve_stage_dev(lii_handle h, int32_t stage, lii_calib_result* inout);

/* LI_Initialization on K sub-ranges ("windows") of one accumulation in one call.  The reference calibrates once per accumulation
 * (include/LI_init/LI_init.cpp:586-632, called from src/laserMapping.cpp:1190-1198 when data_sufficiency_assess says so); whether
 * that extrinsic, bias or time offset is stable it cannot say.  Calibrating on prefixes (what the result would have been had the
 * initialisation fired at frame n) and on sliding windows of the same accumulation answers that, and K independent windows fill
 * the K workgroups per launch that the single call's one-workgroup launches leave idle.
 * DEFINITION.  out[w] is what lii_li_init_resident returns for a job with imu = job->imu + imu_begin, n_imu = imu_count,
 * lidar = job->lidar + lidar_begin, n_lidar = lidar_count, the window's move_start_time and the job's interpolate, orig_odom_freq
 * and cut_frame_num: the same bits in the result and in every report field but launches / host_waits, which are the whole call's.
 * The sequences go up once; a fixed number of launches follows, whatever K is, window w being blockIdx.y of each; the host waits once.
 * A window reads and writes only areas of its own, so a record does not depend on K or on the windows beside it.
 * REFUSALS FOUND BY THE DATA (where the single call returns LII_ERR_INVALID for a reason only the data decides) are the window's
 * `status`; the call returns LII_OK and the other windows are unaffected.
 * REFUSED ON THE HOST, before anything is enqueued, LII_ERR_INVALID: a NULL argument; a wrong job->struct_size or an out_stride
 * other than sizeof(lii_li_init_window_result); what lii_li_init_resident refuses in the job's scalars; n_windows < 1 or > 4096; a
 * range outside the job's sequences; aligned form: imu_begin != lidar_begin, imu_count != lidar_count or a count < 200; raw form:
 * imu_count < 6 or lidar_count < 1.  LII_ERR_CAPACITY: the call's device scratch would exceed 4 GiB, where scratch =
 *   176 (n_imu + n_lidar) + 24 K + K (904 + 8 (116 c + c / 2 + 8) + [raw form] 32 r)   bytes,
 * c = the longest lidar_count, r = the longest imu_count (904 bytes hold a window's control and result block).  From inside
 * lii_scan_job::while_waiting: LII_ERR_STATE.  Like every entry point it ends a pre-armed launch of the handle first.
 * OBSERVER.  The call touches neither the buffers lii_calib_eval / lii_calib_solve_stage* read nor what lii_li_init_resident_fetch
 * serves.  It allocates only when a buffer of an earlier call is too small (lii_li_init_windows_scratch counts). */
typedef struct lii_li_init_window {      /* one sub-range of the job's sequences */
  int32_t imu_begin, imu_count;          /* aligned form: must equal lidar_begin, lidar_count */
  int32_t lidar_begin, lidar_count;
  double  move_start_time;               /* raw form only */
} lii_li_init_window;

enum { LII_WIN_OK = 0, LII_WIN_FILTER61 = 1, LII_WIN_ALIGNED200 = 2, LII_WIN_RAW6 = 3, LII_WIN_NO_OVERLAP = 4 };

typedef struct lii_li_init_window_result {
  int32_t status;                        /* LII_WIN_*; everything below is zero unless LII_WIN_OK */
  int32_t pad;
  lii_calib_result res;
  lii_li_init_report rep;                /* struct_size filled in; launches / host_waits are the whole call's */
} lii_li_init_window_result;

int lii_li_init_windows(lii_handle h, const lii_li_init_job* job, const lii_li_init_window* windows, int32_t n_windows,
                        lii_li_init_window_result* out, uint32_t out_stride /* sizeof the record */);
/* The device scratch lii_li_init_windows holds on this handle, in bytes, and the allocations (device and pinned) its calls have
 * made so far: a call no larger than an earlier one leaves both unchanged.  Either pointer may be NULL. */
int lii_li_init_windows_scratch(lii_handle h, uint64_t* bytes, int64_t* allocations);

/* ---------------------------------------------------------------- multi-GPU (points of one scan sharded across ranks)
 * One process per GPU.  Rank 0 creates an id, the caller ships the 128 bytes to the other ranks (e.g.
 * torch.distributed broadcast), every rank calls lii_comm_init with the SAME state / options per scan; afterwards
 * lii_iekf_iterate / lii_iekf_update / lii_scan_register sum the 91 normal-equation scalars (fp64, in rank order, so every
 * rank forms the bit-identical sum and takes the same decisions) over the ranks.
 * Partition (lii_comm_set_partition; default 1): every rank hands over the WHOLE scan and holds the whole map.
 *   1 - by index: the de-skew and the voxel filter run replicated (their output is bit-identical on every rank, so a voxel is never
 *       split between ranks) and rank r registers the contiguous block [n r / N, n (r + 1) / N) of the down-sampled cloud, which the
 *       filter emits in the order of the voxels' first points - a stretch of the sweep per rank.
 *   2 - by voxel (SURVEY.md section 8e "a voxel-key partition"): where the voxel filter's insert is fused into the de-skew
 *       (lii_scan_register with leaf > 0; the hashed filter is then used for every scan) every rank de-skews the scan but inserts,
 *       filters, searches and fits only the voxels whose key hashes to it (~ 1 / N of them, +- a percent, whatever the scene);
 *       lii_downsample's / lii_scan_download's view of the down-sampled cloud is then this rank's share.  Elsewhere (stand-alone
 *       lii_downsample, leaf 0) the split is by index.  A share that outgrows n / N + 25 % + 2048 points fails the update with
 *       LII_ERR_CAPACITY.  Needs a transport that carries the list exchange below - the peer-mapped mailbox or RCCL - (the host-memory
 *       mailbox stays with 1; lii_comm_describe tells).
 *   0 - the caller hands every rank its own points.
 *   Either way the sharded result equals the single-GPU result up to the re-association of the 91 sums.
 *   lii_map_incremental of a sharded job: every rank decides for ITS points, and the two insert lists (PointToAdd /
 *   PointNoNeedDownsample, src/laserMapping.cpp:516-559) are exchanged - pushed into every rank's gather area behind the mailbox
 *   slots, or gathered with two ncclAllGather calls on the RCCL transport - and put together in rank order, so that every replica of
 *   the map applies the identical batch.  On the host-memory mailbox a job split by index repeats the last search for the whole
 *   cloud instead (no exchange).
 * Transports:
 *   LII_COMM_MAILBOX       ranks of ONE node; the exchange runs inside the reduce+solve kernel (no extra launch, no
 *                          collective-library call).  Every rank keeps the slots it reads in fine-grained HBM, exported through
 *                          a HIP IPC handle: an exchange pushes the 91 sums into the peers' memory (remote stores over xGMI)
 *                          and polls local memory.  Works between processes on one device as well.
 *   LII_COMM_MAILBOX_HOST  the same exchange through a POSIX shared-memory segment registered with every rank's device (host
 *                          memory over PCIe): what LII_COMM_MAILBOX falls back to in AUTO mode when an IPC handle cannot be
 *                          exported or opened.
 *   LII_COMM_RCCL          ncclAllReduce on the handle's stream between a separate final-sum and solve launch (any topology).
 *   LII_COMM_AUTO          the HBM mailbox when all ranks meet on one node within the set-up time (20 s; LII_MAILBOX_TIMEOUT_S=<exchange>[,<set-up>]), else the
 *                          host-memory mailbox, else RCCL.
 * A rank that stops calling (error on one rank only) makes the others' next update fail with LII_ERR_COMM after
 * LII_MAILBOX_TIMEOUT_S (default 30 s; RCCL: its own watchdog); the communicator must then be re-created.  lii_comm_init == lii_comm_init_ex(..., LII_COMM_AUTO). */
enum { LII_COMM_AUTO = 0, LII_COMM_RCCL = 1, LII_COMM_MAILBOX = 2, LII_COMM_MAILBOX_HOST = 3 };
int lii_comm_unique_id(uint8_t id_out[128]);
int lii_comm_init(lii_handle h, int32_t n_ranks, int32_t rank, const uint8_t id[128]);
int lii_comm_init_ex(lii_handle h, int32_t n_ranks, int32_t rank, const uint8_t id[128], int32_t transport);
int lii_comm_transport(lii_handle h, int32_t* transport); /* the transport in use; LII_COMM_AUTO = none (single rank) */
/* Which transport this rank ended up with and why, as text (e.g. "mailbox in registered host memory - the HBM form was not
 * possible: device 0 cannot access its peer 0000:c1:00.0 (hipDeviceCanAccessPeer)"); LII_DIAG=1 prints it at set-up. */
int lii_comm_describe(lii_handle h, char* out, int32_t capacity);
int lii_comm_rccl_ranks(lii_handle h, int32_t* n_ranks);  /* ncclCommCount of the attached RCCL communicator; 0: none attached */
int lii_comm_set_partition(lii_handle h, int32_t library_partition);  /* 0 caller | 1 by index (default) | 2 by voxel */
int lii_comm_destroy(lii_handle h);
/* TEST ENTRY POINT - not part of the per-scan path.  It plays its ranks in the handle's own list buffers: LII_ERR_STATE while a map update
 * of the handle is pending (its lists would be overwritten; call lii_map_commit first); leaves the exchange's sequence number and scratch
 * as it found them.
 * Self-test of the list exchange of a sharded job's map update (lii_map_incremental; lii_exchange.hip) with n_ranks > 1 on ONE device:
 * the handle (not a rank of a job) plays rank 0 .. n_ranks - 1 in turn.  form 0: the gather areas of the mailbox transport; form 1:
 * the trimmed all-gather layout of the RCCL transport (the functions lists_exchange_rccl is made of, device copies standing in for the
 * two ncclAllGather calls - a communicator holds one rank per device, the layout can still be exercised).  Rank r's lists: n_add[r] /
 * n_nodown[r] points (x, y, z, w) behind each other in add_xyzw / nodown_xyzw.  Every played rank must end with the identical pair
 * of joined lists (else LII_ERR_COMM); they are returned (capacity: points per output).  Reference: the two Add_Points calls every
 * replica of the map must receive identically, src/laserMapping.cpp:556-557. */
int lii_selftest_list_exchange(lii_handle h, int32_t n_ranks, int32_t form, const float* add_xyzw, const int32_t* n_add, const float* nodown_xyzw,
                               const int32_t* n_nodown, float* out_add, int32_t* out_n_add, float* out_nodown, int32_t* out_n_nodown, int32_t capacity);

/* ---------------------------------------------------------------- parameter surface (config/<sensor>.yaml + launch/<sensor>.launch)
 * The nh.param<> block of main() (src/laserMapping.cpp:767-799) as a POD: same names (`section/key` -> field), same defaults.
 * roslaunch fills the parameter server from `<rosparam command="load" file="$(find lidar_imu_init)/config/X.yaml"/>` and
 * `<param name=".." value=".."/>` (launch/<sensor>.launch:6-12); a host without ROS calls
 *   lii_params_defaults    the third argument of every nh.param<> call
 *   lii_params_load_yaml   one config/<sensor>.yaml on top (block maps, scalars, quoted strings, flow lists, '#' comments)
 *   lii_params_load_launch a launch file: its rosparam yaml (looked up in `config_dir`, else <launch dir>/../config) first,
 *                          then its <param> tags (names a node never reads are ignored, as on the parameter server)
 *   lii_params_set         one override by name ("max_iteration", "mapping/filter_size_surf", ...)
 *   lii_params_apply       -> lii_config (map down-sample box = mapping/filter_size_map), lii_ingest_opts (lidar_type, scan_line,
 *                          point_filter_num, blind, cut_frame_num; stamp / scan_count stay per message), lii_iekf_opts
 *                          (max_iteration; imu_en = 0 as at start-up, laserMapping.cpp:87), voxel leaf = mapping/filter_size_surf.
 * Host functions (no device work, no handle). */
typedef struct lii_params {
  uint32_t struct_size; /* sizeof(lii_params); set by lii_params_defaults */
  int32_t max_iteration, point_filter_num;
  double filter_size_surf, filter_size_map, cube_side_length, det_range;
  double gyr_cov, acc_cov, grav_cov, b_gyr_cov, b_acc_cov;
  double blind;
  int32_t lidar_type, scan_line, feature_extract_en;
  int32_t cut_frame, cut_frame_num, orig_odom_freq;
  double online_refine_time, mean_acc_norm, data_accum_length;
  double Rot_LI_cov[3], Trans_LI_cov[3];
  int32_t n_Rot_LI_cov, n_Trans_LI_cov; /* entries present in the file (the reference reads vector<double>) */
  int32_t path_en, scan_publish_en, dense_publish_en, scan_bodyframe_pub_en, runtime_pos_log_enable, pcd_save_en, pcd_save_interval;
  int32_t reserved0;
  char lid_topic[128], imu_topic[128], map_file_path[256];
} lii_params;
int lii_params_defaults(lii_params* p);
int lii_params_load_yaml(const char* yaml_path, lii_params* inout);
int lii_params_load_launch(const char* launch_path, const char* config_dir /* may be NULL */, lii_params* inout);
int lii_params_set(lii_params* inout, const char* name, const char* value);
int lii_params_apply(const lii_params* p, int32_t device, int32_t max_scan_points, int32_t max_map_points, lii_config* cfg /* may be NULL */,
                     lii_ingest_opts* ingest /* may be NULL */, lii_iekf_opts* opts /* may be NULL */, float* leaf /* may be NULL */);
/* cube_side_length, mapping/det_range -> lii_local_map_opts with enabled = 1 (lii_local_map_set judges the values) */
int lii_params_local_map(const lii_params* p, lii_local_map_opts* out);
const char* lii_params_last_error(void);

/* ---------------------------------------------------------------- utilities for harnesses */
int lii_dev_alloc(lii_handle h, size_t bytes, void** dev_ptr);
int lii_dev_free(lii_handle h, void* dev_ptr);
int lii_dev_upload(lii_handle h, void* dev_dst, const void* host_src, size_t bytes);
/* Accumulated device timings [ms] since lii_set_profiling(h, 1), measured with HIP events on the handle's stream:
 * lii_iekf_update / lii_scan_register: [5] number of executed k-NN passes, [7] their total time (events around the k-NN launches
 * only: every event is a barrier on the stream), [4] wall time of the last update; lii_iekf_iterate: also [0] / [1] search-pass /
 * residual-pass kernels, [2] the final sum, [6] count of [1]; [3] host solve (host-driven loop only). */
int lii_set_profiling(lii_handle h, int32_t enabled); /* 1: start (zero the accumulators), 2: resume, 0: pause, 3: see below */
int lii_last_timings(lii_handle h, double out_ms[8]);
/* lii_set_profiling(h, 3): lii_scan_register brackets EVERY launch of the scan with HIP events (a barrier packet each: the
 * scan runs slower than unprofiled - this mode is for attributing time, not for measuring throughput) and accumulates, per
 * kind of launch, the time from its event to the next one (kernel + dispatch) and the number of launches that executed.
 * Accumulators start at lii_set_profiling(h, 1), like the others. */
enum lii_kernel_kind {
  LII_KP_DESKEW = 0,     /* adoption + de-skew (+ the voxel filter's insert, + the time-extent launch of an unsorted scan) */
  LII_KP_VOXEL = 1,      /* the rest of the voxel filter - AND, on a handle with lii_local_map_set(enabled = 1), the three launches of the
                            local map (this struct has no kind to spare in ABI 9): + 3 launches per scan and their time */
  LII_KP_KNN = 2,        /* k-NN pass */
  LII_KP_FIT_SEARCH = 3, /* plane fit + residual + reduction behind a k-NN pass */
  LII_KP_FIT = 4,        /* residual + reduction on cached planes */
  LII_KP_SOLVE = 5,      /* final sum + 24-state solve */
  LII_KP_PROPAGATE = 6,  /* lii_scan_register_imu: IMU forward propagation (+ the time-extent launch of an unsorted scan in front of it) */
  LII_KP_PUBLISH = 7,    /* lii_publish_set: the registered clouds of the scan (k_publish_world) */
  LII_KP_KINDS = 8
};
typedef struct lii_kernel_profile {
  uint32_t struct_size; /* sizeof(lii_kernel_profile) */
  int32_t scans;        /* scans profiled */
  double ms[LII_KP_KINDS];
  int32_t launches[LII_KP_KINDS];
} lii_kernel_profile;
int lii_last_kernel_profile(lii_handle h, lii_kernel_profile* out);

#ifdef __cplusplus
}
#endif
#endif /* LIINIT_HIP_H */

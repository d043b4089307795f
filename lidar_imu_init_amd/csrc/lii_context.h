// The handle of libliinit_hip and the host-side internals its translation units share (not part of the C-ABI):
//   lii_capi.cpp           life cycle, scan in / de-skew / voxel grid, downloads, profiling
//   lii_capi_map.cpp       the device-resident local map: (re)build, in-place updates, lii_map_*, lii_map_incremental
//   lii_capi_register.cpp  the registration loop: lii_iekf_*, lii_scan_register, neighbour download
//   lii_capi_comm.cpp      the communicator of a sharded job (node-local mailbox / RCCL)
//   lii_capi_calib.cpp     the LI_init evaluators' entry points
//   lii_capi_imu.cpp       IMU forward propagation: lii_imu_*, lii_cv_propagate, lii_scan_register_imu, lii_scan_register_cv
//   lii_capi_publish.cpp   the registered clouds of a scan: lii_publish_*
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/liinit_hip.h"
#include "lii_launch.h"
#include "lii_owned.h"

using lii::BlockEntry; using lii::IekfCtrl; using lii::IekfResult; using lii::PoseArg; using lii::VoxelHashBuffers; using lii::MailboxHost;
using lii::DevBuf; using lii::PinnedBuf;
constexpr size_t kCtrlBytes = (sizeof(lii::IekfCtrl) + 255) / 256 * 256;

// ---- the handle's small pinned scratch (lii_context::h_small): where a few words travel between the host and the device.  One member
// per use, free again when the call that used it has returned (each ends with a synchronisation of its stream); what an argument check
// enforces is the member's extent.
constexpr int kMapBoxesMax = 4096;  // boxes of one lii_map_delete_boxes / lii_map_box_search
constexpr int kImuSamplesMax = 63;  // IMU samples of one scan (lii_capi_imu.cpp: check_feed); the pose table holds one pose more
constexpr int kGxRanksMax = 128;    // ranks of a job whose map lists travel over RCCL (lii_capi_comm.cpp: gx_prepare)
constexpr int kCalibEvalParams = 24, kCalibEvalOut = 9 * 9 + 9 + 1;  // lii_calib_eval: stage 3 has the most parameters and outputs
constexpr int kLiInitBackDoubles = 128;  // lii_li_init_resident: its control and result block (kSmallDoubles, lii_li_init_resident.hip)
struct PinnedScratch {
  double normal_eq[lii::kNormalEq];        // iterate: the sums of a host-driven pass
  double calib_params[kCalibEvalParams];   // lii_calib_eval: in,
  double calib_out[kCalibEvalOut];         // ... out: JtJ | Jtr | cost
  double li_init_back[kLiInitBackDoubles]; // lii_li_init_resident: ResCtl | ResOut
  lii_calib_result calib_stage;            // lii_calib_solve_stage_dev: in and out
  lii::PoseArg pose;                       // iterate: the pose on its way to d_pose
  lii_pose6d imu_poses[kImuSamplesMax + 1];  // lii_imu_propagate: the pose table
  unsigned long long box_hits;             // lii_map_box_search: the hit counter
  unsigned char gx_headers[kGxRanksMax * lii::kGatherHeaderBytes];  // gx_gather_collect: every rank's list header
  float boxes[kMapBoxesMax * 6];           // lii_map_delete_boxes / lii_map_box_search: the boxes on their way to the device
  float map_range[6];                      // lii_map_range
  unsigned int index_blocks;               // build_index: blocks of the new index
  unsigned int win_box[6];                 // build_index: the box of the occupied blocks
  unsigned int gather_count;               // map_gather: live points
  int n_body[2];                           // resolve_n_body: d_nbody
  int map_ctr[lii::kMapCtrWords];          // read_counters / lii_map_incremental: d_mapctr
  int list_counts[6];                      // lii_map_incremental: d_counts
  int add_events;                          // lii_map_add_points: kMapCtrEvents
};

// A resource of the handle is a member of an owning type (lii_owned.h) and goes with the handle; a raw pointer here is an alias
// into one of them, or memory of somebody else, and its comment says which.
struct lii_context {
  lii_config cfg{};
  int device = 0;
  // the streams come first: members go in reverse order, so the buffers and events are released before the streams they were used on
  lii::Stream stream;
  lii::Stream copy_stream;  // lii_scan_upload_next: the next scan's transfer (created on first use)
  lii::Stream map_stream;   // the in-place update of lii_map_incremental runs here, beside the next scan's pre-processing
  std::string err;

  // ---- local map (device resident).  d_pts is the live point array: cell by cell with slack behind every cell (in-place
  // updates, lii_map.hip); d_map_unsorted / d_map are staging for (re)builds (input, then cell-sorted and compact).
  float ds = 0.2f;              // ikd-Tree downsample box (set_downsample_param)
  DevBuf<unsigned char> d_tomb;
  DevBuf<float4> d_batch;    // a host-provided Add_Points batch (M)
  DevBuf<float4> d_dropped;  // inserts an in-place update found no room for (kMapCtrDropped of them): re-inserted after a rebuild
  unsigned int drop_cap = 0;    // = d_dropped.size() (a kernel argument)
  // dense cell window over the map's box (GridView::win): filled by build_index, dropped by whatever changes a cell entry
  DevBuf<uint2> d_win;
  int win_org[3] = {0, 0, 0}, win_dim[3] = {0, 0, 0};
  bool win_valid = false;
  long long win_kept = 0, win_dropped = 0;  // LII_DIAG: in-place updates the window was kept current through / times it had to be dropped
  bool win_keep = true;          // LII_WINDOW_KEEP=0: the first in-place update drops the window (round 6's first form) instead of keeping it current
  DevBuf<unsigned long long> d_block_key;  // packed block coordinates by block id (WinKeep::key_of_id), cells_cap_blocks entries
  bool map_has_w = false;       // the map may hold intensities (an _xyzi input since the last lii_map_reset / lii_map_build, or map_intensity): the folds and the insert launches carry the points' fourth word
  bool map_intensity = false;   // lii_map_intensity_set: the scan-driven map updates take each inserted point's intensity from inten.d_body
  bool map_tight = false;       // LII_TEST=map_tight: no spare room is provisioned (tests: forces the recovery path)
  long long map_recoveries = 0;
  DevBuf<float4> d_ins;         // fold output (M)
  DevBuf<unsigned int> d_u32_a, d_u32_b;  // flags / ranks (max(N, M) each)
  DevBuf<float4> d_list_add, d_list_nodown;  // map_incremental lists (N each)
  int* d_counts = nullptr;      // inside d_mapctr, behind the kMapCtrWords counters: [0] add list, [1] no-downsample list, [2] alive, [3] inserted, [4] total, [5] events
  DevBuf<float4> d_map_unsorted;
  DevBuf<float4> d_map;
  DevBuf<float4> d_pts;            // pts_cap slots
  unsigned int pts_cap = 0;
  unsigned int pts_cap_eff = 0;  // = pts_cap (LII_TEST=map_tight: a few slots behind the cells, so that updates run out of room)
  DevBuf<unsigned int> d_cell_cap; // capacity end of every cell entry (same indexing as d_cells)
  DevBuf<unsigned int> d_tp;       // per cell entry: on-work-list bit | pending inserts
  DevBuf<unsigned int> d_cs_a, d_cs_b;  // per cell entry scratch (capacities / counts and their scans)
  DevBuf<unsigned int> d_work;     // work list of the update in flight (cell entries)
  unsigned int work_cap = 0;       // = d_work.size() (a kernel argument)
  DevBuf<unsigned int> d_ins_e, d_ins_e2;  // cell entry of every insert (fold output / plain list)
  DevBuf<unsigned long long> d_ah_key;   // hash-grouped fold of lii_map_incremental (lii_map.hip: AddHash): voxel keys,
  DevBuf<unsigned long long> d_ah_best;  // per-slot minima (both all ones between updates),
  DevBuf<unsigned int> d_ah_slot;        // the slot of every batch point
  bool wide_listed = false;                 // the last scan's search passes listed more than kFlagCap unfinished queries: the next one's search launches are followed by k_complete_listed
  bool wide_prev = false;                   // ... the scan before it did (two in a row switch wide_listed)
  bool unfinished_known = false;            // IekfResult::unfinished belongs to the last search the handle ran (lii_last_unfinished_queries)
  bool wide_enabled = true;                 // LII_WIDE_COMPLETION=0: never (every workgroup of the fit launch finishes its own, rounds 4 - 6)
  long long wide_scans = 0, wide_switches = 0;
  void (*wait_hook)(void*) = nullptr;       // lii_scan_job::while_waiting of the call under way (update_on_device calls it once, before its wait)
  void* wait_hook_arg = nullptr;
  bool in_wait_hook = false;               // ... while it runs: entry points that change which frames are current refuse (lii_ingest_end, lii_frame_select)
  bool map_fuse = true;                     // round 6 (LII_MAP_FUSE=0 turns both off): the fold's hash insert rides in k_map_decide, the inserts' cells in the fold launch
  bool ah_filled = false;                   // k_map_decide has filled the fold's table and no fold has consumed it yet
  long long ah_cleared = 0;                 // ... times such a fill had to be cleared (a list that outgrew its bound)
  bool fold_sorted = false;                 // LII_TEST=fold_sort: lii_map_incremental folds through the batch sort as lii_map_add_points does
  DevBuf<int> d_mapctr;            // kMapCtr* counters
  int n_used = 0;                     // host copy of kMapCtrUsed as of the last map_counters()
  bool map_dirty = false;             // an update has been enqueued since the last map_counters(): n_map / n_used / n_blocks are stale
  DevBuf<unsigned long long> d_keys_a, d_keys_b;
  DevBuf<unsigned int> d_idx_a, d_idx_b;
  DevBuf<BlockEntry> d_blocks;   // capacity-managed (grows on demand)
  unsigned int block_mask = 0;      // d_blocks.size() - 1
  DevBuf<uint2> d_cells;         // capacity-managed: 512 entries per occupied block
  size_t cells_cap_blocks = 0;      // = d_block_key.size(): blocks the six cell tables hold (build_index)
  int n_blocks = 0;
  int partial_stride = 0;
  int n_map = 0;
  float cell_size = 0.3f;
  DevBuf<unsigned char> d_sort_temp;  // temporary storage of the sorts and scans (size(): bytes)
  // lii_map_nearest (host form): staging for one chunk of queries and its results, device and pinned, laid out alike (queries |
  // counts | points | d2).  Created by the first call, grown geometrically up to kRowsMax rows (17 MiB each), kept until the handle goes.
  // lii_map_radius (host form) stages through the same two buffers and grows them beyond kRowsMax only for a single ball of more rows.
  struct MapQuery {
    static constexpr size_t kQueriesMax = 65536, kRowsMax = size_t(1) << 20;  // per chunk: queries, and rows (queries x k)
    DevBuf<unsigned char> d_buf;
    PinnedBuf<unsigned char> h_buf;
    size_t rows = 0;  // both hold min(rows, kQueriesMax) queries and `rows` result rows
  } mq;
  // lii_map_radius / lii_map_radius_dev: what the ball query needs beyond mq.  Nothing here exists before the first such call; every
  // buffer grows geometrically and goes with the handle.
  struct MapRadius {
    DevBuf<long long> d_off;             // host form: the offsets of one chunk of queries (kQueriesMax + 1)
    DevBuf<unsigned char> d_temp;        // temporary storage of the scan and of the sort
    DevBuf<unsigned long long> d_key_a, d_key_b;  // LII_RADIUS_SORTED: (query << 32 | d2 bits) per row, before and behind the sort
    DevBuf<unsigned int> d_slot_a, d_slot_b;      // ... and the row's slot in the point array
  } mr;
  // lii_map_crispness: one term per selected point and the figures of the reduction.  Nothing here exists before the first such call;
  // d_terms grows geometrically and goes with the handle.  (The selection itself runs through scratch of the map build - d_idx_a,
  // d_idx_b, d_map - which is free between two builds; lii_map_surface needs nothing beyond mq.)
  struct MapSurface {
    DevBuf<lii::SurfaceTerm> d_terms;
    DevBuf<lii::CrispnessSums> d_sums;
  } msf;
  // lii_pose_score / lii_pose_score_dev (kernels: lii_score.hip).  Nothing here exists before the first such call; every buffer grows
  // geometrically and goes with the handle.  d_part serves both forms; the others stage one chunk of poses of the host form.
  struct PoseScore {
    static constexpr size_t kPairsMax = size_t(1) << 22;  // (pose, point) pairs of one chunk of the host form: 16 MiB of res
    DevBuf<lii::ScorePartial> d_part;       // one record per workgroup of k_pose_score
    DevBuf<double> d_poses;                 // 12 per pose
    DevBuf<lii::ScorePartial> d_scores;     // lii_pose_score's layout
    DevBuf<float> d_res;
    PinnedBuf<double> h_poses;
    PinnedBuf<lii::ScorePartial> h_scores;
    PinnedBuf<float> h_res;
  } psc;
  // lii_pose_refine / lii_pose_refine_dev (kernels: lii_refine.hip).  Nothing here exists before the first such call; every buffer grows
  // geometrically and goes with the handle.  The first four serve both forms; the others stage the poses and records of the host form.
  struct PoseRefine {
    static constexpr size_t kPairsMax = size_t(1) << 22;  // (pose, point) pairs of one call: 33 bytes of scratch each - 132 MiB at the limit
    DevBuf<lii::RefineCtrl> d_ctrl;         // one record per pose
    DevBuf<double> d_planes;                // 4 per pair
    DevBuf<unsigned char> d_flags;          // the pair's selection
    DevBuf<lii::RefinePartial> d_part;      // one record per workgroup of k_refine_pass
    DevBuf<double> d_poses;                 // 12 per pose
    DevBuf<lii::RefineRecord> d_records;    // lii_pose_refined's layout
    PinnedBuf<double> h_poses;
    PinnedBuf<lii::RefineRecord> h_records;
  } prf;

  // ---- scan
  DevBuf<float4> d_scan;   // raw / undistorted (x,y,z,t_ms)
  // lii_frame_select: the frame stays where the ingest left it until something reads the scan - lii_scan_register takes it from
  // there like a caller's device buffer (lii_scan_job::scan_dev), every other reader copies it into d_scan first (scan_materialize)
  const float4* scan_pending = nullptr;  // (a frame of the ingest ring: not the handle's)
  int scan_pending_n = 0;
  // lii_scan_upload_next / lii_scan_advance: the next scan travels on a copy stream into a second buffer
  DevBuf<float4> d_scan_next;
  PinnedBuf<float4> h_stage_next;   // pinned staging for sources that are not (pinned, stride 16)
  lii::Event ev_next;      // the transfer of the next scan
  lii::Event ev_scan_free; // the compute stream has finished with the buffer the next transfer writes to
  int n_scan_next = -1;              // >= 0: a scan is waiting in d_scan_next
  const void* pin_cache_ptr[8] = {};  // lii_scan_upload_next: the last source buffers and whether the copy engine can read them directly
  bool pin_cache_direct[8] = {};
  int pin_cache_at = 0;
  bool scan_buf_idle = false;        // everything ever enqueued on the CURRENT scan buffer is known to have completed (an update's result came back behind it,
                                     // nothing touched the buffer since): lii_scan_upload_next may write the other buffer - the one that was current before the
                                     // last lii_scan_advance - without an event between the two streams
  // the time sort of a scan (lii_scan_job::scan_sorted == 2, lii_scan_sort): created by the first sort (scan_sort_buffers), sized from
  // max_scan_points; nothing else uses them (d_sort_temp may be in use by a map update on map_stream)
  struct ScanSort {
    DevBuf<unsigned int> d_key_a, d_key_b, d_idx_a, d_idx_b;
    DevBuf<float4> d_out;            // a scan that sits in d_scan is gathered into this buffer, and the two are swapped
    DevBuf<unsigned char> d_temp;    // temporary storage of sort_pairs_u32
  } ssort;
  // the optional per-point intensity channel (lii_scan_intensity_*, lii_ingest_set_intensity): one float per point beside the float4
  // clouds, in buffers of their own - created by the first call that attaches intensities (max_scan_points each), never by lii_create
  struct Intensity {
    DevBuf<float> d_scan;      // of the current scan, in the scan's current order (valid while `have`)
    DevBuf<float> d_sort_out;  // the time sort gathers into this buffer, and the two are swapped (created by the first sort that carries intensity)
    DevBuf<float> d_body;      // of the down-sampled cloud, in the device's order (valid while `body_have`): PCL's centroid of the voxel's members
    bool have = false;         // the current scan has intensities: whatever replaces the scan clears it (intensity_detach)
    bool body_have = false;    // the voxel filter / lii_downsample_skip that made the current down-sampled cloud carried them
  } inten;
  DevBuf<float4> d_body;   // down-sampled body points
  DevBuf<float4> d_world;
  DevBuf<float4> d_nbr;    // 5 x cap
  DevBuf<int> d_nbr_count;
  DevBuf<double> d_plane;
  DevBuf<unsigned char> d_selected;
  DevBuf<unsigned char> d_ctrl_poses;  // control block | pose table: one allocation, so that one upload carries both
  IekfCtrl* d_ctrl = nullptr;   // device-resident loop state of lii_iekf_update (the head of d_ctrl_poses)
  DevBuf<PoseArg> d_pose;    // pose slot of the host-driven lii_iekf_iterate
  PinnedBuf<unsigned char> h_ctrl_poses;  // pinned upload image of d_ctrl_poses
  IekfCtrl* h_ctrl = nullptr;   // the head of h_ctrl_poses
  PinnedBuf<IekfResult> h_res;  // pinned, device-mapped: written by the solve kernel of the stopping iteration
  lii_pose6d* h_poses = nullptr;  // pinned staging of the IMU pose table (inside h_ctrl_poses, kCtrlBytes in)
  int update_seq = 0;           // IekfCtrl::seq of the last update (never 0)
  bool poll_result = true;      // LII_TEST=sync_result: end an update with hipStreamSynchronize instead of polling IekfResult::done
  bool poses_preloaded = false, ctrl_preloaded = false;  // lii_scan_register uploaded them already
  lii::Event ev_poses;  // the last pose-table upload
  lii::Event ev_stage;  // the last scan upload through h_stage
  bool host_solve = false;      // LII_TEST=host_solve: drive the loop from the host (A/B, reference arrangement)
  DevBuf<double> d_partials;
  DevBuf<double> d_out91;
  DevBuf<unsigned long long> d_gran;  // k_reduce_solve: the 91 sums of a pass on their way to the solver, 2 x 91 tagged words; [200 ..]: the gap trace's stamps; [240]: the scan's largest count of unfinished queries so far
  DevBuf<unsigned long long> d_extent;  // 2 x {min (time|index), max time}: ping-pong accumulators
  DevBuf<unsigned int> d_mm;           // 2 x {min xyz, max xyz} (order-preserving uints)
  int extent_sel = 0, mm_sel = 0;
  bool knn_plan = true;        // LII_KNN_PLAN=0: every k-NN launch is enqueued (IekfCtrl::plan_mask)
  bool test_pred_small = false;
  bool test_force_rebuild = false;  // LII_TEST=force_rebuild: every in-place map update rebuilds the index first (the branch a map low on room takes)
  int solo_share = 0;             // LII_TEST=solo_share=<N>: kernel-timing rehearsal of one rank's share (N > 1: by voxel, N < -1: by index)
  bool no_gather = false;         // LII_TEST=no_gather: no gather areas behind the mailbox slots (the map update of a sharded job repeats the search)
  bool no_fast_prologue = false;  // LII_TEST=no_fast: a time-sorted scan takes the general path as well (k_time_extent in front of the de-skew)
  bool no_fuse = false;        // LII_TEST=no_fuse: lii_scan_register keeps the de-skew and the voxel filter's insert in separate launches
  bool test_sum_lost = false;  // LII_TEST=sum_lost: one summing workgroup of k_reduce_solve never publishes - the solver's wait must end in LII_ERR_COMM
  bool test_emit_late = false; // LII_TEST=emit_late: every seventh workgroup of k_vhash_emit / k_map_decide publishes its count late: the others count its block themselves (prefix_below)
  int plan_passes_prev = 32;   // passes the update before the last one ran (the plan enqueues the larger of the last two)
  int knn_plan_force = -1;     // LII_TEST=plan_force=<mask>: use this plan for every update (tests: forces the parked path)
  unsigned int plan_next = 0xFFFFFFFFu, plan_cur = 0xFFFFFFFFu;
  long long map_repeats = 0;   // map updates repeated because a list outgrew its predicted size
  long long plan_parked = 0;   // updates that had to be continued by the host
  bool staging_busy = false;  // h_ctrl / h_poses were handed to the device by lii_scan_register and no wait has covered the read yet
  size_t ctrl_pending = 0;    // bytes of h_ctrl (+ poses) the next k_time_extent launch carries to d_ctrl; 0 = nothing pending
  bool extent_valid = false;  // d_extent[extent_sel] holds the time extent of d_scan (lii_scan_set_device computed it on the way)
  DevBuf<unsigned int> d_bbox_rows;  // one row per de-skew workgroup: bounding box of its output points
  int bbox_rows = 0;                    // rows valid for the current d_scan (0: the voxel filter makes its own pass)
  DevBuf<unsigned long long> d_vkeys_a, d_vkeys_b;  // sort keys of the voxel filter (kVoxKeyBits wide)
  DevBuf<unsigned int> d_vidx_b;
  DevBuf<unsigned long long> d_vcomp, d_vsplit;  // sample sort of the voxel filter (lii_vsort.hip)
  DevBuf<unsigned int> d_vhist;
  DevBuf<unsigned short> d_vbucket;
  DevBuf<unsigned int> d_vpcl_in, d_vpcl_out;  // PCL voxel index per input point / per output voxel
  VoxelHashBuffers vh = {};      // the voxel grid by hashing (the default; LII_VOXEL_FILTER=sort: the sample sort): the view the
                                 // launches take by value, its pointers filled from the owners below
  DevBuf<unsigned char> vh_slots;
  DevBuf<unsigned int> vh_slot_of, vh_next, vh_crowded;
  DevBuf<unsigned long long> vh_counts;
  unsigned int vh_epoch = 0;     // number of the last hashed filter run (VoxelHashBuffers::counts)
  bool voxel_sort = false;       // LII_VOXEL_FILTER=sort
  bool vh_pinned = false;        // LII_VOXEL_FILTER=hash: no probing
  float fuse_leaf = 0.f;         // lii_scan_register -> lii_undistort_imu: the voxel filter that follows runs at this leaf (0: none)
  float vh_inserted_leaf = 0.f;
  bool vh_inserted = false;      // ... and the de-skew has filled the hashed filter's table on the way (lii_downsample goes on from there)
  int vh_mode = 1;               // 1: sparse voxels (hashed filter), 0: crowded voxels (sample sort)
  float vh_leaf = -1.f;          // the leaf size the choice was probed for
  unsigned int vh_watch = 0;
  unsigned long long vh_calls = 0, vh_due = 0;  // filter runs so far; the run at which the pending `crowded` read-back is applied
  bool voxel_path_hash = false;  // the path the last filter took
  PinnedBuf<unsigned int> h_vh_crowded;  // pinned: VoxelHashBuffers::crowded of the last hashed filter (read lazily)
  lii::Event ev_vh;
  bool vh_flag_pending = false;
  bool body_partitioned = false; // the down-sampled cloud on this rank holds ITS voxels only (a voxel-partitioned job, fused filter): no split by index
  bool body_reordered = false;   // d_body is in the order of the voxels' first points: the download entry points restore the PCL order (pcl_perm)
  std::vector<int> pcl_perm;     // pcl_perm[r] = position in d_body of the r-th point in PCL order (valid while pcl_perm_valid)
  bool pcl_perm_valid = false;
  double* d_poses = nullptr;     // the IMU pose table (inside d_ctrl_poses, kCtrlBytes in)
  int n_scan = 0, n_body = 0;   // n_body is an upper bound while n_body_pending (the exact count lives in d_nbody)
  bool n_body_pending = false;
  int last_filtered = 1;
  DevBuf<int> d_nbody;       // [0] size of the down-sampled cloud, [1] `filtered` flag of the last voxel filter
  bool body_is_scan = false;
  bool have_search = false;
  DevBuf<int> d_flags;       // the lists of unfinished queries (RegistrationBuffers::flag_count / flag_list): 2 counters + 2 x kFlagCap entries of two float4
  int knn_epoch = 0;            // number of the last enqueued search launch (never 0 again once used)
  int last_pivoted_passes = 0;  // lii_last_solve_info: passes of the last device update whose elimination needed the pivoting routine
  bool map_async = false;            // the update on map_stream may still be running (map_join waits for it: ev_mapflag is its last packet)
  int bound_add = 0, bound_nodown = 0;  // ... the sizes the update in flight was enqueued for
  int list_hist[8][2] = {};             // ... from the sizes of the last eight calls (note_list_sizes)
  int list_hist_n = 0;
  int pred_add = -1, pred_nodown = -1;  // lii_map_incremental: list sizes the next update is enqueued for (< 0: none yet)
  bool map_after_update = false;        // lii_scan_job::map_update: the iterated update in progress enqueues the map update behind its passes
  bool map_enqueued_early = false;      // ... and did (update_on_device -> map_update_early)
  bool lists_predicted = false;         // the update in flight ran on predicted sizes: commit_map checks it against the exact ones
  lii::Event ev_lists;        // the two lists are complete (compute stream -> map stream)
  PinnedBuf<int> h_mapflag;       // pinned, behind the last in-place update: [0..15] the map counters, [16..20] the list counts of
                                  // lii_map_incremental (k_map_decide) - read by commit_map / map_join
  lii::Event ev_mapflag;
  unsigned int decide_epoch = 0;     // runs of k_map_decide so far (its in-launch exchange of block counts tells its words from older ones by it)
  int map_seq = 0;                   // number of the last in-place update: k_map_publish leaves it in h_mapflag[kMapFlagSeqAt] behind the counters
  bool map_flag_pending = false;
  bool diag = false;     // LII_DIAG=1: counters of the rare paths on stderr when the handle is destroyed

  // ---- the pre-armed prologue (lii_launch.h: DeskewGate; lii_scan_job::next_scan_dev)
  struct Prearm {
    PinnedBuf<lii::GateState> state;         // pinned, device-mapped: the state word
    DevBuf<double> d_ring;                // device memory the HOST writes (large BAR): kGateRing records of kGateLines x 8 doubles
    DevBuf<unsigned long long> d_flag;
    unsigned long long seq = 0;
    bool enabled = true;                     // LII_PREARM=0: a job's next_scan_dev is ignored
    bool armed = false;                      // a gated de-skew launch sits on the stream, waiting for its record
    const void* scan_dev = nullptr;          // ... enqueued for this scan,
    int n = 0;
    float leaf = 0.f;                        // ... this leaf,
    bool fuse = false;                       // ... with the hashed filter's insert riding along or not
    bool late = false;                       // ... which was still being uploaded then (lii_scan_upload_next): read in place, behind the wait
    bool want_late = false;
    const void* want_dev = nullptr;          // lii_scan_register -> update_on_device: the job in progress names this next scan
    int want_n = 0;
    float want_leaf = 0.f;
    long long timeout_ticks = 200000000ll;   // 2 s of the 100 MHz clock (LII_PREARM_TIMEOUT_MS)
    long long n_used = 0, n_cancelled = 0, n_expired = 0;  // LII_DIAG
  } pre;

  // ---- pinned staging
  PinnedBuf<float4> h_stage;     // max(max_scan, max_map) float4
  PinnedBuf<PinnedScratch> h_small;  // one record: the small scratch, member by member (above)

  // ---- calibration
  struct CalibState {  // lii_capi_calib.cpp: the LI_init evaluators' buffers
    DevBuf<double> d_cal_imu, d_cal_lidar, d_cal_params, d_cal_out;
    int n_cal = 0;

    bool li_init_device = false;  // lii_li_init_set_device: zero-phase filter + cross-correlation of lii_li_init_run on the device

    // lii_li_init_resident / lii_calib_solve_stage_dev (lii_li_init_resident.hip).  Nothing here exists before the first such call; the
    // buffers grow geometrically and are never released before the handle goes.
    struct Resident {
      DevBuf<double> d_seq;    // sized by cap_n: the sequences (in place, as views), the stage-3 copies, the filter's hand-over, the correlation
      DevBuf<double> d_raw;    // sized by cap_raw: the raw IMU states of the interpolating form, their filtered accelerations and stamps
      DevBuf<double> d_small;  // the control block and the result block
      int cap_n = 0, cap_raw = 0;
      bool have_run = false;            // a resident run has succeeded: lii_li_init_resident_fetch serves it
      int ib12 = 0, lb12 = 0, n12 = 0;  // ... the view of the stage 1/2 sequences in d_seq
      int n3 = 0;                       // ... the length of the stage 3 copies
    } res;
    // lii_li_init_windows (lii_li_init_resident.hip): K sub-ranges of one upload, every window in areas of its own.  Nothing here
    // exists before the first such call; each buffer grows geometrically and is never released before the handle goes.  The call
    // reads and writes nothing of `res` or of the d_cal_* buffers above.
    struct Windows {
      DevBuf<double> d_src;    // the job's sequences as uploaded: IMU records, then LiDAR records
      DevBuf<double> d_seq;    // K areas of WinLayout::doubles(longest window)
      DevBuf<double> d_fts;    // raw form: K areas of 4 doubles per raw IMU state of the longest window (filtered accelerations, stamps)
      DevBuf<double> d_small;  // K control + result blocks
      DevBuf<lii_li_init_window> d_win;
      PinnedBuf<double> h_back;  // the K control + result blocks on their way back
      long long allocations = 0; // allocations made by all calls so far (lii_li_init_windows_scratch)
    } win;
  } cal;
  // ---- IMU processing (lii_capi_imu.cpp, lii_imu.hip)
  struct ImuState {
    lii_imu_noise noise{};
    bool have_noise = false, have_carry = false;
    DevBuf<double> d_buf;       // carry (ping) | carry (pong) | number of poses (an int) | a propagated state (stand-alone calls); created on first use
    int carry_sel = 0;          // which of the two carries is current
    PinnedBuf<double> h_in;     // pinned: state | samples of a stand-alone lii_imu_propagate / lii_cv_propagate
    PinnedBuf<double> h_out;    // pinned, device-mapped: propagated state | carry | number of poses, written by the kernels
    double* d_carry(int sel) const { return d_buf.get() + lii::kImuCarryDoubles * sel; }
    int* d_n_poses() const { return reinterpret_cast<int*>(d_buf.get() + 2 * lii::kImuCarryDoubles); }
    double* d_state() const { return d_buf.get() + 2 * lii::kImuCarryDoubles + 8; }
  } imu;
  // ---- the registered clouds of a scan (lii_capi_publish.cpp, lii_publish.hip): a standing order, off by default.  Nothing here
  // exists before the first lii_publish_set; the clouds land in buffers of their own, two deep (slot `cur` is the one the
  // registration under way writes, `have` the one of the last finished registration), aliased onto nothing else of the handle.
  struct Publish {
    static constexpr int kClouds = 4;  // bit k of lii_publish_opts::clouds: dense, down-sampled, effect, body
    bool on = false;
    int clouds = 0, to_host = 0, save_capacity = 0;
    DevBuf<float4> d_cloud[kClouds][2];     // max_scan_points each (the ordered ones)
    PinnedBuf<float4> h_cloud[kClouds][2];  // to_host: their pinned copies, filled on the copy stream
    DevBuf<int> d_counts;                   // per slot: [0] points of the down-sampled cloud, [1] of the effect cloud
    PinnedBuf<int> h_counts;                // ... and in mapped host memory (4 ints per slot)
    DevBuf<unsigned long long> d_words;     // k_publish_world's in-launch prefix: one word per 256 down-sampled points
    unsigned int epoch = 0;                 // launches so far
    lii::Event ev_pub[2];                   // the slot's launch (and body copy) has completed (handle's stream)
    lii::Event ev_copy[kClouds][2];         // the slot's cloud has arrived in h_cloud (copy stream)
    int last_copy[2] = {-1, -1};            // the cloud whose ev_copy was recorded last for the slot (-1: no copy enqueued yet)
    // LII_PUB_INTENSITY: the intensities of the dense / down-sampled / body cloud (index 0 / 1 / 2), two deep like the clouds
    static constexpr int kIntClouds = 3;
    bool intensity = false;                 // the bit is ordered
    DevBuf<float> d_int[kIntClouds][2];     // max_scan_points each (the ordered ones)
    PinnedBuf<float> h_int[kIntClouds][2];  // to_host: their pinned copies (copy stream, IN FRONT of the slot's cloud copies: last_copy covers them)
    lii::Event ev_int[2];                   // the slot's intensities have arrived in h_int (copy stream)
    int int_at[2] = {0, 0};                 // the LII_PUB_* clouds whose intensities the slot holds (0: the registered scan had none)
    DevBuf<float> d_save_int;               // the save buffer's intensities: appended in lock-step with d_save by the same launch
    DevBuf<float4> d_save;                  // pcl_wait_save: save_capacity points (created by the first order that asks for it)
    DevBuf<int> d_save_ctl;                 // [save_par]: append offset, [save_par ^ 1]: written by the next launch, [2]: sticky overflow flag
    int save_par = 0;
    int cur = 0, have = -1;
    int n_scan_at[2] = {0, 0};              // points of the dense / body cloud in the slot
    int clouds_at[2] = {0, 0};              // the clouds the slot holds
    int kp_idx = -1;                        // lii_set_profiling(h, 3): the mark of the launch enqueued behind the planned passes
    // lii_publish_wire_set: the second standing order - the clouds as 48-byte pcl::PointXYZINormal records, formed by the same launch.
    // Independent of `on`: either order alone keeps the launch, the slots (cur / have), the counts and the prefix words going.
    struct Wire {
      bool on = false;
      int clouds = 0, to_host = 0;
      DevBuf<uint4> d_cloud[kClouds][2];     // lii::kWireQuads * max_scan_points each (the ordered ones)
      PinnedBuf<uint4> h_cloud[kClouds][2];  // to_host: their pinned copies, filled on the copy stream behind the float4 clouds'
      lii::Event ev_copy[kClouds][2];        // the slot's records have arrived in h_cloud (copy stream)
      int last_copy[2] = {-1, -1};           // as Publish::last_copy, for these copies
      int clouds_at[2] = {0, 0};             // the clouds the slot holds as records
      DevBuf<uint4> d_pcd;                   // lii_publish_saved_pcd: the staging area, 2 * lii::kPcdChunkRows (one chunk of 32-byte rows)
    } wire;
    bool any() const { return on || wire.on; }
  } pub;
  // ---- the moving local-map cube (lii_local_map_*, lii_capi_map.cpp; kernels: lii_map.hip, arithmetic: lii_fov.h): durable handle state,
  // off until lii_local_map_set asks for it.  Nothing here exists before the first lii_local_map_set.
  struct LocalMap {
    bool set = false;        // lii_local_map_set has been accepted once (lii_local_map_segment works from then on)
    bool enabled = false;    // every registration call segments by itself
    float det_range = 0.f;
    lii::LocalMapParams P{};
    DevBuf<lii::LocalMapState> d_state;    // two copies: call k reads [cur], writes [cur ^ 1]
    PinnedBuf<lii::LocalMapState> h_state; // the copy the last call's last launch leaves for the host
    int cur = 0;
    int seq = 0;                 // number of the last enqueued call
    bool in_job = false;         // scan_register_job -> update_on_device: this update segments behind commit_map, in front of its first search
    bool counts_pending = false; // a call has been enqueued whose deletes the host's copy of the live-point count does not hold yet
  } lm;
  // ---- the history of what box deletes remove (lii_map_removed_*, lii_capi_map.cpp; collected by the squeeze of a box delete, lii_map.hip):
  // a standing order, off by default.  Nothing here exists before the first lii_map_removed_set that asks for a buffer.
  struct Removed {
    bool set = false;            // lii_map_removed_set has been accepted once (get / acquire / view work from then on)
    bool on = false;             // box deletes collect
    int cap = 0;                 // points d_buf holds (the capacity of the last order that asked for a buffer)
    DevBuf<float4> d_buf;
    DevBuf<unsigned long long> d_ctr;  // [0]: RemovedSink::reserved
    long long collected_base = 0, lost_base = 0;  // the totals up to the last clear (what the buffer holds now is counted on top)
  } rm;
  void* ingest = nullptr;  // lii_ingest.hip state (frames of the last driver message)
  bool ingest_sort_always = false;  // LII_INGEST_SORT=always: the ingest never leaves the time sort out (IngestRing::never_predict)

  // ---- comm
  struct CommState {  // lii_capi_comm.cpp: the communicator of a sharded job
    ncclComm_t comm = nullptr;   // RCCL transport (ranks on several nodes, or forced)
    MailboxHost mailbox;         // node-local transport: the exchange happens inside k_reduce_solve
    DevBuf<unsigned long long> d_mb_seq;
    DevBuf<unsigned int> d_gather_ticket;  // the list exchange of lii_map_incremental (lii_exchange.hip): its ticket word,
    DevBuf<unsigned char> d_gx;            // RCCL form of the list exchange: send block | N gathered blocks | N headers | pointer tables
    size_t gx_block = 0; int gx_ranks = 0;    // ... laid out for this block size (64 + 16 max_scan_points) and this many ranks
    unsigned long long gather_seq = 0;        // ... and the exchanges enqueued so far (the ranks call in lock-step: the same on all)
    long long mailbox_timeout_ticks = 3000000000ll;  // 30 s (LII_MAILBOX_TIMEOUT_S): ranks may start a scan seconds apart
    double mailbox_wait_s = 20.0;   // how long lii_comm_init waits for all ranks in the node-local segment (LII_MAILBOX_TIMEOUT_S=<exchange>,<set-up>)
    int n_ranks = 1, rank = 0;
    std::string comm_why;           // which transport this rank ended up with and why (lii_comm_describe)
    bool library_partition = true;  // lii_comm_set_partition: the library splits the down-sampled cloud over the ranks (every rank
                                    // hands over the whole scan); false: the caller hands every rank its own points
    bool voxel_partition = false;   // lii_comm_set_partition(h, 2): ... by VOXEL where the filter is fused into the de-skew (this rank
                                    // filters and registers the voxels whose key hashes to it), by index otherwise
  } net;

  // ---- profiling
  struct ProfState {  // lii_set_profiling / lii_last_timings / lii_last_kernel_profile, LII_DIAG
    bool kp_active = false;            // inside a lii_scan_register that is being profiled launch by launch
    int prof_mode = 0;                 // the last lii_set_profiling value; 3: an event in front of every launch of lii_scan_register
    std::vector<lii::Event> kp_ev;     // ... the events (created on demand, reused),
    std::vector<int> kp_kind;          // ... kind * 64 + iteration of the launch behind each (kind LII_KP_KINDS: end mark)
    int kp_n = 0;
    lii_kernel_profile kprof{};
    bool profiling = false;
    lii::Event ev[4];
    lii::Event ev_it[32];              // per-iteration brackets of the k-NN kernel in the device-driven loop
    unsigned int ev_it_due = 0u;       // iterations whose pair of ev_it holds a k-NN launch that has not been read yet (harvest_knn_events)
    double timings[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double host_map_us[2] = {0, 0};  // LII_DIAG: per update - waiting for the map update in flight (commit_map), enqueueing the map update behind the passes
    double host_us[6] = {0, 0, 0, 0, 0, 0};  // LII_DIAG: per lii_scan_register - entry -> first launch, -> pre-processing enqueued, -> loop enqueued, -> result; calls; gap between calls
    std::chrono::steady_clock::time_point host_last_return;
    double host_loop_enq_us = 0;
  } prof;
  // ---- the per-point measurement noise (lii_point_noise_*, lii_capi_register.cpp): a standing setting, model 0 by default.  The buffer
  // does not exist before the first lii_point_noise_set with model 1.
  struct PointNoise {
    int model = 0;                  // 0: R_inv = laser_point_cov_inv for every point; 1: range / bearing (calcBodyVar)
    double range_inc = 0.0, degree_inc = 0.0;  // as set (lii_point_noise_get)
    // the model's constants as the fit launches read them (lii::NoiseArg, kNoiseHeadBytes) | max_scan_points floats: one allocation, so
    // that the launch finds the constants through the pointer it carries anyway
    DevBuf<unsigned char> d_buf;
    float* d_sqrt_rinv() const { return d_buf ? reinterpret_cast<float*>(d_buf.get() + lii::kNoiseHeadBytes) : nullptr; }  // RegistrationBuffers::sqrt_rinv
    bool have_pass = false;         // a fit pass has written the buffer since the model was set (lii_point_noise_download)
  } noise;
};


namespace lii_impl {
using namespace lii;

int fail(lii_handle h, int code, const std::string& msg);
inline unsigned int next_pow2(unsigned int v) {
  unsigned int p = 1;
  while (p < v) p <<= 1;
  return p;
}
// lii_capi.cpp
int kp_mark(lii_handle h, int kind, int it = 0);
void harvest_knn_events(lii_handle h);
GridView grid_view(const lii_context* c);
RegistrationBuffers reg_buffers(const lii_context* c);
PoseArg pose_of(const lii_state& s);
int resolve_n_body(lii_handle h);
bool fuse_filter(lii_handle h, float leaf);  // does the de-skew of this scan fill the hashed voxel filter's table on the way?
// The one place that fills a DeskewPlan (bbox_rows, vh, the control-block pull and the LII_GAP_TRACE field are its business).  ctrl:
// none - a stand-alone de-skew (lii_undistort_imu / _cv); ahead - a registration call whose control block a launch in front has pulled
// (k_imu_propagate); pulled - a registration call whose de-skew launch pulls the block itself, with one extra workgroup.
enum class DeskewCtrl { none, ahead, pulled };
DeskewPlan deskew_plan(lii_handle h, const float4* in, float4* out, int n, bool sorted, const unsigned long long* extent, float leaf, bool fused,
                       DeskewCtrl ctrl);
int pcl_order(lii_handle h, const int** perm);
void extent_discard(lii_handle h);
// `src` (n points: a caller's device buffer, a frame of the ingest, or d_scan itself) -> d_scan in ascending time order, stable; the
// launches go on the handle's stream, `src` is only read.  Does not touch the handle's book-keeping of the scan (n_scan, extent, ...).
int scan_sort_into(lii_handle h, const float4* src, int n);
void intensity_detach(lii_handle h);  // the current scan has been replaced: its intensities, and those of the down-sampled cloud, are void
int intensity_buffers(lii_handle h);  // creates lii_context::inten's scan / down-sampled buffers on first use
int scan_materialize(lii_handle h);  // a frame selected by lii_frame_select and not read yet -> d_scan (lii_scan_set_device)
bool gate_move(lii::GateState* st, unsigned long long seq, unsigned long long to);  // the state word: armed -> `to`, if still armed
void prearm_cancel(lii_handle h);  // a gated de-skew launch that waits on the stream is told to end (every entry point that uses the stream calls this first)
void prearm_arm(lii_handle h);  // update_on_device: the launch for the scan the job announced (lii_context::pre.want_*) goes out behind the passes, gate armed
bool prearm_go(lii_handle h, const lii_state* state, const lii_pose6d* poses, int K);  // the gate to GO and the record into the ring; false: the launch had given up
unsigned long long* extent_of_scan(lii_handle h);
MailboxView mailbox_view(lii_handle h);
lii::GatherView gather_view(lii_handle h);  // .peers == nullptr: this job has no list exchange (single rank, host-memory mailbox, RCCL)
// lii_capi_map.cpp
int build_index(lii_handle h, int n, int extra_blocks = 0);
void note_list_sizes(lii_handle h, int n_add, int n_nodown);
int map_join(lii_handle h);
constexpr int kMapFlagSeqAt = 40;  // (h_mapflag: 64 ints; [0, kMapCtrWords + 8): the counters and list sizes)
int map_update_early(lii_handle h);  // 1: enqueued behind the passes of the update in progress, 0: not possible this time, < 0: error
int commit_map(lii_handle h);
int map_counters(lii_handle h, bool already_synced = false);
lii::RemovedSink removed_sink(lii_handle h);  // the history buffer as the launches of a box delete take it (buf == nullptr: nothing is collected)
// one lasermap_fov_segment + Delete_Point_Boxes on the handle's stream (three launches); pos_dev: state.pos_end in device memory, else pos by
// value.  The caller has joined the map update in flight.  mark: lii_set_profiling(h, 3) brackets the launches (LII_KP_VOXEL)
int local_map_enqueue(lii_handle h, const double* pos_dev, const double* pos, bool mark);
void local_map_settle(lii_handle h);  // the stream has passed the last enqueued call: the host's live-point count takes its result
int map_gather(lii_handle h, int* n_out);
int map_rebuild(lii_handle h, int extra_blocks);
int map_apply(lii_handle h, const float4* list, int n_list, bool downsample, const float4* extra, int n_extra, bool beside = false,
              const int* n_list_dev = nullptr, const int* n_extra_dev = nullptr, bool count_events = true, bool prefilled = false);
// lii_capi_register.cpp / lii_capi_imu.cpp
// lii_scan_register_imu hands lii_scan_register's job to the same routine with the scan's IMU samples instead of a pose table
struct ImuFeed {
  const lii_imu_sample* imu;
  int n_imu;
  double pcl_beg_time;
  lii_state* prop_out;  // may be nullptr
};
// ... and lii_scan_register_cv with what the constant-velocity propagation of the LO phase needs
struct CvFeed {
  double dt;
  const double* cov_gyr_scale;  // [3]
  const double* cov_acc_scale;  // [3]
  lii_state* prop_out;          // may be nullptr
};
int scan_register_job(lii_handle h, const lii_scan_job* job, lii_state* state, const lii_state* state_prop, lii_iekf_report* report, const ImuFeed* feed,
                      const CvFeed* cv = nullptr);
int imu_buffers(lii_handle h);  // creates lii_context::imu's buffers on first use
// lii_capi_publish.cpp: the standing order of lii_publish_set.  publish_enqueue puts the launch (+ event, + copies to the host) for slot
// pub.cur on the stream - guard != nullptr: behind the passes of the update under way, pose from the control block; else at `ps` -,
// publish_finish makes that slot the one lii_publish_fetch serves.
int publish_enqueue(lii_handle h, const IekfCtrl* guard, const PoseArg* ps, bool first);
void publish_finish(lii_handle h);
// lii_capi_comm.cpp
void comm_drop(lii_handle h);
void partition_refresh(lii_handle h);  // the voxel filter's view of the job after the communicator or its partition changed
int lists_exchange_rccl(lii_handle h, hipStream_t s);  // the list exchange of lii_map_incremental over ncclAllGather; synchronises the stream once
}  // namespace lii_impl

// Host-callable launchers of the library's kernels, grouped by the unit that defines them (internal; not the C-ABI).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <string>

#include "lii_device.h"
#include "lii_fov.h"

struct lii_context;
// internal hooks of the handle for the translation units that live beside lii_capi.cpp (not exported in the C-ABI header)
int lii_internal_fail(lii_context* h, int code, const std::string& msg);
// The library's one check of a runtime call: a failure is recorded as "<call>: <the runtime's message>" and ends the caller with LII_ERR_HIP.
#define HIPCHK(h, call)                                                                                            \
  do {                                                                                                             \
    hipError_t e_ = (call);                                                                                        \
    if (e_ != hipSuccess) return lii_internal_fail(h, LII_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
int lii_internal_scan_defer(lii_context* h, const void* dev_float4, int32_t n);  // (lii_capi.cpp) lii_frame_select's hand-over
int lii_internal_scan_materialize(lii_context* h);  // (lii_capi.cpp) a selected frame nobody has read yet -> the handle's own scan buffer
int lii_internal_in_wait_hook(lii_context* h);       // (lii_capi.cpp) 1: inside lii_scan_job::while_waiting of a registration under way
int lii_internal_scan_is_deferred(lii_context* h);  // (lii_capi.cpp) 1: a selected frame that nobody has read yet
int lii_internal_intensity_refused(lii_context* h);  // (lii_capi.cpp) 1: a communicator is attached or LII_TEST=host_solve - no intensity channel
// (lii_capi.cpp) lii_frame_select's hand-over of the frame's intensities (dev_float == nullptr: the frame has none); copied on the handle's stream
int lii_internal_scan_intensity_adopt(lii_context* h, const float* dev_float, int32_t n);
void lii_internal_prearm_cancel(lii_context* h);  // (lii_capi.cpp) see lii_impl::prearm_cancel
hipStream_t lii_internal_stream(lii_context* h);
void** lii_internal_ingest_slot(lii_context* h);
void lii_internal_ingest_switches(lii_context* h, bool* diag, bool* sort_always);  // (lii_capi.cpp) LII_DIAG, LII_INGEST_SORT=always

namespace lii {
void ingest_destroy(void* slot);  // lii_ingest.hip

struct UndistArgH { double endR[9], endp[3], RLI[9], TLI[3]; };
struct CvArgH { double omega[3], vel[3], endR[9]; };

// map index (lii_mapindex.hip)
void launch_map_keys(const float4* pts, int n, float inv_cs, unsigned long long* keys, unsigned int* idx, hipStream_t s);
void launch_map_gather(const float4* src, const unsigned int* idx, int n, float4* dst, hipStream_t s);
void launch_body_to_map(const float4* body, int n, const PoseArg& ps, float4* dst, hipStream_t s, const float* inten = nullptr);  // pointBodyToWorld over a cloud: dst[i] = (world xyz, inten ? inten[i] : 0)
void launch_block_flags(const unsigned long long* keys, int n, unsigned int* flags, hipStream_t s);
void launch_table_clear(BlockEntry* blocks, unsigned int cap, hipStream_t s);
void launch_win_bbox(const BlockEntry* blocks, unsigned int cap, unsigned int* box, hipStream_t s);
void launch_win_fill(const BlockEntry* blocks, unsigned int cap, const uint2* cells, uint2* win, const int org[3], const int dim[3], hipStream_t s);
void launch_cells_fill(const unsigned long long* keys, const unsigned int* ranks, int n, BlockEntry* blocks,
                       unsigned int block_mask, uint2* cells, unsigned long long* key_of_id, hipStream_t s);
// map queries (lii_query.hip): Nearest_Search for n points (float xyz every stride_bytes, device memory), one wavefront each.
// n_entries / pts_cap: the sizes of the cell tables (entries) and of the point array (slots) behind `g`; max_d2: the largest float
// that is <= max_dist; r_max: rings of cells that cover the ball (ceil(sqrt(max_dist) / cell) + 1).  Row i * k + j of pts_out (3 floats)
// / d2_out: neighbour j of query i, zeros from count_out[i] on; pts_out / d2_out may be nullptr.
void launch_map_nearest(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, int k,
                        float max_d2, int r_max, float* pts_out, float* d2_out, int* count_out, hipStream_t s, int row_floats = 3);
// ... and the ball query (lii_map_radius): every point with d2 <= max_d2, in two walks of the same cells.  _count: count_out[i] = points in
// the ball of query i (64 bits, so that the scan below turns them into offsets in place).  _fill: the points of query i into rows
// offsets[i] - base .. offsets[i + 1] - base - 1, only rows < capacity; per row 3 floats of pts_out, d2_out, and - for LII_RADIUS_SORTED -
// key_out (query << 32 | d2 bits) and slot_out (the point's slot in the array); each of the four may be nullptr.  _gather: behind the sort
// of (key, slot), rows < min(total[0] - base, capacity): the key's d2 and the slot's point.
void launch_map_radius_count(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2,
                             int r_max, long long* count_out, hipStream_t s);
void launch_map_radius_fill(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2,
                            int r_max, const long long* offsets, long long base, long long capacity, float* pts_out, float* d2_out,
                            unsigned long long* key_out, unsigned int* slot_out, hipStream_t s, int row_floats = 3);
void launch_map_radius_gather(const GridView& g, unsigned int pts_cap, const unsigned long long* keys, const unsigned int* slots, const long long* total,
                              long long base, long long capacity, float* pts_out, float* d2_out, hipStream_t s, int row_floats = 3);
// row_floats (the three launches above): 3 - x, y, z a row of pts_out - or 4: the stored fourth word, the point's intensity, behind them
// (lii_map_nearest_xyzi / lii_map_radius_xyzi; instantiations of their own)
// surface statistics (lii_surface.hip): the ball of lii_map_radius reduced to its moments, one wavefront per query.
//   mean_rel = s1 / n,  C_ab = s2_ab / n - mean_rel_a * mean_rel_b   with s1, s2 the sums of d and d_a d_b, d = (double)m - (double)q,
// formed exactly so (no FMA); eig / normal: lii_eig3.h.  SurfaceRecord is lii_surface's layout, CrispnessSums lii_map_crispness's.
// viewpoint: a HOST pointer to 3 doubles, or nullptr (it travels in the kernel's arguments).
struct SurfaceRecord { int count, valid; double mean[3], eig[3], normal[3], curvature; };
enum { kSurfaceUsed = 0, kSurfaceSparse = 1, kSurfaceDegenerate = 2 };
struct SurfaceTerm { double h, eig0; int count, kind; };  // one selected point of lii_map_crispness: its entropy, eig[0], ball population, kSurface*
struct CrispnessSums { long long n_selected, n_used, n_sparse, n_degenerate; double mme, mpv, mean_count; };
void sym3_eigen_host(const double m[6], double eig[3], double vec[9]);  // lii_eig3.h's routine, compiled for the host in the unit that runs it on the device
void launch_map_surface(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2, int r_max,
                        const double* viewpoint, SurfaceRecord* out, hipStream_t s);
// ... the aggregate: terms[i] of query i (a sparse ball: count < min_count; a degenerate one: eig[0] <= 1e-12 eig[2]) instead of the record;
// _select: flags[i] = mix(point i) % every == 0; _compact: behind the inclusive scan of the flags, the selected points end to end;
// _reduce: one workgroup, a fixed order of additions - out[0] from the n terms (n == 0: zeros)
void launch_map_surface_terms(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2,
                              int r_max, int min_count, SurfaceTerm* terms, hipStream_t s);
void launch_surface_select(const float4* pts, int n, unsigned int every, unsigned int* flags, hipStream_t s);
void launch_surface_compact(const float4* pts, const unsigned int* flags, const unsigned int* ranks, int n, float4* dst, hipStream_t s);
void launch_crispness_reduce(const SurfaceTerm* terms, int n, CrispnessSums* out, hipStream_t s);
// pose scoring (lii_score.hip): the figures of one search pass (src/laserMapping.cpp:957-1020, all-true selection) at each of n_poses
// poses - 12 doubles each in device memory: rot_end row-major, pos_end; the extrinsic is `base`'s - over the n points of `body`.
// ScorePartial is lii_pose_score's layout: scores[k] receives pose k's figures, partials (pose_score_partials(n, n_poses) records of
// scratch) one workgroup's share each; res: nullptr, or n_poses x n floats (res_last).  Two launches whatever n_poses is.
struct ScorePartial { int n_full, effect_num; double total_residual; };
// Workgroups up to which four wavefronts search a workgroup's 64 pairs, one above it (launch_pose_score; launch_pose_refine takes it over
// unmeasured): an estimate (two wavefronts per SIMD) between measured points of k_pose_score at 512 (four win) and 8 192 (one wins) -
// DESIGN.md section 3.4i; the bits do not depend on it.
constexpr int kSmallBatchBlocks = 2048;
size_t pose_score_partials(int n, int n_poses);
void launch_pose_score(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const float4* body, int n, const PoseArg& base, const double* poses_dev,
                       int n_poses, int r_max, double plane_thr, ScorePartial* partials, ScorePartial* scores, float* res, hipStream_t s);
// pose refinement (lii_refine.hip): the iterated update of src/laserMapping.cpp:957-1134 in LO mode on the six pose states, `updates` times
// in a row from each of n_poses poses (laid out as for launch_pose_score) over the n points of `body`; P starts at `prior` for every pose.
// updates x max_iterations rounds of two launches, all enqueued here; records[k] (lii_pose_refined's layout) is written by the round in
// which pose k's last update ends.  The scratch belongs to the call while it runs: a control record per pose, a plane and a selection
// flag per (pose, point) pair, one partial per workgroup of a pass (pose_refine_partials(n, n_poses)).
constexpr int kRefineConverged = 1, kRefineBadPose = 2;  // LII_REFINE_CONVERGED, LII_REFINE_BAD_POSE
struct RefineRecord { double pose[12], cov[36], total_residual; int effect_num, iterations, searches, flags; };
struct RefinePrior { double P[36]; };
struct RefineCtrl {
  double R[9], p[3];    // the pose now
  double Rp[9], pp[3];  // state_propagat of the update under way
  double P[36];         // the covariance that update started with
  int search, done;     // the next pass searches; the last update has ended (or the pose was refused)
  int rem, it, upd;     // rematch_num and iterCount of the update under way; updates ended
  int iterations, searches, pad;
};
struct RefinePartial { double s[28]; int effect_num, pad; };  // 21 sums of h^T h (upper triangle, row by row), 6 of h^T z, sum |pd2|
struct RefineScratch { RefineCtrl* ctrl; double* planes; unsigned char* flags; RefinePartial* partials; };
size_t pose_refine_partials(int n, int n_poses);
void launch_pose_refine(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const float4* body, int n, const PoseArg& base, const RefinePrior& prior,
                        const double* poses_dev, int n_poses, int max_iterations, int updates, int r_max, double plane_thr, double rinv, const RefineScratch& sc,
                        RefineRecord* records, hipStream_t s);
// (lii_sort.hip) counts -> offsets in place: io[i] = io[0] + ... + io[i - 1] over n words; and the sort of the sorted form: bits [0, end_bit)
// of 64-bit keys with 32-bit values, stable.  *_temp_bytes: the temporary storage either needs for that size.
size_t scan_i64_temp_bytes(size_t n);
void exclusive_scan_i64(void* temp, size_t temp_bytes, long long* io, size_t n, hipStream_t s);
size_t sort_u64_bits_temp_bytes(size_t n, int end_bit);
void sort_pairs_u64_bits(void* temp, size_t temp_bytes, const unsigned long long* kin, unsigned long long* kout, const unsigned int* vin,
                         unsigned int* vout, size_t n, int end_bit, hipStream_t s);
// registration: the search launch (lii_knn.hip)
// (`pose`: device memory on every path - a host-driven pass uploads it first)
// epoch: the number of this search launch (> 0, RegistrationBuffers::flag_*) and of the fit launch behind it; 0: no list of unfinished queries
// ev_start / ev_stop (both or none): the launch's own dispatch carries the two events (hipExtLaunchKernelGGL: the time stamps of the
// dispatch packet's completion signal) - the kernel's duration without a barrier packet in front of and behind it on the stream
void launch_knn(const GridView& g, const RegistrationBuffers& rb, const PoseArg* pose,
                const IekfCtrl* ctrl, int forced, double* search_pose_out, hipStream_t s, int epoch,
                hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// registration: the fit launch and the completion of unfinished searches (lii_fit.hip)
#ifdef LII_FALLBACK_TRACE
void fb_trace_read(unsigned long long out[32]);  // (measurement builds: the completion's phase sums)
#endif
void launch_knn_complete(const GridView& g, const RegistrationBuffers& rb, hipStream_t s);
void launch_complete_listed(const GridView& g, const RegistrationBuffers& rb, const IekfCtrl* ctrl, int forced, hipStream_t s, int epoch);  // (k_complete_listed: behind search launch `epoch`)
// rb.sqrt_rinv != nullptr: lii_point_noise_set, model 1 - the instantiations with per-point weights; `rinv` is not used then
void launch_fit_reduce(const GridView& g, const RegistrationBuffers& rb, const PoseArg* pose,
                       const IekfCtrl* ctrl, int forced, int imu_en, double plane_thr, double rinv, hipStream_t s, int epoch);
void launch_reduce91(const RegistrationBuffers& rb, double* out91, const IekfCtrl* ctrl, int forced, hipStream_t s, int epoch);  // epoch: of the fit launch whose columns it sums
// final sum + 24-state solve, the ranks' sum of the normal equations (lii_iekf.hip)
void launch_reduce_solve(const RegistrationBuffers& rb, unsigned long long* gran, IekfCtrl* c, IekfResult* res, const MailboxView& mb,
                         hipStream_t s, int epoch);
void launch_mailbox_allreduce(double* out91, const MailboxView& mb, hipStream_t s);
// node-local mailbox (lii_mailbox.cpp)
struct MailboxHost {
  void* map = nullptr;        // the shared segment in this process (rendezvous; in the host-memory form also the slots)
  size_t bytes = 0;
  double* dev_slots = nullptr;  // host-memory form: device address of the segment's slot area
  bool registered = false;
  char name[64] = {0};        // non-empty while the segment still has a name to unlink
  // HBM form: the own slot area (fine-grained device memory, exported through a HIP IPC handle), the peers' areas as opened
  // here, and the device-resident table of all of them (MailboxView::peers)
  double* own = nullptr;
  double* peer_ptr[64] = {nullptr};
  double** d_peers = nullptr;
  int n_peers = 0;
  // ... and behind the slots of every area the gather area of the list exchange (GatherView; gather_points > 0 at set-up)
  unsigned char** d_gather_peers = nullptr;
  size_t gather_block = 0;
  int gather_cap = 0;
};
size_t mailbox_segment_bytes(int n_ranks);
// want_hbm: try the peer-mapped HBM form first (falls back to host memory inside the same rendezvous when a rank cannot
// export / open the handles).  Returns 0 on success (m->d_peers != nullptr: HBM form; else m->dev_slots: host-memory form).
// gather_points: capacity (float4) of one rank's lists in the exchange of lii_map_incremental (HBM form only; 0: no gather areas).
int mailbox_open(const uint8_t id[128], int n_ranks, int rank, double wait_s, bool want_hbm, int gather_points, MailboxHost* m, std::string* why);
// the list exchange (lii_exchange.hip): push this rank's lists (sizes in counts[0..1], device) into every rank's gather area, wait for
// all ranks' lists of exchange number `seq` (1, 2, ... - the same on every rank) and leave them concatenated in rank order in
// dst_add / dst_nodown (may be the sources), the totals in counts[0..1]; counts[err_at] = 1 when a rank did not deliver in time.
void launch_lists_push(const GatherView& gv, const float4* src_add, const float4* src_nodown, const int* counts, unsigned int* ticket,
                       unsigned long long seq, hipStream_t s);
void launch_lists_collect(const GatherView& gv, unsigned long long seq, float4* dst_add, float4* dst_nodown, int* counts, int err_at, hipStream_t s);
void launch_lists_exchange(const GatherView& gv, const float4* src_add, const float4* src_nodown, int* counts, int err_at, unsigned int* ticket,
                           unsigned long long seq, float4* dst_add, float4* dst_nodown, hipStream_t s);
void mailbox_close(MailboxHost* m);
void launch_loop_resume(IekfCtrl* c, unsigned int plan_mask, hipStream_t s);
void launch_iekf_solve(IekfCtrl* c, const double* ne, IekfResult* res, hipStream_t s);
int register_blocks(int n);  // (lii_fit.hip)
// undistortion (lii_scan.hip)
#ifdef LII_FRONT_TRACE
void front_trace_read(unsigned long long out[32]);  // (measurement builds: the phase sums of the de-skew and emit workgroups)
#endif
void launch_time_extent(const float4* pts, int n, unsigned long long* extent, unsigned long long* extent_next, float4* copy_to,
                        const void* ctrl_src, void* ctrl_dst, size_t ctrl_bytes, hipStream_t s);
// the time sort of a scan: key[i] = order-preserving image of t (-0.0 as +0.0), idx[i] = i; then sort_pairs_u32; then dst[i] = src[idx[i]]
void launch_sort_keys(const float4* pts, int n, unsigned int* key, unsigned int* idx, hipStream_t s);
// (inten_src != nullptr: the scan's intensities travel by the same idx, inten_dst[i] = inten_src[idx[i]])
void launch_sort_gather(const float4* src, const unsigned int* idx, int n, float4* dst, hipStream_t s, const float* inten_src = nullptr, float* inten_dst = nullptr);
// voxel grid (lii_scan.hip)
void launch_voxel_minmax(const float4* pts, int n, unsigned int* mm, unsigned int* mm_next, hipStream_t s);
void launch_voxel_keys(const float4* pts, int n, const unsigned int* mm, const unsigned int* bbox_rows, int n_rows, float leaf,
                       unsigned long long* keys, unsigned int* pcl_keys, int* filtered_dev,
                       unsigned long long* samples, int sample_width, hipStream_t s);
// the voxel grid by hashing (lii_scan.hip: k_vhash_*): `slots` holds voxel_hash_slots(max_n) 64-byte slots, all free between
// scans (launch_voxel_hash_clear once; every emit leaves the slots it used free again)
struct VoxelHashBuffers {
  void* slots;
  unsigned int *slot_of, *next;   // per input point
  unsigned long long* counts;     // per workgroup of 256 points: (run number << 32) | voxels owned by the workgroup
  unsigned int* crowded;          // one word: the longest member list behind a slot so far
  // part_world > 1: a job that shares the FUSED filter (insert inside the de-skew) by voxel - rank part_rank inserts the voxels
  // whose key hashes to it and emits at most voxel_partition_bound(n, part_world) of them (else *part_overflow = 1, mapped host memory)
  int part_world, part_rank;
  int* part_overflow;
};
size_t voxel_hash_slots(int max_n);
int voxel_partition_bound(int n, int world);
void launch_voxel_hash_clear(const VoxelHashBuffers& vh, size_t slots, hipStream_t s);
void launch_voxel_hash(const VoxelHashBuffers& vh, const float4* pts, int n, const unsigned int* mm, const unsigned int* bbox_rows,
                       int n_rows, float leaf, float4* out, int* n_out, int* filtered, unsigned int* pcl_out, int stages, unsigned int epoch,
                       hipStream_t s, int test_late = 0 /* LII_TEST=emit_late: see k_vhash_emit */,
                       // inten != nullptr: the emit also forms every voxel's intensity - the members' in input order from 0.f, divided by the
                       // count, PCL's centroid - at the voxel's place in inten_out (the identity pass-through copies)
                       const float* inten = nullptr, float* inten_out = nullptr);
// de-skew (k_deskew_imu / k_deskew_cv): where the scan comes from and goes to, what is known about it, what rides along
struct DeskewPlan {
  const float4* in;     // the scan as it arrived (a caller's device buffer, or == out)
  float4* out;          // the de-skewed scan
  int n;
  int sorted;           // ascending time order: no time extent needed
  const unsigned long long* extent;  // !sorted: the result of launch_time_extent
  unsigned int* bbox_rows;           // one bounding-box row per workgroup of 256 points is left here
  float leaf;                        // vh != nullptr: the leaf of the hashed voxel filter whose insert rides along
  const VoxelHashBuffers* vh;
  const void* ctrl_src;              // ctrl_bytes > 0: one extra workgroup copies this (pinned host memory) to ctrl_dst
  void* ctrl_dst;
  size_t ctrl_bytes;
#ifdef LII_GAP_TRACE
  unsigned long long* gap;  // measurement builds only (tools/ab_build.sh ... -DLII_GAP_TRACE): words 200 .. 202 of the granule buffer
#endif
};
void launch_deskew_imu(const DeskewPlan& p, const double* poses_host, const double* poses_dev, int K, const UndistArgH& u, hipStream_t s);
// THE PRE-ARMED PROLOGUE (round 6).  The de-skew launch of the NEXT scan is enqueued while the current scan's passes still run, and waits
// on the device for a record the host writes once it knows what that launch needs - the propagated state and the IMU pose table, which
// depend on the current scan's result.  What the host then pays between two scans is a few stores, not a launch: the dependent chain
// result -> host -> first kernel of the next scan loses the runtime's launch path and the command processor's fetch + dispatch
// (profiles/r06_chain.md).
// The record: {K, UndistArgH, K x 22 doubles} in DEVICE memory, which the host writes directly (large BAR: posted writes, no round
// trip; a first form kept it in mapped host memory and had one workgroup fetch and re-publish it - three PCIe round trips and two
// cache-wide fences on the critical path, 10 us slower than the launch it replaced).  It is laid out in 64-byte lines of seven
// payload doubles and a TAG (seq << 2 | kGateGo); the host writes the payload, then the tags, line 0's tag last, a store fence between
// the three - so a workgroup that sees line 0's tag finds every line complete, and a line it finds with another tag is a stale cached
// copy (the record lives in a ring of kGateRing slots), fetched again past the caches.
// The state word (GateState::word, mapped HOST memory) is seq << 2 | state; the host arms it before it enqueues the launch, and exactly
// one side moves it on, by compare-and-swap: the host to GO (then it writes the record) or CANCEL (this scan is not the one that was
// announced, or another entry point needs the stream), the launch itself to EXPIRED when nobody came for `timeout_ticks` (100 MHz) -
// it then ends having touched nothing, so a forgotten launch can delay the stream by that long, never hang it.
constexpr unsigned long long kGateArmed = 0ull, kGateGo = 1ull, kGateCancel = 2ull, kGateExpired = 3ull;
constexpr int kGateMaxPoses = 29;                                   // pose tables the pre-armed form takes (longer ones: the plain launch)
constexpr int kGateLines = (25 + 22 * kGateMaxPoses + 6) / 7;       // 64-byte lines of a record (95)
constexpr int kGateRing = 64;                                       // record slots (seq % kGateRing)
struct GateState { unsigned long long word; };                      // pinned, device-mapped host memory: seq << 2 | kGate*
struct DeskewGate {
  GateState* host;                  // the state word (polled by the gate workgroup alone; one compare-and-swap over PCIe if it gives up)
  const double* rec;                // this launch's record slot in device memory (kGateLines x 8 doubles)
  unsigned long long* dev_flag;     // seq << 2 | kGateCancel when the launch is to end without running (published by the gate workgroup)
  unsigned long long seq;
  long long timeout_ticks;
  int late_load;                    // 1: the scan itself may still be on its way when the launch starts (lii_scan_upload_next): no point is read before the record is there
};
void launch_deskew_imu_gated(const DeskewPlan& p, const DeskewGate& gate, hipStream_t s);
void launch_deskew_cv(const DeskewPlan& p, const CvArgH& a, hipStream_t s);
// The CV de-skew that propagates as well (k_deskew_cv_prop; lii_scan_register_cv): the scan's workgroups plus one, which runs
// k_cv_propagate's arithmetic on the state in pinned host memory (st_in), writes the propagated state to st_out (612 doubles) /
// prop_out (36) / host_out (612, optional, mapped host memory) and pulls the 16-byte words [ctrl_from, p.ctrl_bytes / 16) of the
// control block.  rot / bias_g / vel: rot_end, bias_g, vel_end of the UNPROPAGATED state, for the scan workgroups.
struct CvFuseH {
  double rot[9], bias_g[3], vel[3];
  double dt;
  double cov_gyr_scale[3], cov_acc_scale[3];
  const double* st_in;
  double* st_out;
  double* prop_out;
  double* host_out;
  int ctrl_from;
};
void launch_deskew_cv_prop(const DeskewPlan& p, const CvFuseH& f, hipStream_t s);
// The de-skew behind k_imu_propagate (lii_imu.hip): end pose + extrinsic (the first 24 doubles of the propagated state: IekfCtrl::st),
// the number of poses and the table itself are read from DEVICE memory - none of them has visited the host.
void launch_deskew_imu_dev(const DeskewPlan& p, const double* pose24_dev, const int* n_poses_dev, const double* poses_dev, hipStream_t s);
// IMU forward propagation (lii_imu.hip).  The carry of ImuProcess between two scans: last_imu_ (t, gyr, acc), acc_s_last, angvel_last,
// last_lidar_end_time_, one spare word - 15 + 1 doubles, in one buffer and out another (both workgroups of the launch read the old one).
constexpr int kImuCarryDoubles = 16;
struct ImuPropArgs {
  const double* st_in;      // lii_state as the previous update left it (pinned host memory, or device memory)
  const double* samples;    // n_imu x (t, gyr[3], acc[3]) (pinned host memory, or device memory)
  int n_imu;                // 1 .. 63
  double noise[19];         // cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc, cov_R_LI, cov_T_LI, mean_acc_norm (lii_imu_noise)
  double pcl_beg_time, pcl_end_time;
  const float4* scan;       // != nullptr: pcl_end_time = pcl_beg_time + (the scan's last time stamp) / 1000 instead of the argument
  int n_scan, sorted;       // sorted: the last point carries it; else extent[1] (k_time_extent)
  const unsigned long long* extent;
  const double* carry_in;
  double* carry_out;
  double* poses;            // IMUpose table, lii_pose6d records
  int* n_poses;
  double* st_out;           // the propagated lii_state (612 doubles)
  double* prop_out;         // optional: its first 36 doubles once more (IekfCtrl::prop)
  double* host_out;         // optional, mapped host memory: state (612) | carry (15) | number of poses
  const uint4* ctrl_src;    // ctrl_vec > 0: 16-byte words [ctrl_from, ctrl_vec) of the update's control block are pulled along
  uint4* ctrl_dst;
  int ctrl_from, ctrl_vec;
};
struct CvPropArgs {
  const double* st_in;
  double dt;
  double cov_gyr_scale[3], cov_acc_scale[3];
  double* st_out;
  double* host_out;         // optional, mapped host memory
};
void launch_imu_propagate(const ImuPropArgs& a, hipStream_t s);
void launch_cv_propagate(const CvPropArgs& a, hipStream_t s);
// calibration (lii_li_init_dev.hip)
void launch_calib_eval(int stage, const double* imu, const double* lidar, int n, const double* params, double* out,
                       hipStream_t s);

// device-side map maintenance (lii_map.hip)
void launch_map_decide_compact(const RegistrationBuffers& rb, const PoseArg& ps, double fsd, int have_search, unsigned long long* blk_counts, unsigned int epoch,
                               float4* world, float4* dst_add, float4* dst_nodown, int* counts, int bound_add, int bound_nodown, hipStream_t s,
                               const IekfCtrl* guard = nullptr, int seq = 0, int test_late = 0,
                               // (hkey != nullptr: the hash insert of the fold that follows rides in this launch - table sized by bound_add)
                               unsigned long long* hkey = nullptr, unsigned long long* hbest = nullptr, unsigned int* slot_of = nullptr, float ds = 0.f,
                               unsigned int* ins_flag = nullptr, int* events = nullptr,
                               const float* inten = nullptr /* != nullptr: the lists' records take their fourth word from inten[i] (k_map_decide<true>) */);  // blk_counts: one word per 256 points; epoch: the number of this run (never 0); guard: see k_map_decide
void launch_map_publish(const int* ctr, int n_words, int* host, int seq_at, int seq, hipStream_t s);
void launch_add_keys(const float4* pts, int n, const int* n_dev, float ds, unsigned long long* keys, unsigned int* idx, int* events, hipStream_t s);
void launch_add_fold(const float4* add_pts, const unsigned long long* keys, const unsigned int* idx, int n, float ds, const GridView& g,
                     unsigned char* tomb, float4* ins_pts, unsigned int* ins_flag, unsigned int* events, unsigned int* tp, unsigned int* work,
                     int* ctr, unsigned int work_cap, hipStream_t s, bool carry_w = false);  // carry_w: ins_pts keeps the batch points' fourth word
size_t add_hash_slots(int max_n);
// the cells of the inserts found / created inside the fold launch (k_add_fold8<true, true>) instead of by launch_ins_cells behind it
struct FoldCellsH {
  BlockEntry* blocks; unsigned int mask; unsigned int tables_cap; unsigned int* ins_e; float4* dropped; unsigned int drop_cap; unsigned long long* key_of_id;
  const float4* list2; int n2; const int* n2_dev; unsigned int* ins_e2;
};
void launch_add_fold_hashed(const float4* add_pts, int n, const int* n_dev, float ds, const GridView& g, unsigned long long* hkey,
                            unsigned long long* hbest, unsigned int* slot_of, unsigned char* tomb, float4* ins_pts, unsigned int* ins_flag,
                            unsigned int* events, unsigned int* tp, unsigned int* work, int* ctr, unsigned int work_cap, hipStream_t s,
                            bool inserted = false, const FoldCellsH* cells = nullptr, bool carry_w = false);  // carry_w: the leader keeps its fourth word
// in-place map update (lii_map.hip)
void launch_ins_cells(const float4* list, const unsigned int* flags, int n, const int* n_dev, const float4* list2, int n2, const int* n2_dev, unsigned int* ins_e2,
                      BlockEntry* blocks, unsigned int mask, float inv_cs, unsigned int tables_cap, unsigned int* ins_e, unsigned int* tp,
                      unsigned int* work, int* ctr, unsigned int work_cap, float4* dropped, unsigned int drop_cap, unsigned long long* key_of_id, hipStream_t s,
                      bool carry_w = false);  // carry_w: a parked insert keeps its fourth word
// the history of what box deletes remove (lii_map_removed_*): the squeeze of a box delete appends the points it drops.  `reserved` counts the
// records asked for since the last clear - it runs past `cap` when the buffer is full: min(reserved, cap) records are held, the rest was not stored.
struct RemovedSink {
  float4* buf;                   // cap records (nullptr: nothing is collected - the launches take the forms they have without the order)
  unsigned long long* reserved;
  unsigned int cap;
};
// removed != nullptr with a buffer: the launch serves a box delete and collects (every tombstone is a box tombstone); the fold's updates pass none
void launch_cell_apply(const unsigned int* work, uint2* cells, unsigned int* cell_cap, float4* pts, unsigned char* tomb, unsigned int* tp, int* ctr,
                       unsigned int pts_cap, int launch_bound, const WinKeep& wk, hipStream_t s, const RemovedSink* removed = nullptr);
void launch_ins_write(const float4* list, const unsigned int* ins_e, int n, const int* n_dev, const float4* list2, const unsigned int* ins_e2, int n2, const int* n2_dev,
                      uint2* cells, const unsigned int* cell_cap, float4* pts, int* ctr, float4* dropped, unsigned int drop_cap, hipStream_t s,
                      int* host, int n_words, int seq_at, int seq, const WinKeep& wk)  /* host != nullptr: the last workgroup publishes the counters there */;
void launch_cell_caps(const uint2* cells, int n_entries, unsigned int* caps, hipStream_t s);
void launch_spread(const float4* src, uint2* cells, unsigned int* cell_cap, const unsigned int* caps, const unsigned int* capsum, int n_entries,
                   float4* dst, int* ctr, int n_valid, int n_blocks, hipStream_t s);
void launch_cell_counts(const uint2* cells, int n_entries, unsigned int* cnt, hipStream_t s);
void launch_gather_live(const float4* pts, const uint2* cells, const unsigned int* cntsum, int n_entries, float4* dst, int dst_cap, hipStream_t s);
void launch_box_tomb_cells(const float4* pts, const uint2* cells, int n_entries, const float* boxes, int n_boxes, unsigned char* tomb, unsigned int* tp,
                           unsigned int* work, int* ctr, unsigned int work_cap, hipStream_t s);
// edits and queries by point and box (lii_map.hip: k_point_tomb, k_map_range -> k_map_range_finish, k_box_gather).  list_dev: float xyz every
// stride_bytes in device memory; tomb: 4-byte aligned and padded to a multiple of 4 bytes (the claim is a 32-bit atomic).  partial: 256 x 6
// words of scratch; range6 / n_hits: device memory.  The last two launch a fixed grid.
void launch_point_tomb(const GridView& g, const void* list_dev, int n, int stride_bytes, unsigned char* tomb, unsigned int* tp, unsigned int* work, int* ctr,
                       unsigned int work_cap, hipStream_t s);
void launch_map_range(const float4* pts, const uint2* cells, int n_entries, unsigned int* partial, float* range6, hipStream_t s);
void launch_box_gather(const float4* pts, const uint2* cells, const unsigned long long* key_of_id, int n_blocks, float cs, const float* boxes, int n_boxes,
                       float4* out, unsigned int capacity, unsigned long long* n_hits, hipStream_t s);
// the moving local-map cube (lii_map.hip: k_local_map_tomb -> k_cell_apply_listed -> k_local_map_finish; the arithmetic: lii_fov.h).  `in` / `out`:
// the two copies of the state in device memory; pos_dev != nullptr: state.pos_end is read there, else `pos` travels by value; `host`: the
// pinned copy of the state the last launch leaves.  All three launches have a fixed size.
constexpr int kLocalMapGrid = 512;
void launch_local_map_tomb(const LocalMapState* in, LocalMapState* out, const LocalMapParams& P, const double* pos_dev, const double* pos, const float4* pts,
                           const uint2* cells, const unsigned long long* key_of_id, int n_blocks, float cs, unsigned char* tomb, unsigned int* tp,
                           unsigned int* work, int* ctr, unsigned int work_cap, hipStream_t s);
void launch_cell_apply_listed(const unsigned int* work, uint2* cells, unsigned int* cell_cap, float4* pts, unsigned char* tomb, unsigned int* tp, int* ctr,
                              unsigned int pts_cap, unsigned int work_cap, const WinKeep& wk, hipStream_t s, const RemovedSink* removed = nullptr);
void launch_local_map_finish(LocalMapState* st, int* ctr, LocalMapState* host, int seq, hipStream_t s);

// the registered clouds of a scan (lii_publish.hip: k_publish_world)
struct PublishArgs {
  const float4* scan;       // the de-skewed scan (dense_blocks workgroups of 256 points)
  int n_scan, dense_blocks;
  float4* dense;            // LII_PUB_DENSE (nullptr: not ordered)
  // LII_PUB_INTENSITY (every pointer nullptr: today's launch).  scan_int: the scan's intensities (nullptr: it has none - the save buffer
  // then gets 0.0f), dense_int: -> the dense cloud's, save_int: -> the save buffer's at the cloud's offset, by the workgroups that own it;
  // body_int -> down_int: the down-sampled cloud's, by the workgroups of that cloud
  const float* scan_int;
  float* dense_int;
  float* save_int;
  const float* body_int;
  float* down_int;
  float4* save;             // the save buffer (nullptr: none), save_cap points,
  int save_cap, save_par;
  int* save_ctl;            // ... [save_par]: its append offset as this launch finds it, [save_par ^ 1]: as it leaves it, [2]: sticky "a scan did not fit"
  const float4* body;       // the down-sampled cloud: at most n_body points, *n_body_dev of them if != nullptr
  int n_body;
  const int* n_body_dev;
  float4* down;             // LII_PUB_DOWN (nullptr: not ordered)
  const unsigned char* selected;
  float4* effect;           // LII_PUB_EFFECT (nullptr: not ordered)
  unsigned long long* words;  // one word per workgroup of the down-sampled cloud (prefix_below)
  unsigned int epoch;         // the number of this launch (never 0)
  int* counts_dev;          // [0] points of the down-sampled cloud, [1] of the effect cloud: device memory ...
  int* counts_host;         // ... and mapped host memory
  const IekfCtrl* guard;    // != nullptr: pose from the control block, and nothing is done unless update `seq` has stopped
  int seq;
  int test_late;            // LII_TEST=emit_late: every seventh workgroup of the down-sampled cloud publishes its word late (as k_vhash_emit / k_map_decide)
  // lii_publish_wire_set (every pointer nullptr: the launch without it).  The clouds as 48-byte pcl::PointXYZINormal records, three
  // uint4 each (kWireQuads): w_dense / w_body by the workgroups of the scan, w_down / w_effect by those of the down-sampled cloud.
  // Intensities of their own, because this order hands them on whether or not the other asks for LII_PUB_INTENSITY: w_scan_int the
  // scan's, w_body_int the down-sampled cloud's (nullptr: none - the records get +0.0f).
  uint4* w_dense;
  uint4* w_body;
  uint4* w_down;
  uint4* w_effect;
  const float* w_scan_int;
  const float* w_body_int;
  // lii_point_noise_set, model 1: the intensity of the EFFECT records, per point of the down-sampled cloud (RegistrationBuffers::sqrt_rinv);
  // nullptr: the constant (float)sqrt(1000)
  const float* w_effect_int;
};
constexpr int kWireQuads = 3;       // a record: 48 bytes = 3 x 16
constexpr int kPcdChunkRows = 65536;  // lii_publish_saved_pcd's staging area (the chunk of lii_map_delete_points)
void launch_publish_world(const PublishArgs& a, int down_blocks, const PoseArg& ps, hipStream_t s);
// the save buffer as binary PCD rows (8 floats: x y z 0 0 0 intensity 0): rows [first, first + n) -> out[0, n); inten == nullptr: 0.0f
void launch_pcd_rows(const float4* save, const float* inten, int first, int n, uint4* out, hipStream_t s);
// ... and map points as such rows (lii_map_pcd): the intensity is the point's own fourth word
void launch_pcd_rows_w(const float4* pts, int first, int n, uint4* out, hipStream_t s);

// rocPRIM wrappers (lii_sort.hip)
size_t sort_temp_bytes(int max_n);
void sort_pairs_u64(void* temp, size_t temp_bytes, const unsigned long long* kin, unsigned long long* kout,
                    const unsigned int* vin, unsigned int* vout, int n, hipStream_t s);
// back half of the voxel-grid filter (lii_vsort.hip): sample sort of the (key, index) pairs + centroids
struct VoxelSortBuffers {
  const unsigned long long* keys_in;   // kVoxKeyBits-wide sort keys (lii_device.h)
  unsigned long long* keys_out;
  unsigned int* idx_out;
  unsigned long long* comp;       // n composites, bucket order
  unsigned long long* splitters;  // 2048
  const unsigned long long* samples;  // 4096, written by k_voxel_keys (voxel_sort_plan)
  unsigned int* hist;             // voxel_sort_hist_elems(max n), zero-initialised once
  unsigned short* bucket_of;      // n
  const unsigned int* pcl_in;     // PCL voxel index of every input point ...
  unsigned int* pcl_out;          // ... and of every output voxel (the order the reference's filter would emit them in)
  unsigned int* max_run;          // optional: receives (atomicMax) the largest number of points of one voxel when it exceeds 8
};
size_t voxel_sort_hist_elems(int max_n);
struct VoxelSortPlan { int buckets, samples, width, strata; };
VoxelSortPlan voxel_sort_plan(int n);
// sort + one centroid per voxel: out[0 .. *n_out) in key order, *n_out (device) = number of occupied voxels
// (inten != nullptr: the intensity of every voxel as well, summed like the four floats of the point)
void launch_voxel_sort_centroids(const VoxelSortBuffers& vb, const float4* pts, int n, float4* out, int* n_out, hipStream_t s,
                                 const float* inten = nullptr, float* inten_out = nullptr);
void sort_pairs_u32(void* temp, size_t temp_bytes, const unsigned int* kin, unsigned int* kout, const unsigned int* vin,
                    unsigned int* vout, int n, hipStream_t s);
void inclusive_scan_u32(void* temp, size_t temp_bytes, const unsigned int* in, unsigned int* out, int n, hipStream_t s);

float ord_to_float(unsigned int o);

}  // namespace lii

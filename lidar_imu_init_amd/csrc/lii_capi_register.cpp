// libliinit_hip — the registration loop (host side): lii_iekf_iterate / lii_iekf_update / lii_scan_register and the neighbour
// download.  Kernels: lii_knn.hip (k-NN), lii_fit.hip (fit + reduce), lii_iekf.hip (final sum + 24-state solve), lii_scan.hip (prologue of
// lii_scan_register).  Reference: src/laserMapping.cpp:909-1134.
#include "lii_context.h"
#include <cstddef>

#include "lii_hostmath.h"

using namespace lii_impl;

namespace {

// (every enqueued search launch has a number, which the fit launch behind it shares: the list of unfinished queries the one leaves
// and the other consumes - RegistrationBuffers::flag_*)
int next_knn_epoch(lii_handle h) {
  h->knn_epoch = h->knn_epoch >= 0x3FFFFFFE ? 1 : h->knn_epoch + 1;  // (consecutive numbers alternate between the two slots, across the wrap as well)
  return h->knn_epoch;
}
void launch_knn(lii_handle h, const GridView& g, const RegistrationBuffers& rb, const PoseArg* pose, int forced, int epoch,
                hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
  lii::launch_knn(g, rb, pose, h->d_ctrl, forced, h->d_ctrl->search_pose, h->stream, epoch, ev_start, ev_stop);
}

// lii_point_noise_set, model 1: a fit launch has been enqueued - lii_point_noise_download has something to serve
void note_noise_pass(lii_handle h) { if (h->noise.model == 1) h->noise.have_pass = true; }

int iterate(lii_handle h, const lii_state* st, bool search, bool imu_en, double* out91) {
  if (h->n_body <= 0) return fail(h, LII_ERR_STATE, "no down-sampled scan (call lii_downsample / lii_downsample_skip)");
  int rc = commit_map(h);
  if (rc != LII_OK) return rc;
  if (!search && !h->have_search) return fail(h, LII_ERR_STATE, "non-search iteration before any search");
  GridView g = grid_view(h);
  RegistrationBuffers rb = reg_buffers(h);
  const bool prof = h->prof.profiling;
  if (prof) HIPCHK(h, hipEventRecord(h->prof.ev[0], h->stream));
  // the pose of a host-driven pass travels to the handle's pose slot first: the kernels read it from device memory on every path
  {
    PoseArg* stage = &h->h_small->pose;  // (pinned, a member of its own; this call ends with a synchronisation)
    *stage = pose_of(*st);
    HIPCHK(h, hipMemcpyAsync(h->d_pose, stage, sizeof(PoseArg), hipMemcpyHostToDevice, h->stream));
  }
  if (search) h->unfinished_known = false;  // (a search pass of this host-driven call: lii_last_unfinished_queries reads the device again)
  const int epoch = search ? next_knn_epoch(h) : 0;
  if (search) launch_knn(h, g, rb, h->d_pose, 1, epoch);
  if (prof) HIPCHK(h, hipEventRecord(h->prof.ev[3], h->stream));
  launch_fit_reduce(g, rb, h->d_pose, h->d_ctrl, search ? 1 : 0, imu_en ? 1 : 0, h->cfg.plane_threshold,
                    h->cfg.laser_point_cov_inv, h->stream, epoch);
  note_noise_pass(h);
  if (prof) HIPCHK(h, hipEventRecord(h->prof.ev[1], h->stream));
  launch_reduce91(rb, h->d_out91, h->d_ctrl, 1, h->stream, epoch);
  if (prof) HIPCHK(h, hipEventRecord(h->prof.ev[2], h->stream));
  if (search) h->have_search = true;
  if (h->net.comm) {
    ncclResult_t r = ncclAllReduce(h->d_out91, h->d_out91, kNormalEq, ncclDouble, ncclSum, h->net.comm, h->stream);
    if (r != ncclSuccess) return fail(h, LII_ERR_COMM, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  } else if (h->net.mailbox.dev_slots) {
    launch_mailbox_allreduce(h->d_out91, mailbox_view(h), h->stream);
  }
  HIPCHK(h, hipMemcpyAsync(h->h_small->normal_eq, h->d_out91, sizeof(double) * kNormalEq, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::memcpy(out91, h->h_small->normal_eq, sizeof(double) * kNormalEq);
  if (h->net.mailbox.dev_slots && out91[kNormalEq - 1] != out91[kNormalEq - 1])
    return fail(h, LII_ERR_COMM, "mailbox exchange timed out (a rank of the job did not reach this pass)");
  if (prof) {
    // timings: [0] sum ms search-pass kernel, [1] sum ms residual-pass kernel, [2] sum ms reduce kernel,
    //          [3] host solve ms (last update), [4] total ms (last update), [5]/[6] launch counts of [0]/[1]
    float a = 0, b = 0;
    HIPCHK(h, hipEventElapsedTime(&a, h->prof.ev[0], h->prof.ev[1]));
    HIPCHK(h, hipEventElapsedTime(&b, h->prof.ev[1], h->prof.ev[2]));
    if (search) {
      float k = 0;
      HIPCHK(h, hipEventElapsedTime(&k, h->prof.ev[0], h->prof.ev[3]));
      h->prof.timings[0] += a; h->prof.timings[5] += 1; h->prof.timings[7] += k;  // [7]: the k-NN kernel alone
    } else { h->prof.timings[1] += a; h->prof.timings[6] += 1; }
    h->prof.timings[2] += b;
  }
  return LII_OK;
}

// The whole iterated update enqueued once: prologue (P^-1), then max_iterations x {k-NN, fallback, fit+reduce,
// final reduce, 24-state solve}; every kernel consults the device-resident control block and returns at once when
// its pass is not due (no search scheduled / loop already stopped).  One synchronisation at the end.
void fill_ctrl(lii_handle h, const lii_state* state, const lii_state* state_prop, const lii_iekf_opts* opts) {
  IekfCtrl* hc = h->h_ctrl;
  std::memcpy(hc->st, state, sizeof(lii_state));
  std::memcpy(hc->prop, state_prop, sizeof(hc->prop));
  hc->max_it = opts->max_iterations;
  hc->imu_en = opts->imu_en;
  hc->it = 0; hc->search_next = 1; hc->stop = 0; hc->rematch_num = 0; hc->converged = 0; hc->searches = 0;
  hc->effect_num = 0; hc->singular = 0;
  h->update_seq = h->update_seq == 0x7FFFFFFF ? 1 : h->update_seq + 1;
  hc->seq = h->update_seq;
  // which k-NN launches ride along (IekfCtrl::plan_mask): the first pass always; the others as the previous update needed them
  // (the mask holds 16 passes: a longer loop is enqueued whole - the device takes every pass from 16 on for enqueued, which a
  // plan that ends earlier would not honour - ADVICE r4)
  unsigned int plan = 0xFFFFFFFFu;
  if (h->knn_plan && !h->net.comm && opts->max_iterations <= 16) {
    plan = (h->knn_plan_force >= 0 ? ((unsigned int)h->knn_plan_force | 0xFFFF0000u) : h->plan_next) | 0x00010001u;
  }
  hc->plan_mask = plan;
  h->plan_cur = plan;
}

// ------------------------------------------------------------------------------------------------ the job
// lii_scan_job as the call uses it, read once: a field the caller's ABI does not have reads as zero / null.
// struct_size 88: ABI 9; 72: ABI 8, without while_waiting; 56: ABI 6 - 7, without next_scan_dev; 48: ABI 5, without scan_sorted / map_update.
static_assert(sizeof(lii_scan_job) == 88, "lii_scan_job: the sizes of the earlier ABIs are accepted by number");
constexpr uint32_t kJobAbi5 = 48u, kJobAbi6 = 56u, kJobAbi8 = 72u, kJobAbi9 = 88u;
struct JobView {
  bool sorted;      // ascending time order, as it arrived or (sort_first) once scan_sort_into has run
  bool sort_first;  // scan_sorted == 2: the scan is put into ascending time order on the device first, and the call goes on as for a
                    // scan_sorted == 1 job on the handle's own scan buffer
  bool map_update;
  float leaf;       // 0 when not positive
  int undistort;
  const lii_pose6d* poses; int n_poses;
  const void* scan_dev; int n_scan_dev;
  const void* next_scan_dev; int next_n_scan;
  void (*while_waiting)(void*); void* while_waiting_arg;
};
bool job_size_ok(uint32_t size) { return size == kJobAbi9 || size == kJobAbi8 || size == kJobAbi6 || size == kJobAbi5; }
JobView job_view(const lii_scan_job* job) {
  const uint32_t size = job->struct_size;
  JobView jv = {};
  jv.sort_first = size >= kJobAbi6 && job->scan_sorted == 2;
  jv.sorted = size >= kJobAbi6 && (job->scan_sorted == 1 || jv.sort_first);
  jv.map_update = size >= kJobAbi6 && job->map_update == 1;
  jv.leaf = job->leaf > 0 ? job->leaf : 0.f;
  jv.undistort = job->undistort;
  jv.poses = job->imu_poses; jv.n_poses = job->n_imu_poses;
  jv.scan_dev = job->scan_dev; jv.n_scan_dev = job->n_scan_dev;
  if (size >= kJobAbi8) { jv.next_scan_dev = job->next_scan_dev; jv.next_n_scan = job->next_n_scan; }
  if (size >= kJobAbi9) { jv.while_waiting = job->while_waiting; jv.while_waiting_arg = job->while_waiting_arg; }
  return jv;
}

// The pre-armed prologue (lii_launch.h: DeskewGate; prearm_arm / prearm_go / prearm_cancel: lii_capi.cpp): what this job announces for
// the next call - update_on_device arms it behind the passes.  may_announce: a plain lii_scan_register that neither sorts nor runs the
// local map; every other form announces nothing - next_scan_dev is ignored.
void prearm_wanted(lii_handle h, const JobView& jv, bool may_announce, bool from_job) {
  h->pre.want_dev = nullptr;
  if (!may_announce || !h->pre.enabled || !jv.sorted || jv.undistort != 1) return;
  if (jv.next_scan_dev && jv.next_n_scan > 0 && jv.next_n_scan <= h->cfg.max_scan_points) {
    h->pre.want_dev = jv.next_scan_dev; h->pre.want_n = jv.next_n_scan; h->pre.want_leaf = jv.leaf; h->pre.want_late = false;
  } else if (h->n_scan_next > 0 && h->d_scan_next && !from_job) {
    // a scan is on its way through lii_scan_upload_next: it is the next call's (after lii_scan_advance), de-skewed where it lands
    h->pre.want_dev = h->d_scan_next; h->pre.want_n = h->n_scan_next; h->pre.want_leaf = jv.leaf; h->pre.want_late = true;
  }
}

// ------------------------------------------------------------------------------------------------ the update on the device
// lii_scan_job::while_waiting (ABI 9), once per call that got as far as its update.  inside: from update_on_device - everything is
// enqueued, the thread would only wait now, the caller's hook runs first (entry points that change which frames are current refuse
// meanwhile: in_wait_hook); an arrangement without that wait (LII_TEST=host_solve) calls it behind the update, never otherwise.
void run_wait_hook(lii_handle h, bool inside) {
  if (!h->wait_hook) return;
  void (*hook)(void*) = h->wait_hook;
  h->wait_hook = nullptr;
  if (inside) h->in_wait_hook = true;
  hook(h->wait_hook_arg);
  if (inside) h->in_wait_hook = false;
}

// The passes of one update on the stream: what enqueueing one, waiting for the result and continuing a parked loop share.
struct DevicePasses {
  lii_handle h; const lii_iekf_opts* opts; hipStream_t s;
  GridView g; RegistrationBuffers rb;
  const PoseArg* pose;  // first 24 doubles of IekfCtrl::st
  // (profiling = HIP events around the k-NN launches only - the dominant kernel, lii_last_timings [5] / [7]; every event is a
  // barrier packet on the stream, so the rest of the loop is left alone: launch plan and result polling work as always)
  bool prof;
  unsigned int plan;  // fill_ctrl chose it (the control block on the device carries the same mask)

  int enqueue(int it) {
    const bool knn = it >= 16 || ((plan >> it) & 1u);
    // (a fit launch that is not behind a search launch never runs as a search pass - the plan parks the loop instead - and needs no number)
    const int epoch = knn ? next_knn_epoch(h) : 0;
    if (knn) {
      // (the k-NN launches of a profiled update carry their two events IN the dispatch: the kernel's own start and end stamps.  Rounds
      // 1 - 5 recorded an event in front of and behind the launch - two barrier packets each, + 22 us on a profiled scan, and the
      // bracket held the dispatch as well as the kernel)
      if (h->prof.kp_active) { const int r = kp_mark(h, LII_KP_KNN, it); if (r != LII_OK) return r; }
      if (prof && it < 16) launch_knn(h, g, rb, pose, -1, epoch, h->prof.ev_it[2 * it], h->prof.ev_it[2 * it + 1]);
      else launch_knn(h, g, rb, pose, -1, epoch);
    }
    if (h->prof.kp_active) { const int r = kp_mark(h, LII_KP_FIT, it); if (r != LII_OK) return r; }
    // the scan before left more unfinished queries per search pass than the fit launch's completion workgroups take: this one's
    // are finished by a launch of their own, one wavefront per listed query (k_complete_listed; nothing to do -> it returns at once)
    if (knn && h->wide_listed && !h->net.comm && h->net.n_ranks <= 1) launch_complete_listed(g, rb, h->d_ctrl, -1, s, epoch);
    launch_fit_reduce(g, rb, pose, h->d_ctrl, -1, opts->imu_en ? 1 : 0, h->cfg.plane_threshold, h->cfg.laser_point_cov_inv, s, epoch);
    note_noise_pass(h);
    if (h->prof.kp_active) { const int r = kp_mark(h, LII_KP_SOLVE, it); if (r != LII_OK) return r; }
    if (!h->net.comm) {  // single GPU or node-local mailbox: final sum (+ exchange) and solve in one launch
      launch_reduce_solve(rb, h->d_gran, h->d_ctrl, h->h_res, mailbox_view(h), s, epoch);
      return LII_OK;
    }
    launch_reduce91(rb, h->d_out91, h->d_ctrl, -1, s, epoch);
    // every rank enqueues the same number of all-reduces; a pass that is skipped on the device re-sums the
    // unchanged local buffer on all ranks alike, so the ranks stay in lock-step without a host decision
    ncclResult_t r = ncclAllReduce(h->d_out91, h->d_out91 + 128, kNormalEq, ncclDouble, ncclSum, h->net.comm, s);
    if (r != ncclSuccess) return fail(h, LII_ERR_COMM, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    launch_iekf_solve(h->d_ctrl, h->d_out91 + 128, h->h_res, s);
    return LII_OK;
  }

  // The iteration that stops the loop writes the result block (mapped host memory) and then its sequence number.  Polling
  // that word instead of synchronising the stream returns as soon as the result exists: the passes enqueued behind the
  // stopping one (they only read `stop` and return) drain while the caller already prepares the next scan.
  // The plan also ends the enqueued loop after as many passes as the last updates ran: the launches behind the stopping pass
  // only drain (3 x 4.5 us on stream100k, about what the host needs to come back with the next scan: + 0 .. 3 % scans/s,
  // gpurun_out/r3x4).  A loop that parked itself (the next pass is not there, or needs a search the plan did not hold - the
  // pattern changed against the previous scans) is continued by continue_parked: one host round trip, on those scans.
  int wait() {
    const int parked_word = h->update_seq | kLoopParked;
    if (h->poll_result && !h->net.comm) {
      volatile int* done = &h->h_res->done;
      unsigned int spins = 0;
      while (*done != h->update_seq && *done != parked_word) {
        if ((++spins & 0x3FFF) == 0) {  // every ~50 us: is the stream still alive?
          const hipError_t q = hipStreamQuery(s);
          if (q == hipSuccess) break;  // everything ran; `done` is final (a loop that never stopped is reported by result_code)
          if (q != hipErrorNotReady) return fail(h, LII_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
        }
        __builtin_ia32_pause();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      if (*done != h->update_seq && *done != parked_word) HIPCHK(h, hipStreamSynchronize(s));
    } else {
      HIPCHK(h, hipStreamSynchronize(s));  // the stopping iteration's solve has written h_res (mapped host memory)
    }
    return LII_OK;
  }

  // A parked loop is continued with what it is known to need: the pass it parked in front of - behind a k-NN launch if that pass
  // searches - and as many passes behind it as the longer of the last two updates ran; should that not be enough (the next search
  // comes at another pass as well, or the update runs longer) it parks again and is continued again.  (Round 3 enqueued every
  // remaining pass with every k-NN launch: up to nine launches that only read a flag, ~ 20 us on a scan that parks.)
  int continue_parked(bool* parked_once) {
    for (int round = 0; h->h_res->done == (h->update_seq | kLoopParked); round++) {
      if (round > 2 * opts->max_iterations) return fail(h, LII_ERR_HIP, "device loop parked again and again");
      *parked_once = true;
      const int from = h->h_res->parked_it;
      const bool search = h->h_res->parked_search != 0;
      h->plan_parked++;
      prearm_cancel(h);  // (the launches that continue the loop would queue up behind a launch that waits for this call to return)
      h->map_enqueued_early = false;  // (that launch saw a parked loop and did nothing: the caller makes the map update when the loop has ended)
      g = grid_view(h);  // (never a view older than the last thing that may have rebuilt the index: update_on_device, map_update_early)
      const int last = std::min(opts->max_iterations, std::max(h->plan_passes_prev, from + 1));  // (exclusive; from < max_iterations: the last pass never parks)
      unsigned int rplan = 0u;
      for (int q = from; q < last && q < 16; q++) rplan |= 1u << (16 + q);
      if (search && from < 16) rplan |= 1u << from;
      plan = rplan;
      h->h_res->done = 0;  // (the parked word of this round must not be taken for the next one's)
      std::atomic_thread_fence(std::memory_order_release);
      launch_loop_resume(h->d_ctrl, rplan, s);
      for (int it = from; it < last; it++) {
        const int rc = enqueue(it);
        if (rc != LII_OK) return rc;
      }
      if (h->prof.kp_active) { const int rc = kp_mark(h, LII_KP_KINDS); if (rc != LII_OK) return rc; }
      const int rc = wait();
      if (rc != LII_OK) return rc;
    }
    return LII_OK;
  }
};

#ifdef LII_SOLVE_TRACE
void solve_trace(const IekfResult* hr) {
  static int cnt = 0;
  if (++cnt % 100 != 0) return;
  auto row = [&](const long long* t) {
    fprintf(stderr, " loads+sums %lld | A %lld | elimination %lld (its own %lld) | solution %lld | state %lld (rotations %lld, pose stores %lld) | barrier + cov %lld | all %lld | clock %.2f GHz ;",
            t[1] - t[0], t[2] - t[1], t[4] - t[3], t[5] - t[3], t[8] - t[4], t[9] - t[8], t[7] - t[8], t[9] - t[7], t[10] - t[9], t[10] - t[0],
            t[5] > t[3] ? (double)(t[12] - t[11]) / (10.0 * (double)(t[5] - t[3])) : 0.0);
  };
  fprintf(stderr, "[solve trace, 10 ns ticks] stopping pass:");
  row(hr->ts);
  fprintf(stderr, "  pass 0:");
  row(hr->ts0);
  fprintf(stderr, "\n");
}
#endif

// (the launch plan of the completions, see DevicePasses::enqueue)
void note_unfinished(lii_handle h) {
  h->unfinished_known = !h->net.comm;
  if (h->net.comm || !h->wide_enabled) return;
  // (two scans in a row decide: a stream on which one scan in eight crosses the capacity - bench --edge - would pay for a launch that
  // finds nothing behind every such scan and never have it where it is needed)
  const bool wide = h->h_res->unfinished > lii::kFlagCap;
  if (wide == h->wide_prev && wide != h->wide_listed) { h->wide_listed = wide; h->wide_switches++; }
  h->wide_prev = wide;
  if (wide) h->wide_scans++;
}

// per-launch brackets (lii_set_profiling(h, 3)): the time from the event in front of a launch to the next event, for the
// launches that executed (a pass the loop did not reach, or a k-NN launch whose pass did not search, only read a flag)
int account_brackets(lii_handle h, const IekfResult* hr) {
  if (!(h->prof.kp_active && h->prof.kp_n > 1 && hr->it > 0)) return LII_OK;
  HIPCHK(h, hipEventSynchronize(h->prof.kp_ev[size_t(h->prof.kp_n - 1)]));
  for (int i = 0; i + 1 < h->prof.kp_n; i++) {
    int kind = h->prof.kp_kind[size_t(i)] / 64;
    const int it = h->prof.kp_kind[size_t(i)] % 64;
    if (kind >= LII_KP_KINDS) continue;
    const bool loop_kind = kind == LII_KP_KNN || kind == LII_KP_FIT || kind == LII_KP_SOLVE;
    if (loop_kind && (it >= hr->it || it >= 16)) continue;
    if (kind == LII_KP_KNN && !(hr->search_log[it] & 1)) continue;
    if (kind == LII_KP_FIT && (hr->search_log[it] & 1)) kind = LII_KP_FIT_SEARCH;
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->prof.kp_ev[size_t(i)], h->prof.kp_ev[size_t(i + 1)]) != hipSuccess) continue;
    h->prof.kprof.ms[kind] += ms;
    h->prof.kprof.launches[kind] += 1;
  }
  h->prof.kprof.scans += 1;
  return LII_OK;
}

// what the result block says about the update, as the call's return code
int result_code(lii_handle h, const IekfResult* hr) {
  if (hr->part_overflow) {
    h->h_res->part_overflow = 0;
    return fail(h, LII_ERR_CAPACITY, "voxel-partitioned job: this rank's share of the down-sampled cloud exceeds its bound (mean share + 25 % + 2048 points); use lii_comm_set_partition(h, 1)");
  }
  if (hr->singular == 3)
    return fail(h, LII_ERR_COMM, "mailbox exchange timed out (a rank of the job did not reach this pass); re-create the communicator");
  if (hr->singular == 4)
    return fail(h, LII_ERR_COMM, "the sums of a pass did not reach the solver within 2 s (a summing workgroup of the launch was not scheduled: is the device shared?)");
  if (hr->singular) return fail(h, LII_ERR_INVALID, "singular covariance / normal matrix in the device solve");
  if (hr->it < 0) return fail(h, LII_ERR_HIP, "device loop ended without a result");
  return LII_OK;
}

// the next update's plan: this one's pattern; passes it did not reach keep their launch
void plan_from_result(lii_handle h, const IekfResult* hr) {
  h->last_pivoted_passes = 0;
  for (int q = 0; q < 16 && q < hr->it; q++) h->last_pivoted_passes += (hr->search_log[q] >> 1) & 1;
  unsigned int next = 0xFFFFFFFFu;
  for (int q = 0; q < 16 && q < hr->it; q++)
    if (!(hr->search_log[q] & 1)) next &= ~(1u << q);
  // ... and as many passes as the longer of the last two updates ran (a scan that needs more parks and is continued)
  for (int q = std::max(hr->it, h->plan_passes_prev); q < 16; q++) next &= ~(1u << (16 + q));
  h->plan_passes_prev = hr->it;
  h->plan_next = next;
}

void fill_report(lii_iekf_report* report, int iterations, int searches, int effect_num, int converged, const double* normal_eq) {
  if (!report) return;
  report->iterations = iterations;
  report->searches = searches;
  report->effect_num = effect_num;
  report->converged = converged;
  std::memcpy(report->normal_eq, normal_eq, sizeof(double) * kNormalEq);
}

int update_on_device(lii_handle h, lii_state* state, const lii_state* state_prop, const lii_iekf_opts* opts,
                     lii_iekf_report* report) {
  static_assert(sizeof(lii_state) == sizeof(double) * kStateDoubles, "lii_state layout");
  if (h->n_body <= 0) return fail(h, LII_ERR_STATE, "no down-sampled scan (call lii_downsample / lii_downsample_skip)");
  const auto t_map0 = std::chrono::steady_clock::now();
  int rc = commit_map(h);
  if (rc != LII_OK) return rc;
  if (h->diag) h->prof.host_map_us[0] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_map0).count();
  hipStream_t s = h->stream;
  // The stream lii_map_incremental leaves its update on is created with the first update of a handle that is NOT a rank of a
  // sharded job (those never update beside a scan).  Not in lii_create: a second compute queue per process - even one whose
  // stream has been destroyed again: the runtime keeps the hardware queue - makes several processes on one device oversubscribe
  // the hardware queues, and a kernel that waits for a peer's kernel (the mailbox) then waits for a time slice: the one-device
  // rehearsal of a 2-rank job fell from 4 000 to 1 350 scans/s.
  if (!h->map_stream && h->net.n_ranks <= 1) HIPCHK(h, h->map_stream.create(hipStreamNonBlocking));
  if (!h->ctrl_preloaded) {
    if (h->staging_busy) HIPCHK(h, hipStreamSynchronize(s));  // a lii_scan_register that failed half way left the buffer in use
    fill_ctrl(h, state, state_prop, opts);
    HIPCHK(h, hipMemcpyAsync(h->d_ctrl, h->h_ctrl, sizeof(IekfCtrl), hipMemcpyHostToDevice, s));
  }
  h->ctrl_preloaded = false;
  h->h_res->singular = 0; h->h_res->it = -1;  // (it: overwritten by the stopping iteration)
  // lii_local_map_set(enabled): lasermap_fov_segment + the box delete at the reference's place - behind the propagation (state.pos_end of
  // the control block, which every prologue has put on the stream by now) and the map update that commit_map joined, in front of the
  // first search.  Three launches of fixed size.
  if (h->lm.in_job) {
    rc = local_map_enqueue(h, h->d_ctrl->st + 9, nullptr, h->prof.kp_active);
    if (rc != LII_OK) return rc;
  }
  const bool prof = h->prof.profiling && h->prof.prof_mode != 3;  // (mode 3 brackets every launch itself: kp_mark)
  DevicePasses p = {h, opts, s, grid_view(h), reg_buffers(h), reinterpret_cast<const PoseArg*>(h->d_ctrl), prof, h->plan_cur};
  if (prof) harvest_knn_events(h);  // (the events are about to be used again)
  const unsigned int plan0 = p.plan;
  const auto t_loop0 = std::chrono::steady_clock::now();
  for (int it = 0; it < opts->max_iterations; it++) {
    if (it < 16 && !((p.plan >> (16 + it)) & 1u)) break;  // the plan ends here
    rc = p.enqueue(it);
    if (rc != LII_OK) return rc;
  }
  if (h->diag) h->prof.host_loop_enq_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_loop0).count();
  if (h->prof.kp_active) { rc = kp_mark(h, LII_KP_KINDS); if (rc != LII_OK) return rc; }  // (end mark of the planned passes)
  h->map_enqueued_early = false;
  if (h->map_after_update && !h->net.comm && !h->prof.profiling) {
    // lii_scan_job::map_update: the map update goes out now, behind the passes, while the device still works on them
    const auto t_me0 = std::chrono::steady_clock::now();
    // (a batch that cannot be enqueued now - no room for the predicted sizes - is not this update's failure: the map update is made
    // when the update has ended, by the call that reports such things)
    h->map_enqueued_early = map_update_early(h) == 1;
    // (map_apply rebuilds the index when the map is short of room - build_index may free and reallocate the block table, the cell
    // tables and their side arrays and change the mask: a loop that parks is continued below with launches that must see the map
    // as it is NOW, not the view taken before the passes went out - ADVICE r4)
    p.g = grid_view(h);
    if (h->diag) h->prof.host_map_us[1] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_me0).count();
  }
  // lii_publish_set: the registered clouds go out now as well - behind the passes and the map update, in front of a pre-armed prologue.
  // The launch reads the final state from the control block and does nothing if the loop has parked (then it is enqueued again below).
  if (h->pub.any()) { rc = publish_enqueue(h, h->d_ctrl, nullptr, true); if (rc != LII_OK) return rc; }
  prearm_arm(h);
  run_wait_hook(h, true);
  bool parked_once = false;
  rc = p.wait();
  if (rc == LII_OK) rc = p.continue_parked(&parked_once);
  if (rc != LII_OK) return rc;
  if (h->pub.any() && parked_once) {  // (the launch behind the planned passes saw a parked loop and did nothing: once more, behind the passes that ended it)
    if (h->pub.kp_idx >= 0) h->prof.kp_kind[size_t(h->pub.kp_idx)] = LII_KP_KINDS * 64;  // (lii_set_profiling(h, 3): that launch did not execute)
    rc = publish_enqueue(h, h->d_ctrl, nullptr, false);
    if (rc != LII_OK) return rc;
  }
  note_unfinished(h);
  h->staging_busy = false;  // the wait above covers everything enqueued before the stopping pass
  h->scan_buf_idle = !h->pub.any();  // ... every launch that read or wrote the current scan buffer among it (what was enqueued behind - drained passes, the map update, a pre-armed launch on the OTHER buffer - does not touch it;
                                   // the launch and the body copy of a standing lii_publish_set order DO read it behind the stopping pass: with one, lii_scan_upload_next puts its event pair between the streams)
  const IekfResult* hr = h->h_res;
  h->have_search = true;
#ifdef LII_SOLVE_TRACE
  solve_trace(hr);
#endif
  rc = account_brackets(h, hr);
  if (rc == LII_OK) rc = result_code(h, hr);
  if (rc != LII_OK) return rc;
  std::memcpy(state, hr->st, sizeof(lii_state));
  publish_finish(h);  // (the clouds of this registration are the ones lii_publish_fetch serves from here on)
  plan_from_result(h, hr);
  fill_report(report, hr->it, hr->searches, hr->effect_num, hr->converged, hr->ne);
  if (prof) {
    // the k-NN kernel alone, over EVERY pass that actually searched (the device logs which iterations did).  The events are READ
    // LATER (harvest_knn_events: in front of the next profiled update, or when the timings are asked for): asking the runtime for
    // an event's time right behind the launch it belongs to makes it wait for its completion handler - ~10 us per pair on the
    // host's path to the next scan (round 6: a profiled step cost + 22 us against its neighbours).
    unsigned int due = 0u;
    for (int it = 0; it < opts->max_iterations && it < 16; it++) {
      if (it >= hr->it || !(hr->search_log[it] & 1) || !((plan0 >> it) & 1u)) continue;
      due |= 1u << it;
    }
    h->prof.ev_it_due = due;
  }
  return LII_OK;
}

// ------------------------------------------------------------------------------------------------ the prologues
// The 16-byte words [from, vec) of IekfCtrl are what a launch that propagates pulls from pinned memory: the two states in front of them
// are written on the device.
struct CtrlWords { int from, vec; };
CtrlWords ctrl_words() {
  static_assert(offsetof(IekfCtrl, solution) % 16 == 0 && offsetof(IekfCtrl, prop) + sizeof(IekfCtrl::prop) == offsetof(IekfCtrl, solution), "IekfCtrl: the two states come first");
  return {int(offsetof(IekfCtrl, solution) / 16), int((sizeof(IekfCtrl) + 15) / 16)};
}

// The staging buffer (control block + pose table) is this call's from here on.  poses_too: the table's half is written as well - a
// pose table uploaded by a stand-alone lii_undistort_imu (long done) must have left it.
int claim_staging(lii_handle h, bool poses_too) {
  if (h->staging_busy) HIPCHK(h, hipStreamSynchronize(h->stream));  // (a call that failed half way left the buffer in use)
  if (poses_too) HIPCHK(h, hipEventSynchronize(h->ev_poses));
  h->staging_busy = true;
  return LII_OK;
}
// Scan admission: the handle's book-keeping of the scan a prologue launch is about to de-skew.  Returns whether the insert of the
// hashed voxel filter rides in that launch.
bool admit_scan(lii_handle h, int n_next, float leaf) {
  extent_discard(h);
  h->n_scan = n_next;
  h->n_body = 0;
  h->n_body_pending = false;
  h->have_search = false;
  h->vh_inserted = fuse_filter(h, leaf);
  if (h->vh_inserted) h->vh_inserted_leaf = leaf;
  return h->vh_inserted;
}
// A scan in any order: the time-extent reduction in front - the sweep's end and the time-earliest point - adopting the scan on the
// way; the de-skew then reads the handle's buffer.  Returns the accumulator that holds the extent.
const unsigned long long* extent_for_unsorted(lii_handle h, const float4*& in, int n, bool adopt) {
  unsigned long long* e = h->d_extent + 2 * h->extent_sel;
  launch_time_extent(in, n, e, h->d_extent + 2 * (h->extent_sel ^ 1), adopt ? h->d_scan.get() : nullptr, nullptr, nullptr, 0, h->stream);
  h->extent_sel ^= 1;
  in = h->d_scan;
  return e;
}

// Behind the de-skew launch of a prologue that pre-loads the control block: the box rows it leaves - or its failure.
int deskew_launched(lii_handle h, int n_next, const char* what) {
  h->bbox_rows = (n_next + 255) / 256;
  h->ctrl_preloaded = true;
  const hipError_t e_launch = hipGetLastError();
  if (e_launch == hipSuccess) return LII_OK;
  h->vh_inserted = false; h->ctrl_preloaded = false;
  return fail(h, LII_ERR_HIP, std::string(what) + hipGetErrorString(e_launch));
}

// The prologue of lii_scan_register_imu: IMU forward propagation and de-skew, back to back on the stream.  The host's part is what it
// knows BEFORE the previous update has ended - the samples - and the state that update left; everything that depends on them (the
// propagated state, the IMUpose table, the update's control block with state and state_propagat filled in) is formed on the device.
int imu_prologue(lii_handle h, const JobView& jv, const lii_iekf_opts* opts, const ImuFeed* feed, const lii_state* state, bool adopt, const float4* src_dev,
                 int n_next) {
  if (n_next <= 0) return fail(h, LII_ERR_STATE, "lii_scan_register_imu: no scan (lii_scan_upload / lii_frame_select / lii_scan_job::scan_dev)");
  int rc = imu_buffers(h);
  if (rc != LII_OK) return rc;
  rc = claim_staging(h, true);  // (the samples take the pose table's staging area)
  if (rc != LII_OK) return rc;
  fill_ctrl(h, state, state, opts);  // (st / prop of the block on the device are written by k_imu_propagate, not pulled)
  std::memcpy(h->h_poses, feed->imu, sizeof(lii_imu_sample) * size_t(feed->n_imu));
  const bool fused = admit_scan(h, n_next, jv.leaf);
  const float4* in = adopt ? src_dev : h->d_scan.get();
  const unsigned long long* ext = jv.sorted ? nullptr : extent_for_unsorted(h, in, n_next, adopt);
  ImuPropArgs a = {};
  a.st_in = h->h_ctrl->st;
  a.samples = reinterpret_cast<const double*>(h->h_poses);
  a.n_imu = feed->n_imu;
  static_assert(sizeof(lii_imu_noise) == 8 + 19 * sizeof(double), "lii_imu_noise layout");
  std::memcpy(a.noise, h->imu.noise.cov_gyr, sizeof(a.noise));
  a.pcl_beg_time = feed->pcl_beg_time;
  a.scan = in; a.n_scan = n_next; a.sorted = jv.sorted ? 1 : 0; a.extent = ext;
  a.carry_in = h->imu.d_carry(h->imu.carry_sel);
  a.carry_out = h->imu.d_carry(h->imu.carry_sel ^ 1);
  a.poses = h->d_poses;
  a.n_poses = h->imu.d_n_poses();
  a.st_out = h->d_ctrl->st;
  a.prop_out = h->d_ctrl->prop;
  a.host_out = feed->prop_out ? h->imu.h_out.get() : nullptr;
  a.ctrl_src = reinterpret_cast<const uint4*>(h->h_ctrl);
  a.ctrl_dst = reinterpret_cast<uint4*>(h->d_ctrl);
  a.ctrl_from = ctrl_words().from;
  a.ctrl_vec = ctrl_words().vec;
  launch_imu_propagate(a, h->stream);
  const hipError_t e_prop = hipGetLastError();
  if (e_prop != hipSuccess) { h->vh_inserted = false; return fail(h, LII_ERR_HIP, std::string("IMU propagation launch: ") + hipGetErrorString(e_prop)); }
  h->imu.carry_sel ^= 1;  // the launch is on the stream: the carry it writes is the current one from here on, whatever becomes of the rest of the call
  if (h->prof.kp_active) { rc = kp_mark(h, LII_KP_DESKEW); if (rc != LII_OK) return rc; }
  const DeskewPlan dp = deskew_plan(h, in, h->d_scan, n_next, jv.sorted, ext, jv.leaf, fused, DeskewCtrl::ahead);
  launch_deskew_imu_dev(dp, h->d_ctrl->st, h->imu.d_n_poses(), h->d_poses, h->stream);
  return deskew_launched(h, n_next, "de-skew launch behind the IMU propagation: ");
}

// The prologue of lii_scan_register_cv: ONE launch, the CV de-skew whose extra workgroup propagates (k_deskew_cv_prop).  The host hands
// over the state the previous update left - inside the control block in pinned memory for the extra workgroup, rot_end / bias_g /
// vel_end by value for the scan workgroups - and never sees the propagated one unless it asks for it.
int cv_prologue(lii_handle h, const JobView& jv, const lii_iekf_opts* opts, const CvFeed* cv, const lii_state* state, bool adopt, const float4* src_dev,
                int n_next) {
  if (n_next <= 0) return fail(h, LII_ERR_STATE, "lii_scan_register_cv: no scan (lii_scan_upload / lii_frame_select / lii_scan_job::scan_dev)");
  int rc = LII_OK;
  if (cv->prop_out) { rc = imu_buffers(h); if (rc != LII_OK) return rc; }
  rc = claim_staging(h, false);
  if (rc != LII_OK) return rc;
  fill_ctrl(h, state, state, opts);  // (st / prop of the block on the device are written by the extra workgroup, not pulled; st is what it reads)
  const bool fused = admit_scan(h, n_next, jv.leaf);
  const float4* in = adopt ? src_dev : h->d_scan.get();
  // (a scan in any order: as on lii_scan_register's general path)
  const unsigned long long* ext = jv.sorted ? nullptr : extent_for_unsorted(h, in, n_next, adopt);
  const DeskewPlan dp = deskew_plan(h, in, h->d_scan, n_next, jv.sorted, ext, jv.leaf, fused, DeskewCtrl::pulled);
  CvFuseH f = {};
  std::memcpy(f.rot, state->rot_end, 72);
  std::memcpy(f.bias_g, state->bias_g, 24);
  std::memcpy(f.vel, state->vel_end, 24);
  f.dt = cv->dt;
  std::memcpy(f.cov_gyr_scale, cv->cov_gyr_scale, 24);
  std::memcpy(f.cov_acc_scale, cv->cov_acc_scale, 24);
  f.st_in = h->h_ctrl->st;
  f.st_out = h->d_ctrl->st;
  f.prop_out = h->d_ctrl->prop;
  f.host_out = cv->prop_out ? h->imu.h_out.get() : nullptr;
  f.ctrl_from = ctrl_words().from;
  launch_deskew_cv_prop(dp, f, h->stream);
  return deskew_launched(h, n_next, "de-skew launch with the CV propagation: ");
}

// The prologue of a lii_scan_register job whose scan is in ascending time order: ONE launch takes it from wherever it arrived (the
// caller's device buffer is read in place) to the de-skewed scan with the voxel filter's table filled, and one extra workgroup of it
// pulls the update's control block over PCIe; the IMU pose table (<= 64 poses) travels in the kernel arguments.  Round 3 needed
// k_time_extent in front (copy + time extent + pull: 8.9 us per scan).  use_pre: that launch waits on the stream already (prearm_go).
// A failed launch is reported through *rc and the call goes on to its clean-up; the return value ends the call at once.
int fast_prologue(lii_handle h, const JobView& jv, const lii_iekf_opts* opts, const lii_state* state, const lii_state* state_prop, bool adopt,
                  const float4* src_dev, int n_next, bool use_pre, int* rc) {
  const int rc_claim = claim_staging(h, false);
  if (rc_claim != LII_OK) return rc_claim;
  fill_ctrl(h, state, state_prop, opts);
  h->ctrl_preloaded = true;
  const bool fused = admit_scan(h, n_next, jv.leaf);
  if (use_pre) use_pre = prearm_go(h, state, jv.poses, jv.n_poses);
  const DeskewPlan dp = deskew_plan(h, adopt ? src_dev : h->d_scan.get(), h->d_scan, n_next, true, nullptr, jv.leaf, fused, DeskewCtrl::pulled);
  if (use_pre) {
    // (the launch is on the stream already and has its go)
  } else if (jv.undistort == 1) {
    UndistArgH u;
    std::memcpy(u.endR, state->rot_end, 72);
    std::memcpy(u.endp, state->pos_end, 24);
    std::memcpy(u.RLI, state->offset_R_L_I, 72);
    std::memcpy(u.TLI, state->offset_T_L_I, 24);
    launch_deskew_imu(dp, reinterpret_cast<const double*>(jv.poses), nullptr, jv.n_poses, u, h->stream);
  } else {
    CvArgH a;  // CV model: bias_g = omega, vel_end = v
    std::memcpy(a.omega, state->bias_g, 24);
    std::memcpy(a.vel, state->vel_end, 24);
    std::memcpy(a.endR, state->rot_end, 72);
    launch_deskew_cv(dp, a, h->stream);
  }
  *rc = deskew_launched(h, n_next, "de-skew launch: ");
  return LII_OK;
}

// The prologue of every other lii_scan_register job (a scan in any order, LII_TEST=host_solve / no_fast, a long pose table, no
// de-skew): control block and pose staging, then the public entry points.  *rc and the return value: as for fast_prologue.
int general_prologue(lii_handle h, const JobView& jv, const lii_iekf_opts* opts, const lii_state* state, const lii_state* state_prop, bool adopt,
                     const void* src_dev, int src_n, int n_next, int* rc) {
  if (jv.undistort == 1 && !h->host_solve && jv.poses && jv.n_poses >= 2 && jv.n_poses <= 1024 && n_next > 0) {
    // the control block of the update AND the pose table of the de-skew (they sit behind each other) reach the device once.
    // The staging buffer is free again: the previous call returned after its stopping pass, which runs behind the kernel
    // that read the buffer - unless that call failed half way (then wait).  No event: recording one between the de-skew and
    // the voxel filter cost a ~5 us bubble on the device per scan.
    const int rc_claim = claim_staging(h, true);
    if (rc_claim != LII_OK) return rc_claim;
    fill_ctrl(h, state, state_prop, opts);
    std::memcpy(h->h_poses, jv.poses, sizeof(lii_pose6d) * size_t(jv.n_poses));
    const size_t bytes = kCtrlBytes + sizeof(lii_pose6d) * size_t(jv.n_poses);
    if (adopt || !h->extent_valid) {
      h->ctrl_pending = (bytes + 15) / 16 * 16;  // rides in the scan's first kernel (k_time_extent), which is launched below
    } else {
      // (size rounded to 1 KiB: the runtime splits an H2D copy with an unaligned tail into two blit kernels)
      HIPCHK(h, hipMemcpyAsync(h->d_ctrl, h->h_ctrl, (bytes + 1023) / 1024 * 1024, hipMemcpyHostToDevice, h->stream));
    }
    h->poses_preloaded = h->ctrl_preloaded = true;
  }
  if (adopt) {
    const bool keep = h->inten.have;  // (a selected ingest frame moves into the handle's buffer: its intensities, copied when it was selected, stay)
    const int rc_set = lii_scan_set_device(h, src_dev, src_n);
    if (rc_set == LII_OK) h->inten.have = keep;
    if (rc_set != LII_OK) { h->ctrl_pending = 0; h->poses_preloaded = h->ctrl_preloaded = false; return rc_set; }
  }
  if (jv.undistort == 1 || jv.undistort == 2) {
    h->fuse_leaf = jv.leaf;  // (the voxel filter follows in this call: its insert may ride in the de-skew)
    *rc = jv.undistort == 1 ? lii_undistort_imu(h, jv.poses, jv.n_poses, state->rot_end, state->pos_end, state->offset_R_L_I, state->offset_T_L_I)
                            : lii_undistort_cv(h, state->bias_g, state->vel_end, state->rot_end);  // CV model: bias_g = omega, vel_end = v
    h->fuse_leaf = 0.f;
    if (*rc != LII_OK) h->vh_inserted = false;
  }
  return LII_OK;
}

// LII_DIAG: the host's times of one call (lii_context::prof.host_us)
void note_host_times(lii_handle h, std::chrono::steady_clock::time_point t_entry, std::chrono::steady_clock::time_point t_first,
                     std::chrono::steady_clock::time_point t_pre) {
  if (!h->diag) return;
  const auto t_end = std::chrono::steady_clock::now();
  h->prof.host_us[0] += std::chrono::duration<double, std::micro>(t_first - t_entry).count();
  h->prof.host_us[1] += std::chrono::duration<double, std::micro>(t_pre - t_entry).count();
  h->prof.host_us[2] += h->prof.host_loop_enq_us;
  h->prof.host_us[3] += std::chrono::duration<double, std::micro>(t_end - t_entry).count();
  h->prof.host_us[4] += 1;
  h->prof.host_last_return = t_end;
}

}  // namespace

// lii_scan_register, and - feed != nullptr - lii_scan_register_imu, - cv != nullptr - lii_scan_register_cv (lii_capi_imu.cpp: their checks
// are made there; state_prop is not used)
int lii_impl::scan_register_job(lii_handle h, const lii_scan_job* job, lii_state* state, const lii_state* state_prop, lii_iekf_report* report,
                                const ImuFeed* feed, const CvFeed* cv) {
  const char* const who = feed ? "lii_scan_register_imu" : (cv ? "lii_scan_register_cv" : "lii_scan_register");
  if (!h || !job || !job_size_ok(job->struct_size) || !state || (!state_prop && !feed && !cv) || job->opts.max_iterations < 1)
    return fail(h, LII_ERR_INVALID, std::string(who) + ": bad arguments");
  const JobView jv = job_view(job);
  if (jv.sort_first && (h->net.comm || h->net.n_ranks > 1)) return fail(h, LII_ERR_STATE, std::string(who) + ": scan_sorted = 2 is single rank only for now (a communicator is attached)");
  // lii_local_map_set(enabled): this call segments by itself (update_on_device).  Single rank, and not under LII_TEST=host_solve: the
  // decision reads the device-resident control block, which the host-driven loop does not have.
  const bool local_map = h->lm.enabled;
  if (local_map && (h->net.comm || h->net.n_ranks > 1)) return fail(h, LII_ERR_STATE, std::string(who) + ": the local map (lii_local_map_set) is single rank only for now (a communicator is attached)");
  if (local_map && h->host_solve) return fail(h, LII_ERR_STATE, std::string(who) + ": the local map (lii_local_map_set) is not available under LII_TEST=host_solve; call lii_local_map_segment");
  h->scan_buf_idle = false;
  int rc = LII_OK;
  const auto t_entry = std::chrono::steady_clock::now();
  if (h->diag && h->prof.host_us[4] > 0) h->prof.host_us[5] += std::chrono::duration<double, std::micro>(t_entry - h->prof.host_last_return).count();
  // the scan to adopt: the caller's device buffer (lii_scan_job::scan_dev), or the frame lii_frame_select left where the ingest put it
  const bool from_job = jv.scan_dev != nullptr && jv.n_scan_dev > 0;
  const void* src_dev = from_job ? jv.scan_dev : static_cast<const void*>(h->scan_pending);
  const int src_n = from_job ? jv.n_scan_dev : h->scan_pending_n;
  bool adopt = src_dev != nullptr && src_n > 0;
  // (this refusal comes BEFORE a waiting launch is told to end, the undistort range check below behind it: both stay where they were)
  if (adopt && src_n > h->cfg.max_scan_points) return fail(h, LII_ERR_CAPACITY, std::string(who) + ": n_scan_dev > max_scan_points");
  if (from_job) intensity_detach(h);  // (the job's scan_dev replaces the current scan: a scan with intensities is handed over by lii_scan_set_device + lii_scan_intensity_set_device)
  const int n_next = adopt ? src_n : h->n_scan;
  // A gated de-skew launch waits on the stream (the previous call enqueued it for the scan its job announced): it is used when THIS
  // call asks for exactly that, and told to end otherwise - before anything here could wait for the stream.
  // (the announced scan: the job's own device buffer, or - announced while lii_scan_upload_next was bringing it - the handle's current
  // scan after lii_scan_advance, de-skewed in place)
  const void* const cur_dev = from_job ? jv.scan_dev : (adopt ? nullptr : static_cast<const void*>(h->d_scan));
  const int cur_n = from_job ? jv.n_scan_dev : h->n_scan;
  // (lii_scan_register_imu / _cv, a job that sorts, a handle with the local map enabled: a waiting launch is ended, and nothing is announced)
  const bool may_announce = !feed && !cv && !jv.sort_first && !local_map;
  bool use_pre = may_announce && h->pre.armed && jv.sorted && jv.undistort == 1 && jv.poses && jv.n_poses >= 2 && jv.n_poses <= lii::kGateMaxPoses &&
                 cur_dev != nullptr && cur_dev == h->pre.scan_dev && cur_n == h->pre.n && h->pre.late == !from_job && jv.leaf == h->pre.leaf && !h->host_solve && !h->no_fast_prologue &&
                 h->prof.prof_mode != 3 && !h->staging_busy && fuse_filter(h, jv.leaf) == h->pre.fuse;
  if (!use_pre) prearm_cancel(h);
  prearm_wanted(h, jv, may_announce, from_job);
  h->prof.kp_active = h->prof.prof_mode == 3 && !h->host_solve;
  h->prof.kp_n = 0;
  if (h->prof.kp_active) { rc = kp_mark(h, feed ? LII_KP_PROPAGATE : LII_KP_DESKEW); if (rc != LII_OK) { h->prof.kp_active = false; return rc; } }
  const bool fast = jv.sorted && !h->host_solve && n_next > 0 && !h->no_fast_prologue &&
                    ((jv.undistort == 1 && jv.poses && jv.n_poses >= 2 && jv.n_poses <= 64) || jv.undistort == 2);
  if (use_pre && !fast) { prearm_cancel(h); use_pre = false; }  // (cannot happen with the conditions above; a waiting launch must never be left behind a call that will not feed it)
  if (jv.undistort != 0 && jv.undistort != 1 && jv.undistort != 2) return fail(h, LII_ERR_INVALID, std::string(who) + ": undistort must be 0, 1 or 2");
  const auto t_first = std::chrono::steady_clock::now();
  if (jv.sort_first && n_next > 0) {
    // (behind the first profiling mark: lii_set_profiling(h, 3) counts these launches where it counts the time-extent launch of a scan in any order)
    rc = scan_sort_into(h, adopt ? static_cast<const float4*>(src_dev) : h->d_scan.get(), n_next);
    if (rc != LII_OK) { h->prof.kp_active = false; return rc; }
    extent_discard(h);  // (the sorted scan in d_scan is the current one: a selected frame has been read, an extent of the old order is void)
    h->n_scan = n_next;
    h->bbox_rows = 0;
    adopt = false;
    src_dev = nullptr;
  }
  const float4* const src4 = static_cast<const float4*>(src_dev);
  if (feed || cv) {
    rc = feed ? imu_prologue(h, jv, &job->opts, feed, state, adopt, src4, n_next) : cv_prologue(h, jv, &job->opts, cv, state, adopt, src4, n_next);
    if (rc != LII_OK) { h->prof.kp_active = false; return rc; }
  } else {
    const int rc_now = fast ? fast_prologue(h, jv, &job->opts, state, state_prop, adopt, src4, n_next, use_pre, &rc)
                            : general_prologue(h, jv, &job->opts, state, state_prop, adopt, src_dev, src_n, n_next, &rc);
    if (rc_now != LII_OK) return rc_now;
  }
  if (h->ctrl_preloaded && h->ctrl_pending) {  // no kernel picked the block up (cannot happen with the conditions above; a guard)
    HIPCHK(h, hipMemcpyAsync(h->d_ctrl, h->h_ctrl, h->ctrl_pending, hipMemcpyHostToDevice, h->stream));
    h->ctrl_pending = 0;
  }
  if (rc == LII_OK) rc = jv.leaf > 0 ? lii_downsample(h, jv.leaf, nullptr, nullptr) : lii_downsample_skip(h, nullptr);
  const auto t_pre = std::chrono::steady_clock::now();
  h->map_after_update = jv.map_update && !h->host_solve;
  h->map_enqueued_early = false;
  h->wait_hook = rc == LII_OK ? jv.while_waiting : nullptr;  // (run_wait_hook)
  h->wait_hook_arg = jv.while_waiting_arg;
  h->lm.in_job = local_map && rc == LII_OK;
  if (rc == LII_OK) rc = lii_iekf_update(h, state, state_prop ? state_prop : state, &job->opts, report);
  if (h->lm.in_job) {
    // (the update's result came back behind the local-map call: its report is in pinned memory, and the host's live-point count takes
    // it - a call that failed on the way leaves the count to the next read of the device's counters)
    if (rc == LII_OK) local_map_settle(h);
    else h->lm.counts_pending = true;
    h->lm.in_job = false;
  }
  run_wait_hook(h, false);
  h->map_after_update = false;
  // map_incremental behind the update: already enqueued behind its passes (update_on_device), or made now
  if (rc == LII_OK && jv.map_update && !h->map_enqueued_early) rc = lii_map_incremental(h, state, nullptr, nullptr);
  h->map_enqueued_early = false;
  h->poses_preloaded = h->ctrl_preloaded = false;  // also on the error paths
  h->prof.kp_active = false;
  note_host_times(h, t_entry, t_first, t_pre);
  // the propagated state, as k_imu_propagate (lii_scan_register_imu) / the extra workgroup of k_deskew_cv_prop (lii_scan_register_cv) left
  // it in mapped host memory (it ran in front of the passes whose result has arrived)
  lii_state* const prop_out = feed ? feed->prop_out : (cv ? cv->prop_out : nullptr);
  if (rc == LII_OK && prop_out) std::memcpy(prop_out, h->imu.h_out.get(), sizeof(lii_state));
  return rc;
}

extern "C" {

// ------------------------------------------------------------------------------------------------ registration
int lii_last_solve_info(lii_handle h, int32_t* pivoted_passes) {
  if (!h || !pivoted_passes) return LII_ERR_INVALID;
  *pivoted_passes = h->last_pivoted_passes;
  return LII_OK;
}

int lii_last_unfinished_queries(lii_handle h, int32_t* n_last) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !n_last) return LII_ERR_INVALID;
  if (h->unfinished_known) { *n_last = h->h_res->unfinished; return LII_OK; }  // (came with the last update's result: the largest count among its search passes)
  int c[2] = {0, 0};
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(c, h->d_flags, sizeof(c), hipMemcpyDeviceToHost));  // RegistrationBuffers::flag_count, one word per slot
  *n_last = c[h->knn_epoch & 1];  // (consecutive launch numbers alternate between the two slots; a launch clears the other one)
  return LII_OK;
}

int lii_iekf_iterate(lii_handle h, const lii_state* state, int32_t search, int32_t imu_en, double out91[91]) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !state || !out91) return fail(h, LII_ERR_INVALID, "lii_iekf_iterate: bad arguments");
  return iterate(h, state, search != 0, imu_en != 0, out91);
}

int lii_iekf_update(lii_handle h, lii_state* state, const lii_state* state_prop, const lii_iekf_opts* opts,
                    lii_iekf_report* report) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !state || !state_prop || !opts || opts->max_iterations < 1) return fail(h, LII_ERR_INVALID, "lii_iekf_update: bad arguments");
  const int max_it = opts->max_iterations;
  auto t_begin = std::chrono::steady_clock::now();
  if (!h->host_solve) {
    int rc = update_on_device(h, state, state_prop, opts, report);
    h->prof.timings[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    return rc;
  }
  double host_ms = 0;
  // cov is constant inside the loop (it is only rewritten on exit, :1112-1114), so invert it once
  std::vector<double> Pinv(kDim * kDim), A(kDim * kDim), K1(kDim * kDim), KH(kDim * 12), G(kDim * kDim);
  if (!mat_inverse(state->cov, kDim, Pinv.data())) return fail(h, LII_ERR_INVALID, "state covariance is singular");
  int rematch_num = 0;
  bool search = true, stop = false, converged = false;
  int it = 0, searches = 0;
  double ne[kNormalEq];
  for (it = 0; it < max_it; it++) {
    int rc = iterate(h, state, search, opts->imu_en != 0, ne);
    if (rc != LII_OK) return rc;
    if (search) searches++;
    auto t0 = std::chrono::steady_clock::now();
    // H_T_H (+) P^-1  (:1080-1081)
    A = Pinv;
    double HTH[12][12];
    int t = 0;
    for (int i = 0; i < 12; i++)
      for (int j = i; j < 12; j++) { HTH[i][j] = ne[t]; HTH[j][i] = ne[t]; t++; }
    for (int i = 0; i < 12; i++)
      for (int j = 0; j < 12; j++) A[size_t(i) * kDim + j] += HTH[i][j];
    if (!mat_inverse(A.data(), kDim, K1.data())) return fail(h, LII_ERR_INVALID, "normal matrix is singular");
    double vec[kDim], sol[kDim];
    state_minus(*state_prop, *state, vec);
    for (int r = 0; r < kDim; r++) {
      double kz = 0;
      for (int c = 0; c < 12; c++) kz += K1[size_t(r) * kDim + c] * ne[78 + c];
      double khv = 0;
      for (int c = 0; c < 12; c++) {
        double s = 0;
        for (int k = 0; k < 12; k++) s += K1[size_t(r) * kDim + k] * HTH[k][c];
        KH[size_t(r) * 12 + c] = s;
        khv += s * vec[c];
      }
      sol[r] = kz + vec[r] - khv;
    }
    state_plus(*state, sol);
    double rn = std::sqrt(sol[0] * sol[0] + sol[1] * sol[1] + sol[2] * sol[2]);
    double tn = std::sqrt(sol[3] * sol[3] + sol[4] * sol[4] + sol[5] * sol[5]);
    converged = (rn * 57.3 < 0.01) && (tn * 100 < 0.015);
    search = false;
    if (converged || ((rematch_num == 0) && (it == (max_it - 2)))) {
      search = true;
      rematch_num++;
    }
    if (!stop && (rematch_num >= 2 || (it == max_it - 1))) {
      // state.cov = (I - G) cov, G[:, :12] = K H   (:1111-1114)
      std::vector<double> newcov(kDim * kDim);
      for (int r = 0; r < kDim; r++)
        for (int c = 0; c < kDim; c++) {
          double s = state->cov[size_t(r) * kDim + c];
          for (int k = 0; k < 12; k++) s -= KH[size_t(r) * 12 + k] * state->cov[size_t(k) * kDim + c];
          newcov[size_t(r) * kDim + c] = s;
        }
      std::memcpy(state->cov, newcov.data(), sizeof(double) * kDim * kDim);
      stop = true;
    }
    host_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stop) { it++; break; }
  }
  fill_report(report, it, searches, int(ne[90]), converged ? 1 : 0, ne);
  h->prof.timings[3] = host_ms;
  h->prof.timings[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return LII_OK;
}

int lii_scan_register(lii_handle h, const lii_scan_job* job, lii_state* state, const lii_state* state_prop,
                      lii_iekf_report* report) {
  return scan_register_job(h, job, state, state_prop, report, nullptr);
}
// ------------------------------------------------------------------------------------------------ per-point measurement noise
int lii_point_noise_set(lii_handle h, const lii_point_noise* m) {
  if (!h) return LII_ERR_INVALID;
  if (m && m->struct_size != sizeof(lii_point_noise)) return fail(h, LII_ERR_INVALID, "lii_point_noise_set: struct_size");
  const int model = m ? m->model : 0;
  if (model != 0 && model != 1) return fail(h, LII_ERR_INVALID, "lii_point_noise_set: model must be 0 or 1");
  if (m && !(std::isfinite(m->range_inc) && m->range_inc >= 0.0 && std::isfinite(m->degree_inc) && m->degree_inc >= 0.0))
    return fail(h, LII_ERR_INVALID, "lii_point_noise_set: range_inc and degree_inc must be finite and not negative");
  if (h->net.comm || h->net.n_ranks > 1) return fail(h, LII_ERR_STATE, "lii_point_noise_set: single rank only for now (a communicator is attached)");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_point_noise_set: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end)
  if (model == 1 && !h->noise.d_buf) {
    const size_t bytes = size_t(lii::kNoiseHeadBytes) + sizeof(float) * size_t(std::max(h->cfg.max_scan_points, 1));
    HIPCHK(h, h->noise.d_buf.alloc(bytes));
    HIPCHK(h, hipMemsetAsync(h->noise.d_buf, 0, bytes, h->stream));  // (nothing reads a point's entry before a fit pass has written it; zeros all the same)
  }
  h->noise.model = model;
  h->noise.range_inc = m ? m->range_inc : 0.0;
  h->noise.degree_inc = m ? m->degree_inc : 0.0;
  h->noise.have_pass = false;
  if (model == 1) {
    // calcBodyVar (src/laserMapping.cpp:158-164): range_inc, range_var and degree_inc are floats there.  0.017453293: PCL's DEG2RAD macro as
    // the reference compiles it - restated from knowledge of PCL, not pinned by a build.
    const float ri = (float)m->range_inc;
    const double sn = std::sin((double)(float)m->degree_inc * 0.017453293);
    static_assert(sizeof(lii::NoiseArg) <= size_t(lii::kNoiseHeadBytes), "the constants stand in front of the buffer");
    const lii::NoiseArg arg = {1.0 / h->cfg.laser_point_cov_inv /* LASER_POINT_COV */, (double)(ri * ri), sn * sn};
    // (the fit launches read them there; launches still on the stream are drained passes, which return before they would)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(h->noise.d_buf, &arg, sizeof(arg), hipMemcpyHostToDevice));
  }
  return LII_OK;
}
int lii_point_noise_get(lii_handle h, lii_point_noise* m) {
  if (!h) return LII_ERR_INVALID;
  if (!m || m->struct_size != sizeof(lii_point_noise)) return fail(h, LII_ERR_INVALID, "lii_point_noise_get: bad arguments");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_point_noise_get: a registration is under way (lii_scan_job::while_waiting)");
  m->model = h->noise.model;
  m->range_inc = h->noise.range_inc;
  m->degree_inc = h->noise.degree_inc;
  return LII_OK;
}
int lii_point_noise_download(lii_handle h, float* sqrt_rinv, int32_t capacity, int32_t* n) {
  if (!h) return LII_ERR_INVALID;
  if (!n) return fail(h, LII_ERR_INVALID, "lii_point_noise_download: bad arguments");
  if (h->in_wait_hook) return fail(h, LII_ERR_STATE, "lii_point_noise_download: a registration is under way (lii_scan_job::while_waiting)");
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (h->noise.model != 1) return fail(h, LII_ERR_STATE, "lii_point_noise_download: model 0 (lii_point_noise_set)");
  if (!h->noise.have_pass) return fail(h, LII_ERR_STATE, "lii_point_noise_download: no fit pass since the model was set");
  { int rc0 = resolve_n_body(h); if (rc0 != LII_OK) return rc0; }
  const int rows = h->n_body;
  *n = rows;
  if (capacity < rows) return fail(h, LII_ERR_CAPACITY, "lii_point_noise_download: capacity too small");
  if (rows == 0) return LII_OK;
  if (!sqrt_rinv) return fail(h, LII_ERR_INVALID, "lii_point_noise_download: bad arguments");
  HIPCHK(h, hipMemcpyAsync(h->h_stage, h->noise.d_sqrt_rinv(), sizeof(float) * size_t(rows), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::memcpy(sqrt_rinv, h->h_stage.get(), sizeof(float) * size_t(rows));
  return LII_OK;
}

int lii_neighbors_download(lii_handle h, float* pts, int32_t* counts, uint8_t* selected, int32_t capacity) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h) return LII_ERR_INVALID;
  { int rc0 = resolve_n_body(h); if (rc0 != LII_OK) return rc0; }
  const int n = h->n_body;
  if (capacity < n) return fail(h, LII_ERR_CAPACITY, "lii_neighbors_download: capacity too small");
  if (n == 0) return LII_OK;
  const size_t cap = size_t(h->cfg.max_scan_points);
  hipStream_t s = h->stream;
  const int* perm = nullptr;  // rows come out in the order lii_scan_download(1) uses (the reference's feats_down_body order)
  { int rc1 = pcl_order(h, &perm); if (rc1 != LII_OK) return rc1; }
  if (pts) {
    for (int k = 0; k < kMatch; k++)
      HIPCHK(h, hipMemcpyAsync(h->h_stage + size_t(k) * n, h->d_nbr + size_t(k) * cap, sizeof(float4) * size_t(n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int i = 0; i < n; i++)
      for (int k = 0; k < kMatch; k++) {
        const float4 v = h->h_stage[size_t(k) * n + (perm ? perm[i] : i)];
        float* o = pts + (size_t(i) * kMatch + k) * 3;
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
      }
  }
  if (counts) {
    HIPCHK(h, hipMemcpyAsync(h->h_stage, h->d_nbr_count, sizeof(int) * size_t(n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const int* src = reinterpret_cast<const int*>(h->h_stage.get());
    for (int i = 0; i < n; i++) counts[i] = src[perm ? perm[i] : i] & kCountMask;  // (without the completion flags)
  }
  if (selected) {
    HIPCHK(h, hipMemcpyAsync(h->h_stage, h->d_selected, size_t(n), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const uint8_t* src = reinterpret_cast<const uint8_t*>(h->h_stage.get());
    for (int i = 0; i < n; i++) selected[i] = src[perm ? perm[i] : i];
  }
  return LII_OK;
}
}  // extern "C"

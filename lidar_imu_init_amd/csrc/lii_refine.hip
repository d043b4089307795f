// libliinit_hip — the iterated update at K candidate poses, on the device (lii_pose_refine / lii_pose_refine_dev).
// Reference: src/laserMapping.cpp:957-1134 in LO mode (imu_en = false, :1063-1066) restricted to the six pose states - the per-point pass
// (:968-1020: pointBodyToWorld, Nearest_Search, the test of :981-984, esti_plane, pd2 and the gate s > 0.9), the rows and sums
// (:1035-1080, R_inv the config's constant), the solve (:1081-1087), the rematch schedule and the covariance update (:1093-1133) - run
// `updates` times in a row from each pose.
//
// A ROUND is two launches, and a call is updates x max_iterations rounds enqueued at once; the device decides what a round does for a
// pose from that pose's control record (RefineCtrl), which the solve of the round before wrote.  Round 0 reads the caller's poses instead.
// k_refine_pass<WAVES>: one workgroup of WAVES wavefronts per 64 consecutive points of one pose - k_pose_score's shape (lii_score.hip).
//   search pass   every lane forms the world point of pair (threadIdx.x & 63); each wavefront takes 64 / WAVES of the pairs through the
//                 exact search of the map queries (ring_walk_nearest: k = 5, d2 <= max_match_dist2 inclusive), lists in LDS only; lane L of
//                 the first wavefront fits the plane of pair L (canon_ties, fit_plane) and stores it with the pair's selection flag.
//   cached pass   lane L loads the plane and the flag of pair L: the lists and the sticky selection of this pose's last pass.
//   either way    pd2, the gate, the row h = [[p_I]x R^T n, n] and z = -pd2 (residual_row, lii_row.h), then the workgroup's partial: the 21
//                 sums of h^T h, the 6 of h^T z, the sum of |pd2| - lane t adds term t of the 64 rows in lane order, in double - and
//                 effect_num as the popcount of a ballot.
// k_refine_solve: one wavefront per pose; lane l adds the partials l, l + 64, ... in that order, then a fixed tree over the lanes; lane 0
//   then takes the step of :1081-1087 on the six states (two 6 x 6 Gauss-Jordan eliminations with row pivoting, in LDS), the boxplus, the
//   convergence test and the schedule, the covariance update where an update ends, and writes the control record of the next round -
//   and, where the last update ends, the caller's record.
// A pose whose last update has ended, or one with a NaN / Inf entry, costs a round one load of its control record per workgroup.
// Which workgroup holds which pairs, and every order of addition, depend on the point's index alone; a pose reads and writes only its own
// records: its bits are the same wherever it stands in whatever batch.  No atomics, no launch that waits for another workgroup, no
// spin on memory.  Every loop is bounded by a number known before it starts: 64 pairs, the walk's own bounds, 64 rows, the partials of a
// pose, 6 pivots.
#include "lii_launch.h"
#include "lii_plane.h"
#include "lii_ringwalk.h"
#include "lii_row.h"

namespace lii {
namespace {

constexpr int kRefinePairs = 64;        // (pose, point) pairs of a workgroup: one per lane of the wavefront that fits
// (kSmallBatchBlocks, lii_launch.h: workgroups up to which four wavefronts search a workgroup's pairs - lii_score.hip's estimate, taken over;
// nothing was measured for this launch, whose workgroups also form rows and sums.  The bits do not depend on it.)
constexpr int kTerms = 28;              // 21 (upper triangle of h^T h) + 6 (h^T z) + 1 (sum |pd2|)
constexpr int kRowStride = 9;           // doubles a row in LDS: h[6], z, |pd2|, one of padding

struct PassShared {
  float4 nb[kRefinePairs][kMatch];  // the list of pair j: xyz, w = d2
  int found[kRefinePairs];
  double row[kRefinePairs * kRowStride];
};

__device__ __forceinline__ bool finite12(const double* pk) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 12; c++) ok = ok && fabs(pk[c]) <= 1.7976931348623157e308;  // (false for NaN)
  return ok;
}

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_refine_pass(GridView g, unsigned int n_entries, unsigned int pts_cap, const float4* __restrict__ body, int n,
                                                             int chunks, PoseArg ps, const double* __restrict__ poses, int round,
                                                             const RefineCtrl* __restrict__ ctrl, int r_max, double plane_thr,
                                                             double* __restrict__ planes, unsigned char* __restrict__ flags,
                                                             RefinePartial* __restrict__ partials) {
  __shared__ PassShared sh;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned int pose = blockIdx.x / (unsigned int)chunks, chunk = blockIdx.x - pose * (unsigned int)chunks;
  // ---- what this round does for the pose (uniform over the workgroup)
  bool search = true;
  if (round == 0) {
    const double* pk = poses + 12 * (size_t)pose;
    if (!finite12(pk)) return;
#pragma unroll
    for (int c = 0; c < 9; c++) ps.R[c] = pk[c];
#pragma unroll
    for (int c = 0; c < 3; c++) ps.p[c] = pk[9 + c];
  } else {
    const RefineCtrl* ck = ctrl + pose;
    if (ck->done) return;
    search = ck->search != 0;
#pragma unroll
    for (int c = 0; c < 9; c++) ps.R[c] = ck->R[c];
#pragma unroll
    for (int c = 0; c < 3; c++) ps.p[c] = ck->p[c];
  }
  const int first = (int)chunk * kRefinePairs;  // (< n: chunks = ceil(n / 64))
  const int n_here = min(kRefinePairs, n - first);
  const bool live = lane < n_here;
  const float4 pb = live ? body[first + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
  float wx, wy, wz;
  body_to_world(ps, pb, wx, wy, wz);
  if (search) {
    // ---- this wavefront's pairs one after the other, the whole wavefront on each (uniform trip count)
    constexpr int kPairsPerWave = kRefinePairs / WAVES;
    for (int j = wave * kPairsPerWave; j < (wave + 1) * kPairsPerWave; j++) {
      const float qx = __shfl(wx, j), qy = __shfl(wy, j), qz = __shfl(wz, j);
      float my_d = INFINITY;
      unsigned int my_i = kFree;
      if (j < n_here) ring_walk_nearest(g, n_entries, pts_cap, qx, qy, qz, kMatch, g.max_d2, r_max, my_d, my_i);  // (uniform)
      const bool have = lane < kMatch && my_i != kFree;
      if (lane < kMatch) {
        float4 v = make_float4(0.f, 0.f, 0.f, my_d);
        if (have) {
          const F3 m = load_xyz(g.pts, my_i);  // (my_i < pts_cap: cell_range_checked cuts every range there)
          v.x = m.x; v.y = m.y; v.z = m.z;
        }
        sh.nb[j][lane] = v;
      }
      const int found = __popcll(__ballot(have));
      if (lane == 0) sh.found[j] = found;
    }
    __syncthreads();  // (search is uniform: every wavefront arrives)
  }
  if (wave != 0) return;  // (nothing below waits for the workgroup)
  // ---- plane and candidate flag of pair L: fitted behind a search, else what this pose's last pass left
  const size_t pair = (size_t)pose * (size_t)n + (size_t)(first + lane);  // (< 2^31: the caller bounds n_poses * n)
  bool candidate = false;
  double pa = 0, pbn = 0, pc = 0, pd = 0;
  if (live) {
    if (search) {
      float4 nb[kMatch];
#pragma unroll
      for (int j = 0; j < kMatch; j++) nb[j] = sh.nb[lane][j];
      const bool full = sh.found[lane] == kMatch;
      if (full) canon_ties(nb);
      candidate = full && !(nb[4].w > 5.0f);  // (:981-984)
      if (candidate) candidate = fit_plane(nb, plane_thr, pa, pbn, pc, pd);
      double* pl = planes + 4 * pair;
      pl[0] = pa; pl[1] = pbn; pl[2] = pc; pl[3] = pd;
    } else {
      candidate = flags[pair] != 0;
      const double* pl = planes + 4 * pair;
      pa = pl[0]; pbn = pl[1]; pc = pl[2]; pd = pl[3];
    }
  }
  // ---- gate and row
  RowOut o;
#pragma unroll
  for (int c = 0; c < 12; c++) o.h[c] = 0.0;
  o.z = 0.0;
  o.sel = false;
  if (candidate) {
    const double bx = pb.x, by = pb.y, bz = pb.z;
    const double ix = ps.RLI[0] * bx + ps.RLI[1] * by + ps.RLI[2] * bz + ps.TLI[0];  // p_I, as body_to_world forms it
    const double iy = ps.RLI[3] * bx + ps.RLI[4] * by + ps.RLI[5] * bz + ps.TLI[1];
    const double iz = ps.RLI[6] * bx + ps.RLI[7] * by + ps.RLI[8] * bz + ps.TLI[2];
    const NoiseArg none = {0.0, 0.0, 0.0};
    double w_unused = 0.0;
    residual_row<false>(ps, 0, bx, by, bz, ix, iy, iz, wx, wy, wz, pa, pbn, pc, pd, o, none, w_unused);
  }
  if (live) flags[pair] = o.sel ? 1 : 0;  // the sticky selection (:989-994, :1004)
  // ---- this workgroup's share of the pose's sums: a row of zeros for a pair that is not selected
  double* mine = sh.row + lane * kRowStride;
#pragma unroll
  for (int c = 0; c < 6; c++) mine[c] = o.h[c];
  mine[6] = o.z;
  mine[7] = fabs(o.z);  // |pd2|: res_last (:1009), the float widened
  const int effect = __popcll(__ballot(o.sel));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the wavefront reads back what its own lanes wrote)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  RefinePartial* out = partials + blockIdx.x;
  if (lane < kTerms) {
    // term t: (a, b) of the upper triangle row by row for t < 21, then (t - 21, z), then |pd2| alone
    int a = 0, b = 0;
    if (lane < 21) {
      int t = lane;
#pragma unroll
      for (int r = 0; r < 5; r++)
        if (a == r && t >= 6 - r) { t -= 6 - r; a = r + 1; }  // row r of the triangle holds 6 - r terms
      b = a + t;
    } else if (lane < 27) {
      a = lane - 21; b = 6;
    } else {
      a = 7; b = 7;
    }
    double sum = 0.0;
    if (lane < 27) {
      for (int j = 0; j < kRefinePairs; j++) sum += sh.row[j * kRowStride + a] * sh.row[j * kRowStride + b];  // lane order
    } else {
      for (int j = 0; j < kRefinePairs; j++) sum += sh.row[j * kRowStride + 7];
    }
    out->s[lane] = sum;
  }
  if (lane == 0) { out->effect_num = effect; out->pad = 0; }
}

// ---- the solve: one wavefront per pose; the step itself on lane 0, its matrices in the wavefront's own LDS
struct SolveShared {
  double G[36], P[36], Pinv[36], K1[36], KG[36], aug[72];
};

// out = A^-1 (6 x 6, row-major) by Gauss-Jordan with row pivoting on [A | I]; a zero pivot leaves NaN / Inf behind, which the caller's
// record then shows.  One lane.
__device__ void inverse6(const double* A, double* out, double* aug) {
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      aug[12 * r + c] = A[6 * r + c];
      aug[12 * r + 6 + c] = r == c ? 1.0 : 0.0;
    }
  for (int k = 0; k < 6; k++) {
    int piv = k;
    double best = fabs(aug[12 * k + k]);
    for (int r = k + 1; r < 6; r++) {
      const double v = fabs(aug[12 * r + k]);
      if (v > best) { best = v; piv = r; }
    }
    if (piv != k)
      for (int c = 0; c < 12; c++) { const double t = aug[12 * k + c]; aug[12 * k + c] = aug[12 * piv + c]; aug[12 * piv + c] = t; }
    const double d = aug[12 * k + k];
    for (int c = 0; c < 12; c++) aug[12 * k + c] /= d;
    for (int r = 0; r < 6; r++) {
      if (r == k) continue;
      const double f = aug[12 * r + k];
      if (f != 0.0)
        for (int c = 0; c < 12; c++) aug[12 * r + c] -= f * aug[12 * k + c];
    }
  }
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) out[6 * r + c] = aug[12 * r + 6 + c];
}

// Exp(v) - so3_math.h:61-79 (identity below 1e-5) - and Log - :100-107
__device__ void so3_exp_dev(const double* v, double* R) {
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  for (int e = 0; e < 9; e++) R[e] = (e % 4 == 0) ? 1.0 : 0.0;
  if (n > 0.00001) {
    const double ax[3] = {v[0] / n, v[1] / n, v[2] / n};
    const double K[9] = {0, -ax[2], ax[1], ax[2], 0, -ax[0], -ax[1], ax[0], 0};
    double cK[9], KK[9];
    const double s = sin(n), c1 = 1.0 - cos(n);
    for (int e = 0; e < 9; e++) cK[e] = c1 * K[e];  // `(1.0 - cos) * K * K` = ((1 - cos) K) K, so3_math.h:73
    mat3_mul(cK, K, KK);
    for (int e = 0; e < 9; e++) R[e] = (R[e] + s * K[e]) + KK[e];
  }
}
__device__ void so3_log_dev(const double* R, double* out) {
  const double tr = R[0] + R[4] + R[8];
  const double theta = (tr > 3.0 - 1e-6) ? 0.0 : acos(0.5 * (tr - 1));
  const double K[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double f = (fabs(theta) < 0.001) ? 0.5 : (0.5 * theta / sin(theta));
  out[0] = f * K[0]; out[1] = f * K[1]; out[2] = f * K[2];
}

constexpr int kSolveWaves = kBlock / 64;  // poses per workgroup of the solve

__device__ void write_record(RefineRecord* o, const double* R, const double* p, const double* P, double total, int effect, int iterations, int searches,
                             int flags) {
  for (int c = 0; c < 9; c++) o->pose[c] = R[c];
  for (int c = 0; c < 3; c++) o->pose[9 + c] = p[c];
  for (int c = 0; c < 36; c++) o->cov[c] = P[c];
  o->total_residual = total;
  o->effect_num = effect;
  o->iterations = iterations;
  o->searches = searches;
  o->flags = flags;
}

__global__ __launch_bounds__(kBlock) void k_refine_solve(const RefinePartial* __restrict__ partials, int chunks, int n_poses, const double* __restrict__ poses,
                                                         RefinePrior prior, int round, int max_iterations, int updates, double rinv,
                                                         RefineCtrl* __restrict__ ctrl, RefineRecord* __restrict__ records) {
  __shared__ SolveShared shared[kSolveWaves];
  const int lane = threadIdx.x & 63;
  const long long pose = (long long)blockIdx.x * kSolveWaves + (threadIdx.x >> 6);
  if (pose >= n_poses) return;  // (the whole wavefront)
  RefineCtrl* ck = ctrl + pose;
  const double* pk = poses + 12 * (size_t)pose;
  if (round == 0) {
    if (!finite12(pk)) {  // returned as given, the counts 0; no later round touches it
      if (lane == 0) {
        ck->done = 1;
        write_record(records + pose, pk, pk + 9, prior.P, 0.0, 0, 0, 0, kRefineBadPose);
      }
      return;
    }
  } else if (ck->done) {
    return;
  }
  // ---- the pose's sums
  const RefinePartial* mine = partials + (size_t)pose * (size_t)chunks;
  double s[kTerms];
#pragma unroll
  for (int t = 0; t < kTerms; t++) s[t] = 0.0;
  int effect = 0;
  for (int c = lane; c < chunks; c += 64) {  // ascending
    const RefinePartial* p = mine + c;
#pragma unroll
    for (int t = 0; t < kTerms; t++) s[t] += p->s[t];
    effect += p->effect_num;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {  // a fixed tree: lane l takes lane l + off
#pragma unroll
    for (int t = 0; t < kTerms; t++) s[t] += __shfl_down(s[t], off);
    effect += __shfl_down(effect, off);
  }
  if (lane != 0) return;
  // ---- the step (lane 0)
  SolveShared& w = shared[threadIdx.x >> 6];
  double R[9], p[3], Rp[9], pp[3];
  int it = 0, rem = 0, upd = 0, iterations = 0, searches = 0, searched = 1;
  if (round == 0) {
    for (int c = 0; c < 9; c++) R[c] = Rp[c] = pk[c];
    for (int c = 0; c < 3; c++) p[c] = pp[c] = pk[9 + c];
    for (int c = 0; c < 36; c++) w.P[c] = prior.P[c];
  } else {
    for (int c = 0; c < 9; c++) { R[c] = ck->R[c]; Rp[c] = ck->Rp[c]; }
    for (int c = 0; c < 3; c++) { p[c] = ck->p[c]; pp[c] = ck->pp[c]; }
    for (int c = 0; c < 36; c++) w.P[c] = ck->P[c];
    it = ck->it; rem = ck->rem; upd = ck->upd; iterations = ck->iterations; searches = ck->searches; searched = ck->search;
  }
  iterations++;
  searches += searched ? 1 : 0;
  // G = R^-1 sum h^T h, g = R^-1 sum h^T z (:1068, :1080)
  double gv[6];
  {
    int t = 0;
    for (int a = 0; a < 6; a++)
      for (int b = a; b < 6; b++, t++) w.G[6 * a + b] = w.G[6 * b + a] = rinv * s[t];
    for (int a = 0; a < 6; a++) gv[a] = rinv * s[21 + a];
  }
  // K_1 = (G + P^-1)^-1 (:1081)
  inverse6(w.P, w.Pinv, w.aug);
  for (int c = 0; c < 36; c++) w.KG[c] = w.G[c] + w.Pinv[c];
  inverse6(w.KG, w.K1, w.aug);
  for (int a = 0; a < 6; a++)
    for (int b = 0; b < 6; b++) {
      double acc = 0.0;
      for (int c = 0; c < 6; c++) acc += w.K1[6 * a + c] * w.G[6 * c + b];
      w.KG[6 * a + b] = acc;
    }
  // vec = state_propagat - state (:1083): Log(R^T R_prop), p_prop - p
  double v[6], RtRp[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) RtRp[3 * r + c] = R[r] * Rp[c] + R[3 + r] * Rp[3 + c] + R[6 + r] * Rp[6 + c];
  so3_log_dev(RtRp, v);
  for (int c = 0; c < 3; c++) v[3 + c] = pp[c] - p[c];
  // solution = K z + vec - K H vec (:1084) with K z = K_1 g and K H = K_1 G
  double sol[6];
  for (int a = 0; a < 6; a++) {
    double kg = 0.0, kgv = 0.0;
    for (int c = 0; c < 6; c++) { kg += w.K1[6 * a + c] * gv[c]; kgv += w.KG[6 * a + c] * v[c]; }
    sol[a] = (kg + v[a]) - kgv;
  }
  // state += solution (:1087)
  double E[9], Rn[9];
  so3_exp_dev(sol, E);
  mat3_mul(R, E, Rn);
  for (int c = 0; c < 9; c++) R[c] = Rn[c];
  for (int c = 0; c < 3; c++) p[c] += sol[3 + c];
  // the schedule (:1093-1133)
  const bool converged = sqrt(sol[0] * sol[0] + sol[1] * sol[1] + sol[2] * sol[2]) * 57.3 < 0.01 &&
                         sqrt(sol[3] * sol[3] + sol[4] * sol[4] + sol[5] * sol[5]) * 100 < 0.015;
  int search_next = 0;
  if (converged || (rem == 0 && it == max_iterations - 2)) { search_next = 1; rem++; }
  int done = 0;
  if (rem >= 2 || it == max_iterations - 1) {
    // state.cov = (I - K H) state.cov (:1114); w.G is free now
    for (int a = 0; a < 6; a++)
      for (int b = 0; b < 6; b++) {
        double acc = 0.0;
        for (int c = 0; c < 6; c++) acc += ((a == c ? 1.0 : 0.0) - w.KG[6 * a + c]) * w.P[6 * c + b];
        w.G[6 * a + b] = acc;
      }
    // ... and leaves as its symmetric part, as the registration path's posterior does (lii_iekf.hip): the next update's gain relies on
    // P = P^T, and a record's cov is a prior the call accepts again
    for (int a = 0; a < 6; a++)
      for (int b = 0; b < 6; b++) w.P[6 * a + b] = 0.5 * (w.G[6 * a + b] + w.G[6 * b + a]);
    upd++;
    if (upd == updates) {
      done = 1;
      write_record(records + pose, R, p, w.P, s[27], effect, iterations, searches, rem >= 2 ? kRefineConverged : 0);
    } else {  // the next update starts where this one ended
      for (int c = 0; c < 9; c++) Rp[c] = R[c];
      for (int c = 0; c < 3; c++) pp[c] = p[c];
      it = 0; rem = 0; search_next = 1;
    }
  } else {
    it++;
  }
  for (int c = 0; c < 9; c++) { ck->R[c] = R[c]; ck->Rp[c] = Rp[c]; }
  for (int c = 0; c < 3; c++) { ck->p[c] = p[c]; ck->pp[c] = pp[c]; }
  for (int c = 0; c < 36; c++) ck->P[c] = w.P[c];
  ck->search = search_next; ck->done = done; ck->rem = rem; ck->it = it; ck->upd = upd; ck->iterations = iterations; ck->searches = searches;
  ck->pad = 0;
}

}  // namespace

size_t pose_refine_partials(int n, int n_poses) { return (size_t)n_poses * (size_t)((n + kRefinePairs - 1) / kRefinePairs); }

void launch_pose_refine(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const float4* body, int n, const PoseArg& base, const RefinePrior& prior,
                        const double* poses_dev, int n_poses, int max_iterations, int updates, int r_max, double plane_thr, double rinv, const RefineScratch& sc,
                        RefineRecord* records, hipStream_t s) {
  if (n <= 0 || n_poses <= 0) return;
  const int chunks = (n + kRefinePairs - 1) / kRefinePairs;
  const size_t blocks = (size_t)n_poses * (size_t)chunks;  // (the caller bounds n_poses * n)
  const unsigned int solve_blocks = (unsigned int)((n_poses + kSolveWaves - 1) / kSolveWaves);
  for (int round = 0; round < updates * max_iterations; round++) {
    // (either form leaves the same partials: which pairs a workgroup holds and how it adds them up do not depend on WAVES)
    if (blocks <= (size_t)kSmallBatchBlocks)
      hipLaunchKernelGGL(k_refine_pass<4>, dim3((unsigned int)blocks), dim3(256), 0, s, g, n_entries, pts_cap, body, n, chunks, base, poses_dev, round, sc.ctrl,
                         r_max, plane_thr, sc.planes, sc.flags, sc.partials);
    else
      hipLaunchKernelGGL(k_refine_pass<1>, dim3((unsigned int)blocks), dim3(64), 0, s, g, n_entries, pts_cap, body, n, chunks, base, poses_dev, round, sc.ctrl,
                         r_max, plane_thr, sc.planes, sc.flags, sc.partials);
    hipLaunchKernelGGL(k_refine_solve, dim3(solve_blocks), dim3(kBlock), 0, s, sc.partials, chunks, n_poses, poses_dev, prior, round, max_iterations, updates,
                       rinv, sc.ctrl, records);
  }
}

}  // namespace lii

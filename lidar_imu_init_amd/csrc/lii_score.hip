// libliinit_hip — the quality figures of one search pass at K candidate poses (lii_pose_score / lii_pose_score_dev).
// Reference: src/laserMapping.cpp:957-1020 - one pass of the per-point loop with nearest_search_en on an all-true selection: pointBodyToWorld
// (:209-220), Nearest_Search (ikd_Tree.cpp:349-379), esti_plane (common_lib.h:236-269), pd2 and the gate s > 0.9 (:999-1001), res_last
// (:987, :1008), effect_feat_num (:1013-1020) and the total_residual of :961 / :1022 the reference declares and never accumulates.
//
// TWO LAUNCHES, whatever K is.  k_pose_score<WAVES>: one workgroup of WAVES wavefronts per 64 consecutive points of one pose.
//   search  every lane forms the world point of pair (threadIdx.x & 63); each wavefront then takes 64 / WAVES of the pairs one after the
//           other through the exact search the map queries use (ring_walk_nearest, lii_ringwalk.h: k = 5, d2 <= max_match_dist2 inclusive) and
//           leaves each list - five points and their d2 - in LDS.  No list ever reaches memory.
//   fit     lane L of the first wavefront fits the plane of pair L with the registration path's own routines (lii_plane.h: canon_ties,
//           fit_plane), forms pd2 and the gate with its float / double mix (lii_fit.hip: residual_row) and writes res_last.  All 64 lanes
//           fit: the ~730 fp64 instructions of a fit are paid once per 64 pairs, not once per pair's wavefront.
//   sum     the counts are popcounts of ballots; the 64 residuals are added by one lane in lane order, in double.
// k_pose_score_final: one wavefront per pose; lane l adds the partials l, l + 64, ... in that order, then a fixed tree over the lanes.
// WAVES: 1 when the launch has workgroups enough to fill the chip, 4 below that (launch_pose_score) - a small batch is one dependent chain
// of searches per wavefront, and four wavefronts cut it to a quarter; a large one loses to the three wavefronts that idle through the fit.
// Which workgroup holds which pairs, and every order of addition, depend on the point's index alone: a pose's figures are the same
// bits wherever it stands in whatever batch.  No atomics.
// Every loop is bounded by a number known before it starts: 64 pairs, the walk's own bounds, 64 terms, the partials of a pose.
#include "lii_launch.h"
#include "lii_plane.h"
#include "lii_ringwalk.h"

namespace lii {
namespace {

constexpr int kScorePairs = 64;  // (pose, point) pairs of a workgroup: one per lane of the wavefront that fits
// (kSmallBatchBlocks - the launch size up to which four wavefronts search a workgroup's pairs: lii_launch.h, shared with lii_refine.hip)

struct ScoreShared {
  float4 nb[kScorePairs][kMatch];  // the list of pair j: xyz, w = d2
  int found[kScorePairs];
  double term[kScorePairs];
};

template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_pose_score(GridView g, unsigned int n_entries, unsigned int pts_cap, const float4* __restrict__ body, int n,
                                                            int chunks, PoseArg ps, const double* __restrict__ poses, int r_max, double plane_thr,
                                                            ScorePartial* __restrict__ partials, float* __restrict__ res) {
  __shared__ ScoreShared sh;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned int pose = blockIdx.x / (unsigned int)chunks, chunk = blockIdx.x - pose * (unsigned int)chunks;
  const int first = (int)chunk * kScorePairs;  // (< n: chunks = ceil(n / 64))
  const int n_here = min(kScorePairs, n - first);
  const bool live = lane < n_here;
  // the base state with rot_end / pos_end replaced by pose k; a NaN or Inf entry: the pose scores nothing
  const double* pk = poses + 12 * (size_t)pose;
  bool pose_ok = true;
#pragma unroll
  for (int c = 0; c < 12; c++) {
    const double v = pk[c];
    pose_ok = pose_ok && fabs(v) <= 1.7976931348623157e308;  // (false for NaN)
    if (c < 9) ps.R[c] = v;
    else ps.p[c - 9] = v;
  }
  const float4 pb = live ? body[first + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
  float wx, wy, wz;
  body_to_world(ps, pb, wx, wy, wz);
  // ---- search: this wavefront's pairs one after the other, the whole wavefront on each (uniform trip count)
  constexpr int kPairsPerWave = kScorePairs / WAVES;
  for (int j = wave * kPairsPerWave; j < (wave + 1) * kPairsPerWave; j++) {
    const float qx = __shfl(wx, j), qy = __shfl(wy, j), qz = __shfl(wz, j);
    float my_d = INFINITY;
    unsigned int my_i = kFree;
    if (pose_ok && j < n_here) ring_walk_nearest(g, n_entries, pts_cap, qx, qy, qz, kMatch, g.max_d2, r_max, my_d, my_i);  // (uniform)
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
  __syncthreads();
  if (wave != 0) return;  // (nothing below waits for the workgroup)
  // ---- fit, gate, res_last: lane L of the first wavefront owns pair L
  bool full = false, sel = false;
  float r_out = -1000.0f;  // (:987)
  if (live && pose_ok) {
    float4 nb[kMatch];
#pragma unroll
    for (int j = 0; j < kMatch; j++) nb[j] = sh.nb[lane][j];
    full = sh.found[lane] == kMatch;
    if (full) canon_ties(nb);
    bool candidate = full && !(nb[4].w > 5.0f);  // (:990)
    double pa = 0, pbn = 0, pc = 0, pd = 0;
    if (candidate) candidate = fit_plane(nb, plane_thr, pa, pbn, pc, pd);
    if (candidate) {
      // (the arithmetic of residual_row, lii_fit.hip)
      const double bx = pb.x, by = pb.y, bz = pb.z;
      const float pd2 = (float)(pa * wx + pbn * wy + pc * wz + pd);
      const double pbnorm = sqrt(bx * bx + by * by + bz * bz);
      const float s = (float)(1 - 0.9 * fabsf(pd2) / sqrt(pbnorm));
      if (s > 0.9) {
        sel = true;
        r_out = fabsf(pd2);
      }
    }
  }
  if (live && res) res[(size_t)pose * (size_t)n + (size_t)(first + lane)] = r_out;
  // ---- this workgroup's share of the pose's figures
  sh.term[lane] = sel ? (double)r_out : 0.0;
  const int n_full = __popcll(__ballot(full)), effect = __popcll(__ballot(sel));
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the wavefront reads back what its own lanes wrote)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (lane == 0) {
    double sum = 0.0;
    for (int j = 0; j < kScorePairs; j++) sum += sh.term[j];  // lane order
    ScorePartial p;
    p.n_full = n_full; p.effect_num = effect; p.total_residual = sum;
    partials[blockIdx.x] = p;
  }
}

constexpr int kFinalWaves = kBlock / 64;  // poses per workgroup of the final pass

__global__ __launch_bounds__(kBlock) void k_pose_score_final(const ScorePartial* __restrict__ partials, int chunks, int n_poses, ScorePartial* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const long long pose = (long long)blockIdx.x * kFinalWaves + (threadIdx.x >> 6);
  if (pose >= n_poses) return;  // (the whole wavefront)
  const ScorePartial* mine = partials + (size_t)pose * (size_t)chunks;
  int n_full = 0, effect = 0;
  double sum = 0.0;
  for (int c = lane; c < chunks; c += 64) {  // ascending
    const ScorePartial p = mine[c];
    n_full += p.n_full; effect += p.effect_num; sum += p.total_residual;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {  // a fixed tree: lane l takes lane l + off
    n_full += __shfl_down(n_full, off);
    effect += __shfl_down(effect, off);
    sum += __shfl_down(sum, off);
  }
  if (lane == 0) {
    ScorePartial out;
    out.n_full = n_full; out.effect_num = effect; out.total_residual = sum;
    scores[pose] = out;
  }
}

}  // namespace

size_t pose_score_partials(int n, int n_poses) { return (size_t)n_poses * (size_t)((n + kScorePairs - 1) / kScorePairs); }

void launch_pose_score(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const float4* body, int n, const PoseArg& base, const double* poses_dev,
                       int n_poses, int r_max, double plane_thr, ScorePartial* partials, ScorePartial* scores, float* res, hipStream_t s) {
  if (n <= 0 || n_poses <= 0) return;
  const int chunks = (n + kScorePairs - 1) / kScorePairs;
  const size_t blocks = (size_t)n_poses * (size_t)chunks;  // (< 2^31 / 64 + 2^16: the caller bounds n_poses * n)
  // (either form leaves the same partials: which pairs a workgroup holds and how it adds them up do not depend on WAVES)
  if (blocks <= (size_t)kSmallBatchBlocks)
    hipLaunchKernelGGL(k_pose_score<4>, dim3((unsigned int)blocks), dim3(256), 0, s, g, n_entries, pts_cap, body, n, chunks, base, poses_dev, r_max, plane_thr,
                       partials, res);
  else
    hipLaunchKernelGGL(k_pose_score<1>, dim3((unsigned int)blocks), dim3(64), 0, s, g, n_entries, pts_cap, body, n, chunks, base, poses_dev, r_max, plane_thr,
                       partials, res);
  hipLaunchKernelGGL(k_pose_score_final, dim3((unsigned int)((n_poses + kFinalWaves - 1) / kFinalWaves)), dim3(kBlock), 0, s, partials, chunks, n_poses, scores);
}

}  // namespace lii

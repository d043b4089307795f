// libliinit_hip — the surface the map holds at a point: normal, curvature and the covariance spectrum of a ball of map points
// (lii_map_surface / lii_map_surface_dev), and their whole-map aggregate, the crispness figures of the calibration literature - mean map
// entropy and mean plane variance (lii_map_crispness).  The reference has no counterpart: PCL's NormalEstimation (computePointNormal,
// flipNormalTowardsViewpoint, "surface variation" as curvature) and the MME / MPV of the LiDAR calibration papers are the models.
//
// ONE WAVEFRONT PER QUERY, on the ball walk of lii_map_radius (ball_walk, lii_ringwalk.h): the acceptance rule is that query's, bit for
// bit - float32 dist2_ref against max_d2, inclusive - so `count` IS the length of the query's lii_map_radius segment.  Where the ball
// query lists a trip's points, this kernel REDUCES them: a lane adds its accepted point to nine double sums of its own,
//   d = (double)m - (double)q per axis,   s1[a] += d_a,   s2[ab] += d_a * d_b   (xx, xy, xz, yy, yz, zz)
// relative to the query, so that nothing cancels at map coordinates of hundreds of metres (|d| <= the ball's radius).  Behind the walk
// one fixed-shape butterfly (wave_sum: DPP inside the rows of 16 lanes, the four row sums through scalars) adds the 64 lanes' sums and
// leaves every lane with the same bits.  Every lane then forms (redundantly; lanes 0 .. 10 store a word of the record each)
//   mean_rel = s1 / n,   C_ab = s2_ab / n - mean_rel_a * mean_rel_b            (no FMA: the unit is compiled with -ffp-contract=off)
// and the eigen-decomposition of C by lii_eig3.h (cyclic Jacobi, a fixed number of sweeps).
// Which lane a point falls to and in which trip depends on the query and the map state alone: a query's record is the same bits alone
// or in any batch.  No atomics, no LDS, no wavefront waits for another; every loop is bounded as in k_map_radius.
//
// The aggregate: the map's live points, gathered as lii_map_download gathers them, are the queries.  k_surface_select flags the points
// with mix(x, y, z) % every == 0 - a hash of the point's float bits, so the selection is a property of the point, not of its slot -, a
// scan ranks them, k_surface_compact lays them end to end.  k_map_surface<true> writes one 24-byte term per selected point instead of
// the record, and k_crispness_reduce - ONE workgroup - adds the terms: thread j takes terms j, j + 1024, ... in that order, then a
// fixed tree over the 1024 partial sums in LDS.  The figures are the same bits on every call for a given map state.
#include "lii_eig3.h"
#include "lii_launch.h"
#include "lii_ringwalk.h"

namespace lii {
namespace {

constexpr int kQueryWaves = kBlock / 64;  // queries per workgroup
constexpr int kReduceThreads = 1024;
// (the kernel stores both records as 64-bit words, one a lane)
static_assert(sizeof(SurfaceRecord) == 88 && offsetof(SurfaceRecord, valid) == 4 && offsetof(SurfaceRecord, mean) == 8 && offsetof(SurfaceRecord, curvature) == 80, "11 words");
static_assert(sizeof(SurfaceTerm) == 24 && offsetof(SurfaceTerm, count) == 16 && offsetof(SurfaceTerm, kind) == 20, "3 words");

struct Viewpoint {
  int on;
  double v[3];
};

// The sum of v over the 64 lanes, the same bits in every lane, in ONE fixed shape: inside each row of 16 lanes a butterfly by DPP moves
// (quad_perm [1,0,3,2] and [2,3,0,1], row_ror:4, row_ror:8 - vector-ALU moves, no trip through the LDS crossbar, which 108 bpermutes a
// query would make the launch's floor), then the four rows' sums as lane 0 of each row holds them, read into scalars and added
// ((r0 + r1) + r2) + r3.  Which additions meet in which order is fixed by the lane numbers alone.
template <int kCtrl>
__device__ __forceinline__ double dpp_take(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, kCtrl, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, kCtrl, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value(double v, int src_lane) {  // (src_lane: a constant)
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src_lane), __builtin_amdgcn_readlane(__double2loint(v), src_lane));
}
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_take<0xB1>(v);   // quad_perm [1,0,3,2]: lane ^ 1
  v += dpp_take<0x4E>(v);   // quad_perm [2,3,0,1]: lane ^ 2
  v += dpp_take<0x124>(v);  // row_ror:4
  v += dpp_take<0x128>(v);  // row_ror:8
  return ((lane_value(v, 0) + lane_value(v, 16)) + lane_value(v, 32)) + lane_value(v, 48);
}

// kTerms: the per-point terms of lii_map_crispness (terms[qi]) instead of the record (out[qi])
template <bool kTerms>
__global__ __launch_bounds__(kBlock) void k_map_surface(GridView g, unsigned int n_entries, unsigned int pts_cap, const char* __restrict__ queries, int n,
                                                        int stride_bytes, float max_d2, int r_max, Viewpoint vp, int min_count,
                                                        SurfaceRecord* __restrict__ out, SurfaceTerm* __restrict__ terms) {
  const int lane = threadIdx.x & 63;
  const long long qi = (long long)blockIdx.x * kQueryWaves + (threadIdx.x >> 6);
  if (qi >= n) return;  // (the whole wavefront)
  const float* qp = reinterpret_cast<const float*>(queries + (size_t)qi * (size_t)stride_bytes);
  const float qx = qp[0], qy = qp[1], qz = qp[2];
  const double qdx = (double)qx, qdy = (double)qy, qdz = (double)qz;
  double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  unsigned int accepted = 0u;
  ball_walk(g, n_entries, pts_cap, qx, qy, qz, max_d2, r_max, true,
            [&](unsigned int, bool, bool in_ball, unsigned long long hits, float mx, float my, float mz, float) {
              if (in_ball) {
                const double dx = (double)mx - qdx, dy = (double)my - qdy, dz = (double)mz - qdz;
                s1x += dx; s1y += dy; s1z += dz;
                sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
                syy += dy * dy; syz += dy * dz; szz += dz * dz;
              }
              accepted += (unsigned int)__popcll(hits);
            });
  s1x = wave_sum(s1x); s1y = wave_sum(s1y); s1z = wave_sum(s1z);
  sxx = wave_sum(sxx); sxy = wave_sum(sxy); sxz = wave_sum(sxz);
  syy = wave_sum(syy); syz = wave_sum(syz); szz = wave_sum(szz);
  // every lane holds the same sums and forms the outputs redundantly (the same instructions a single lane would issue): the record then
  // leaves as ONE store of 11 lanes, a word each, instead of eleven stores of lane 0
  const int count = (int)min(accepted, 0x7FFFFFFFu);
  SurfaceRecord rec;
  rec.count = count;
  rec.valid = count >= 3 ? 1 : 0;
  for (int k = 0; k < 3; k++) { rec.mean[k] = 0.0; rec.eig[k] = 0.0; rec.normal[k] = 0.0; }
  rec.curvature = 0.0;
  if (count > 0) {
    const double nn = (double)count;
    const double mx = s1x / nn, my = s1y / nn, mz = s1z / nn;  // mean_rel
    rec.mean[0] = qdx + mx; rec.mean[1] = qdy + my; rec.mean[2] = qdz + mz;
    if (rec.valid) {
      // C_ab = s2_ab / n - mean_rel_a * mean_rel_b
      const double c6[6] = {sxx / nn - mx * mx, sxy / nn - mx * my, sxz / nn - mx * mz, syy / nn - my * my, syz / nn - my * mz, szz / nn - mz * mz};
      double eig[3], vec[9];
      sym3_eigen(c6, eig, vec);
      for (int k = 0; k < 3; k++) rec.eig[k] = eig[k] < 0.0 ? 0.0 : eig[k];  // (negative rounding residue of a flat or thin ball)
      const double sum = rec.eig[0] + rec.eig[1] + rec.eig[2];
      rec.curvature = sum > 0.0 ? rec.eig[0] / sum : 0.0;
      double nx = vec[0], ny = vec[1], nz = vec[2];
      bool flip;
      if (vp.on) {  // PCL's flipNormalTowardsViewpoint: the normal looks at the viewpoint
        const double dot = nx * (vp.v[0] - rec.mean[0]) + ny * (vp.v[1] - rec.mean[1]) + nz * (vp.v[2] - rec.mean[2]);
        flip = dot < 0.0;
      } else {  // the component of largest magnitude is positive; on a tie the lowest index decides
        double big = nx;
        if (fabs(ny) > fabs(big)) big = ny;
        if (fabs(nz) > fabs(big)) big = nz;
        flip = big < 0.0;
      }
      if (flip) { nx = 0.0 - nx; ny = 0.0 - ny; nz = 0.0 - nz; }
      rec.normal[0] = nx; rec.normal[1] = ny; rec.normal[2] = nz;
    }
  }
  if (kTerms) {
    SurfaceTerm t;
    t.h = 0.0;
    t.eig0 = 0.0;
    t.count = count;
    if (count < min_count) t.kind = kSurfaceSparse;
    else if (rec.eig[0] <= 1e-12 * rec.eig[2]) t.kind = kSurfaceDegenerate;
    else {
      t.kind = kSurfaceUsed;
      t.eig0 = rec.eig[0];
      // the differential entropy of the ball's Gaussian: 0.5 ln((2 pi e)^3 det C); 3 ln(2 pi e) = 8.513631199228035...
      t.h = 0.5 * (8.51363119922803635 + log(rec.eig[0]) + log(rec.eig[1]) + log(rec.eig[2]));
    }
    const unsigned long long tail = (unsigned long long)(unsigned int)t.count | ((unsigned long long)(unsigned int)t.kind << 32);
    const unsigned long long w = lane == 0 ? (unsigned long long)__double_as_longlong(t.h) : lane == 1 ? (unsigned long long)__double_as_longlong(t.eig0) : tail;
    if (lane < 3) reinterpret_cast<unsigned long long*>(terms + qi)[lane] = w;
  } else {
    const unsigned long long head = (unsigned long long)(unsigned int)rec.count | ((unsigned long long)(unsigned int)rec.valid << 32);
    const double v = lane == 1 ? rec.mean[0] : lane == 2 ? rec.mean[1] : lane == 3 ? rec.mean[2] : lane == 4 ? rec.eig[0] : lane == 5 ? rec.eig[1] :
                     lane == 6 ? rec.eig[2] : lane == 7 ? rec.normal[0] : lane == 8 ? rec.normal[1] : lane == 9 ? rec.normal[2] : rec.curvature;
    if (lane < 11) reinterpret_cast<unsigned long long*>(out + qi)[lane] = lane == 0 ? head : (unsigned long long)__double_as_longlong(v);
  }
}

// mix(x, y, z) over the float bits, in uint32 arithmetic
__device__ __forceinline__ unsigned int surface_mix(float x, float y, float z) {
  unsigned int h = __float_as_uint(x) * 0x9E3779B1u ^ __float_as_uint(y) * 0x85EBCA77u ^ __float_as_uint(z) * 0xC2B2AE3Du;
  h ^= h >> 15;
  return h;
}

__global__ __launch_bounds__(kBlock) void k_surface_select(const float4* __restrict__ pts, int n, unsigned int every, unsigned int* __restrict__ flags) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  flags[i] = surface_mix(p.x, p.y, p.z) % every == 0u ? 1u : 0u;
}

// ranks: the inclusive scan of flags; selected point i goes to row ranks[i] - 1 < n
__global__ __launch_bounds__(kBlock) void k_surface_compact(const float4* __restrict__ pts, const unsigned int* __restrict__ flags,
                                                            const unsigned int* __restrict__ ranks, int n, float4* __restrict__ dst) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned int r = ranks[i];
  if (flags[i] && r >= 1u && r <= (unsigned int)n) dst[r - 1u] = pts[i];
}

struct CrispSums {
  double h, e0;
  long long cnt, used, sparse, degenerate;
};
__device__ __forceinline__ void crisp_add(CrispSums& a, const CrispSums& b) {
  a.h += b.h; a.e0 += b.e0; a.cnt += b.cnt; a.used += b.used; a.sparse += b.sparse; a.degenerate += b.degenerate;
}

__global__ __launch_bounds__(kReduceThreads) void k_crispness_reduce(const SurfaceTerm* __restrict__ terms, int n, CrispnessSums* __restrict__ out) {
  __shared__ CrispSums part[kReduceThreads];
  const int j = threadIdx.x;
  CrispSums a = {0.0, 0.0, 0, 0, 0, 0};
  for (int i = j; i < n; i += kReduceThreads) {  // (n is fixed before the loop starts)
    const SurfaceTerm t = terms[i];
    if (t.kind == kSurfaceUsed) { a.h += t.h; a.e0 += t.eig0; a.cnt += t.count; a.used++; }
    else if (t.kind == kSurfaceSparse) a.sparse++;
    else a.degenerate++;
  }
  part[j] = a;
  __syncthreads();
  for (int s = kReduceThreads / 2; s >= 1; s >>= 1) {
    if (j < s) crisp_add(part[j], part[j + s]);
    __syncthreads();
  }
  if (j == 0) {
    const CrispSums t = part[0];
    CrispnessSums o;
    o.n_selected = (long long)n; o.n_used = t.used; o.n_sparse = t.sparse; o.n_degenerate = t.degenerate;
    const double u = (double)t.used;
    o.mme = t.used > 0 ? t.h / u : 0.0;
    o.mpv = t.used > 0 ? t.e0 / u : 0.0;
    o.mean_count = t.used > 0 ? (double)t.cnt / u : 0.0;
    out[0] = o;
  }
}

Viewpoint viewpoint_of(const double* v) {
  Viewpoint vp = {0, {0.0, 0.0, 0.0}};
  if (v) { vp.on = 1; vp.v[0] = v[0]; vp.v[1] = v[1]; vp.v[2] = v[2]; }
  return vp;
}

}  // namespace

void sym3_eigen_host(const double m[6], double eig[3], double vec[9]) { sym3_eigen(m, eig, vec); }

void launch_map_surface(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2, int r_max,
                        const double* viewpoint, SurfaceRecord* out, hipStream_t s) {
  if (n <= 0) return;
  const unsigned int blocks = (unsigned int)(((long long)n + kQueryWaves - 1) / kQueryWaves);
  hipLaunchKernelGGL(k_map_surface<false>, dim3(blocks), dim3(kBlock), 0, s, g, n_entries, pts_cap, static_cast<const char*>(queries), n, stride_bytes, max_d2,
                     r_max, viewpoint_of(viewpoint), 0, out, (SurfaceTerm*)nullptr);
}

void launch_map_surface_terms(const GridView& g, unsigned int n_entries, unsigned int pts_cap, const void* queries, int n, int stride_bytes, float max_d2,
                              int r_max, int min_count, SurfaceTerm* terms, hipStream_t s) {
  if (n <= 0) return;
  const unsigned int blocks = (unsigned int)(((long long)n + kQueryWaves - 1) / kQueryWaves);
  hipLaunchKernelGGL(k_map_surface<true>, dim3(blocks), dim3(kBlock), 0, s, g, n_entries, pts_cap, static_cast<const char*>(queries), n, stride_bytes, max_d2,
                     r_max, viewpoint_of(nullptr), min_count, (SurfaceRecord*)nullptr, terms);
}

void launch_surface_select(const float4* pts, int n, unsigned int every, unsigned int* flags, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_surface_select, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pts, n, every, flags);
}

void launch_surface_compact(const float4* pts, const unsigned int* flags, const unsigned int* ranks, int n, float4* dst, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_surface_compact, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, pts, flags, ranks, n, dst);
}

void launch_crispness_reduce(const SurfaceTerm* terms, int n, CrispnessSums* out, hipStream_t s) {
  hipLaunchKernelGGL(k_crispness_reduce, dim3(1), dim3(kReduceThreads), 0, s, terms, n, out);
}

}  // namespace lii

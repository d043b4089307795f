// Feature extraction on the device (preprocess/feature_extract_en; lii_ingest_set_features), gfx950.  Replaces the feature branches of
//   Preprocess::avia_handler / oust_handler / velodyne_handler   reference src/preprocess.cpp:373-418, :487-536, :585-652
//   Preprocess::give_feature                                     :715-965
//   Preprocess::plane_judge / edge_jump_judge                    :976-1071, :1073-1102
// behind the whole-message ingest's decode (lii_ingest.hip).  Five launches: k_feat_hist -> k_feat_offsets -> k_feat_scatter (the stable
// partition of the kept points by line: a counting scatter over chunks of 256, message order kept within a line), k_feat_lines (one
// workgroup of ONE wavefront per line: range / dista, the four passes, the line's pl_surf / pl_corn into staging at the line's
// offset), k_feat_emit (line-major compaction into the frame and the corner buffer, the frame table).
//
// Inside a line the plane walk is a chain: where group k + 1 starts depends on where group k ended, and the Edge_Plane test on the
// direction before.  The 64 lanes cooperate INSIDE a plane_judge - the search for i_nex by ballot over 64 candidates at a time, the
// maximum cross-product norm, and the three order statistics of disarr (largest, element size / 2, second smallest: selections, exact
// without the reference's O(m^2) exchange sort).  Pass 2 is per point; pass 3 (a firing at i keeps i + 1 from firing) is a parity scan
// over runs of candidates; pass 4 a segmented scan over plane runs; both by ballot, 64 points at a time with a carry.  More wavefronts
// per line would wait for the one that walks.  No workgroup waits on another, every loop is bounded by the line length.
//
// Arithmetic: every decision is an IEEE add / mul / div / sqrt in the reference's types and order (float where it computes in float,
// double in plane_judge and pass 2, float in the emission mean); the file is built without FMA contraction like the rest of the library.
// Defined here where the reference reads memory nobody wrote or runs off an array (include/liinit_hip.h): disB = 0,
// types[plsize - 1].dista = 0, a line blind throughout or empty yields nothing, vecs[j] beside a blind neighbour is the zero vector, a
// plane group that runs off the end of its line marks the points the line has.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/liinit_hip.h"
#include "lii_feature.h"

namespace lii {

namespace {

enum : uint8_t { kNor = 0, kPossPlane = 1, kRealPlane = 2, kEdgeJump = 3, kEdgePlane = 4, kWire = 5 };  // Feature, src/preprocess.h:12
enum { kNrNor = 0, kNrZero = 1, kNr180 = 2, kNrInf = 3, kNrBlind = 4 };                                  // E_jump, :14

constexpr int kChunk = 256;  // kept points per workgroup of the partition by line
constexpr int kGroupSize = 8;
constexpr double kDisA = 0.1, kDisB = 0.0;  // (:15-16 sets disA twice; disB is whatever the object's memory held: 0 here)
constexpr double kInfBound = 10, kP2lRatio = 225;
constexpr double kLimitMaxMid = 6.25, kLimitMidMin = 6.25, kLimitMaxMin = 3.24;
constexpr double kEdgeA = 2, kEdgeB = 0.1, kSmallpRatio = 1.2;

__device__ __forceinline__ double sq3(double a, double b, double c) {  // a * a + b * b + c * c, left to right
  return __dadd_rn(__dadd_rn(__dmul_rn(a, a), __dmul_rn(b, b)), __dmul_rn(c, c));
}
__device__ __forceinline__ double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}
__device__ __forceinline__ double dsub(float a, float b) { return (double)__fsub_rn(a, b); }  // float difference, widened (vx = pl[a].x - pl[b].x)
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

struct LineView {
  const float4* P;
  const double* rng;
  const double* dista;
  double* inter;
  uint8_t* F;
  int m;
  double blind;
};

// edge_jump_judge (:1073-1102)
__device__ bool edge_jump_judge(const LineView& L, int i, int nor_dir) {
  if (nor_dir == 0) {
    if (L.rng[i - 1] < L.blind || L.rng[i - 2] < L.blind) return false;
  } else {
    if (L.rng[i + 1] < L.blind || L.rng[i + 2] < L.blind) return false;
  }
  double d1 = L.dista[i + nor_dir - 1];
  double d2 = L.dista[i + 3 * nor_dir - 2];
  if (d1 < d2) { const double d = d1; d1 = d2; d2 = d; }
  d1 = __dsqrt_rn(d1);
  d2 = __dsqrt_rn(d2);
  if (d1 > __dmul_rn(kEdgeA, d2) || __dsub_rn(d1, d2) > kEdgeB) return false;
  return true;
}

// The stable partition of the kept points by line, a counting scatter in three launches.  A chunk is 256 consecutive kept points.
// (1) lines of a chunk's points, counted in LDS (integer atomics: the counts do not depend on their order)
__global__ __launch_bounds__(kChunk) void k_feat_hist(const uint8_t* __restrict__ line_of_raw, const unsigned int* __restrict__ kept_idx,
                                                      const unsigned int* __restrict__ rank, int n, int* __restrict__ hist) {
  __shared__ int s_cnt[kMaxLines];
  const int tid = threadIdx.x;
  if (tid < kMaxLines) s_cnt[tid] = 0;
  __syncthreads();
  const int kept = n > 0 ? (int)min(rank[n - 1], (unsigned int)n) : 0;
  const int r = blockIdx.x * kChunk + tid;
  if (r < kept) {
    const unsigned int i = kept_idx[r];
    if (i < (unsigned int)n) {
      const int l = line_of_raw[i];
      if (l < kMaxLines) atomicAdd(&s_cnt[l], 1);
    }
  }
  __syncthreads();
  if (tid < kMaxLines) hist[blockIdx.x * kMaxLines + tid] = s_cnt[tid];
}
// (2) one wavefront per line: the exclusive prefix of the line's counts over the chunks (in place), the line's length
__global__ __launch_bounds__(64) void k_feat_offsets(int* __restrict__ hist, int n_chunks, int* __restrict__ per_line) {
  const int L = blockIdx.x, lane = threadIdx.x;
  int total = 0;
  for (int c0 = 0; c0 < n_chunks; c0 += 64) {
    const int c = c0 + lane;
    const int v = c < n_chunks ? hist[c * kMaxLines + L] : 0;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    if (c < n_chunks) hist[c * kMaxLines + L] = total + incl - v;
    total += __shfl(incl, 63);
  }
  if (lane == 0) {
    per_line[L] = total;
    per_line[kMaxLines + L] = 0;
    per_line[2 * kMaxLines + L] = 0;
    per_line[3 * kMaxLines + L] = 0;
  }
}
// (3) kept point r -> its line's segment, at (points of the line in the chunks before) + (points of the line before it in its chunk)
__global__ __launch_bounds__(kChunk) void k_feat_scatter(const float4* __restrict__ pts, const uint8_t* __restrict__ line_of_raw,
                                                         const unsigned int* __restrict__ kept_idx, const unsigned int* __restrict__ rank, int n,
                                                         int n_lines, const int* __restrict__ hist, const int* __restrict__ per_line,
                                                         float4* __restrict__ lp, unsigned int* __restrict__ lidx) {
  __shared__ int s_line[kChunk], s_off[kMaxLines];
  const int tid = threadIdx.x;
  const int kept = n > 0 ? (int)min(rank[n - 1], (unsigned int)n) : 0;
  const int r = blockIdx.x * kChunk + tid;
  int l = -1;
  unsigned int i = 0;
  if (r < kept) {
    i = kept_idx[r];
    if (i < (unsigned int)n && line_of_raw[i] < n_lines) l = line_of_raw[i];
  }
  s_line[tid] = l;
  if (tid == 0) {
    int o = 0;
    for (int k = 0; k < n_lines; k++) { s_off[k] = o; o += per_line[k]; }
  }
  __syncthreads();
  if (l < 0) return;
  int before = 0;
  for (int j = 0; j < tid; j++) before += s_line[j] == l ? 1 : 0;
  const int pos = s_off[l] + hist[blockIdx.x * kMaxLines + l] + before;
  if (pos < kept) {
    lp[pos] = pts[i];
    lidx[pos] = i;
  }
}

// one wavefront per line
__global__ __launch_bounds__(64) void k_feat_lines(FeatureParams fp, const unsigned int* __restrict__ rank, int n, float4* lp, unsigned int* lidx, double* rng_all, double* dista_all, double* inter_all,
                                                   uint8_t* ftype_all, uint8_t* fire_all, float4* __restrict__ surf_stage,
                                                   float4* __restrict__ corn_stage, unsigned int* __restrict__ corn_sidx, int* per_line) {
  const int Lno = blockIdx.x, lane = threadIdx.x;
  const int kept = n > 0 ? (int)min(rank[n - 1], (unsigned int)n) : 0;
  int off = 0;
  for (int l = 0; l < Lno; l++) off += per_line[l];
  const int m = per_line[Lno];
  if (off + m > kept || m <= 0) return;  // (the partition's counts: never beyond the kept points)
  float4* P = lp + off;
  unsigned int* PI = lidx + off;
  double* rng = rng_all + off;
  double* dista = dista_all + off;
  double* inter = inter_all + off;
  uint8_t* F = ftype_all + off;
  uint8_t* fire = fire_all + off;
  const bool avia = fp.lidar_type == LII_LIDAR_AVIA;
  const double blind = fp.blind;

  // (avia_handler :399, velodyne_handler :638; oust_handler does not skip, an empty line never gets here)
  if ((avia && m <= 5) || (fp.lidar_type == LII_LIDAR_VELO && m < 2)) return;
  if (lane == 0) per_line[3 * kMaxLines + Lno] = 1;

  // range / dista (:406-413, :527-534, :643-650); orgtype's constructor
  for (int j = lane; j < m; j += 64) {
    const float4 p = P[j];
    const float r2 = __fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y));
    rng[j] = avia ? (double)r2 : (double)__fsqrt_rn(r2);
    double d = 0.0;  // (types[plsize - 1].dista is never written there: 0 here)
    if (j + 1 < m) {
      const float4 q = P[j + 1];
      d = sq3(dsub(p.x, q.x), dsub(p.y, q.y), dsub(p.z, q.z));
    }
    dista[j] = d;
    inter[j] = 2.0;
    F[j] = kNor;
    fire[j] = 0;
  }
  __syncthreads();

  // head (:724-726); a line blind throughout yields nothing
  int head = -1;
  for (int j0 = 0; j0 < m && head < 0; j0 += 64) {
    const int j = j0 + lane;
    const unsigned long long mk = __ballot(j < m && !(rng[j] < blind));
    if (mk) head = j0 + __ffsll((long long)mk) - 1;
  }
  if (head < 0) return;
  LineView LV{P, rng, dista, inter, F, m, blind};

  // ---- 1. the plane walk (:729-825); every variable of the walk is the same in all lanes
  {
    const int plsize2 = m > kGroupSize ? m - kGroupSize : 0;
    int last_state = 0;
    double ldx = 0, ldy = 0, ldz = 0;
    int i = head;
    while (i < plsize2) {
      if (rng[i] < blind) { i++; continue; }
      // plane_judge(i) (:976-1071)
      const float4 c = P[i];
      double group_dis = __dadd_rn(__dmul_rn(kDisA, rng[i]), kDisB);
      group_dis = __dmul_rn(group_dis, group_dis);
      int type = -1, i_nex = i;
      double vx = 0, vy = 0, vz = 0, two_dis = 0;
      {
        const unsigned long long mk = __ballot(lane < kGroupSize && rng[i + lane] < blind);  // (i + 8 <= m - 1)
        if (mk) { type = 2; i_nex = i + __ffsll((long long)mk) - 1; }
      }
      if (type < 0) {
        bool found = false;
        for (int b0 = i + kGroupSize; b0 < m; b0 += 64) {
          const int j = b0 + lane;
          bool bl = false, st = false;
          double ax = 0, ay = 0, az = 0, t2 = 0;
          if (j < m) {
            const float4 q = P[j];
            ax = dsub(q.x, c.x); ay = dsub(q.y, c.y); az = dsub(q.z, c.z);
            t2 = sq3(ax, ay, az);
            bl = rng[j] < blind;
            st = t2 >= group_dis;
          }
          const unsigned long long mk = __ballot(bl || st);
          if (mk) {
            const int f = __ffsll((long long)mk) - 1;
            i_nex = b0 + f;
            if (__shfl((int)bl, f)) type = 2;
            vx = __shfl(ax, f); vy = __shfl(ay, f); vz = __shfl(az, f); two_dis = __shfl(t2, f);
            found = true;
            break;
          }
        }
        if (!found) {  // ran off the line: vx, vy, vz, two_dis are those of its last point
          i_nex = m;
          const float4 q = P[m - 1];
          vx = dsub(q.x, c.x); vy = dsub(q.y, c.y); vz = dsub(q.z, c.z);
          two_dis = sq3(vx, vy, vz);
        }
      }
      if (type < 0) {
        double leng_wid = 0;
        const int hi = min(i_nex, m);
        for (int j = i + 1 + lane; j < hi; j += 64) {
          const float4 q = P[j];
          const double v10 = dsub(q.x, c.x), v11 = dsub(q.y, c.y), v12 = dsub(q.z, c.z);
          const double v20 = __dsub_rn(__dmul_rn(v11, vz), __dmul_rn(vy, v12));
          const double v21 = __dsub_rn(__dmul_rn(v12, vx), __dmul_rn(v10, vz));
          const double v22 = __dsub_rn(__dmul_rn(v10, vy), __dmul_rn(vx, v11));
          const double lw = sq3(v20, v21, v22);
          if (lw > leng_wid) leng_wid = lw;
        }
        for (int o = 32; o >= 1; o >>= 1) {
          const double other = __shfl_xor(leng_wid, o);
          if (other > leng_wid) leng_wid = other;
        }
        if (__ddiv_rn(__dmul_rn(two_dis, two_dis), leng_wid) < kP2lRatio) type = 0;
      }
      if (type < 0) {
        // disarr = dista[i .. i_nex - 1] sorted in descending order: [0], [size / 2], [size - 2]
        const int cnt = i_nex - i;
        const double* D = dista + i;
        double mn1 = INFINITY, mn2 = INFINITY, mx = -INFINITY;
        for (int j = lane; j < cnt; j += 64) {
          const double d = D[j];
          if (d > mx) mx = d;
          if (d < mn1) { mn2 = mn1; mn1 = d; }
          else if (d < mn2) mn2 = d;
        }
        for (int o = 32; o >= 1; o >>= 1) {
          const double omx = __shfl_xor(mx, o), o1 = __shfl_xor(mn1, o), o2 = __shfl_xor(mn2, o);
          if (omx > mx) mx = omx;
          const double lo = fmin(mn1, o1), hi1 = fmax(mn1, o1);
          mn2 = fmin(hi1, fmin(mn2, o2));
          mn1 = lo;
        }
        if (mn2 < 1e-16) {
          type = 0;
        } else if (avia) {
          const int k0 = cnt / 2;
          double mid = 0;
          for (int j0 = 0; j0 < cnt; j0 += 64) {
            const int j = j0 + lane;
            const double v = j < cnt ? D[j] : 0.0;
            int gt = 0, ge = 0;
            for (int k = 0; k < cnt; k++) {
              const double d = D[k];
              gt += d > v ? 1 : 0;
              ge += d >= v ? 1 : 0;
            }
            const unsigned long long mk = __ballot(j < cnt && gt <= k0 && k0 < ge);
            if (mk) { mid = __shfl(v, __ffsll((long long)mk) - 1); break; }
          }
          if (__ddiv_rn(mx, mid) >= kLimitMaxMid || __ddiv_rn(mid, mn2) >= kLimitMidMin) type = 0;
        } else if (__ddiv_rn(mx, mn2) >= kLimitMaxMin) {
          type = 0;
        }
      }
      double cdx = 0, cdy = 0, cdz = 0;
      if (type < 0) {
        type = 1;
        const double nrm = __dsqrt_rn(sq3(vx, vy, vz));
        cdx = __ddiv_rn(vx, nrm); cdy = __ddiv_rn(vy, nrm); cdz = __ddiv_rn(vz, nrm);
      }
      if (type == 1) {
        uint8_t at_i = kPossPlane;
        if (last_state == 1 && __dsqrt_rn(sq3(ldx, ldy, ldz)) > 0.1) {
          const double mod = dot3(ldx, ldy, ldz, cdx, cdy, cdz);
          at_i = (mod > -0.707 && mod < 0.707) ? kEdgePlane : kRealPlane;
        }
        for (int j = i + lane; j <= i_nex && j < m; j += 64) F[j] = j == i ? at_i : (j == i_nex ? kPossPlane : kRealPlane);
        __syncthreads();  // (the next group's first point is this one's last: its mark comes second)
        i = i_nex - 1;
        last_state = 1;
      } else {
        i = i_nex;
        last_state = 0;
      }
      ldx = cdx; ldy = cdy; ldz = cdz;
      i++;
    }
  }
  __syncthreads();

  // ---- 2. edge jumps and wires (:827-895), per point
  {
    const int plsize2 = m > 3 ? m - 3 : 0;
    for (int i = head + 3 + lane; i < plsize2; i += 64) {
      if (rng[i] < blind || F[i] >= kRealPlane) continue;
      if (dista[i - 1] < 1e-16 || dista[i] < 1e-16) continue;
      const float4 pa = P[i];
      const double a0 = pa.x, a1 = pa.y, a2 = pa.z;
      int edj[2] = {kNrNor, kNrNor};
      double v[2][3] = {{0, 0, 0}, {0, 0, 0}};  // (unset beside a blind neighbour there: the zero vector here)
      for (int j = 0; j < 2; j++) {
        const int mm = j == 0 ? -1 : 1;
        if (rng[i + mm] < blind) {
          edj[j] = rng[i] > kInfBound ? kNrInf : kNrBlind;
          continue;
        }
        const float4 q = P[i + mm];
        v[j][0] = __dsub_rn((double)q.x, a0); v[j][1] = __dsub_rn((double)q.y, a1); v[j][2] = __dsub_rn((double)q.z, a2);
        const double angle = __ddiv_rn(__ddiv_rn(dot3(a0, a1, a2, v[j][0], v[j][1], v[j][2]), __dsqrt_rn(sq3(a0, a1, a2))),
                                       __dsqrt_rn(sq3(v[j][0], v[j][1], v[j][2])));
        if (angle < fp.jump_up_limit) edj[j] = kNr180;
        else if (angle > fp.jump_down_limit) edj[j] = kNrZero;
      }
      const double isect = __ddiv_rn(__ddiv_rn(dot3(v[0][0], v[0][1], v[0][2], v[1][0], v[1][1], v[1][2]), __dsqrt_rn(sq3(v[0][0], v[0][1], v[0][2]))),
                                     __dsqrt_rn(sq3(v[1][0], v[1][1], v[1][2])));
      inter[i] = isect;
      const double dp = dista[i - 1], dc = dista[i];
      if (edj[0] == kNrNor && edj[1] == kNrZero && dc > 0.0225 && dc > __dmul_rn(4.0, dp)) {
        if (isect > fp.cos160 && edge_jump_judge(LV, i, 0)) F[i] = kEdgeJump;
      } else if (edj[0] == kNrZero && edj[1] == kNrNor && dp > 0.0225 && dp > __dmul_rn(4.0, dc)) {
        if (isect > fp.cos160 && edge_jump_judge(LV, i, 1)) F[i] = kEdgeJump;
      } else if (edj[0] == kNrNor && edj[1] == kNrInf) {
        if (edge_jump_judge(LV, i, 0)) F[i] = kEdgeJump;
      } else if (edj[0] == kNrInf && edj[1] == kNrNor) {
        if (edge_jump_judge(LV, i, 1)) F[i] = kEdgeJump;
      } else if (edj[0] > kNrNor && edj[1] > kNrNor) {
        if (F[i] == kNor) F[i] = kWire;
      }
    }
  }
  __syncthreads();

  // ---- 3. small planes (:897-925): point i fires when it is a candidate and i - 1 did not fire (a firing turns i + 1 into
  // Real_Plane) - inside a run of candidates every second one, counted from the run's start
  {
    int prev_fired = 0;  // did the last point of the chunk before fire
    for (int j0 = head + 1; j0 < m - 1; j0 += 64) {
      const int i = j0 + lane;
      bool cand = false;
      if (i < m - 1 && !(rng[i] < blind || rng[i - 1] < blind || rng[i + 1] < blind) && !(dista[i - 1] < 1e-8 || dista[i] < 1e-8) &&
          F[i] == kNor) {
        const double dp = dista[i - 1], dc = dista[i];
        const double ratio = dp > dc ? __ddiv_rn(dp, dc) : __ddiv_rn(dc, dp);
        cand = inter[i] < fp.smallp_intersect && ratio < kSmallpRatio;
      }
      const unsigned long long mk = __ballot(cand);
      const unsigned long long gaps = ~mk & lanes_below(lane);  // non-candidates below this lane
      bool fires = false;
      if (cand) {
        if (gaps) fires = ((lane - (63 - __clzll((long long)gaps)) - 1) & 1) == 0;
        else fires = ((lane & 1) == 0) != (prev_fired != 0);
      }
      if (fires) fire[i] = 1;
      prev_fired = __shfl((int)fires, 63);
    }
    __syncthreads();
    for (int j = lane; j < m; j += 64)
      if (F[j] == kNor && (fire[j] || (j > 0 && fire[j - 1]) || (j + 1 < m && fire[j + 1]))) F[j] = kRealPlane;
  }
  __syncthreads();

  // ---- 4. emission (:927-964): inside a run of plane points every pfn-th one; at the first point behind a run the float mean of the
  // unfinished remainder; a remainder that reaches the end of the line is lost
  {
    const int pfn = fp.pfn;
    int carry = 0;  // length of the plane run that ends at the chunk's last point
    int n_surf = 0, n_corn = 0;
    for (int j0 = head; j0 < m; j0 += 64) {
      const int j = j0 + lane;
      const bool valid = j < m;
      const uint8_t f = valid ? F[j] : (uint8_t)kNor;
      const bool plane = valid && (f == kPossPlane || f == kRealPlane);
      const unsigned long long pm = __ballot(plane);
      const unsigned long long gaps = ~pm & lanes_below(lane);
      int run_incl = 0;  // points of the run up to and including this one
      if (plane) run_incl = gaps ? lane - (63 - __clzll((long long)gaps)) : lane + carry + 1;
      int before = __shfl_up(run_incl, 1);
      if (lane == 0) before = carry;
      bool emit = false;
      float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
      if (plane) {
        if (run_incl % pfn == 0) {
          emit = true;
          const float4 p = P[j];
          out = make_float4(p.x, p.y, p.z, p.w);
        }
      } else if (valid) {
        const int r = before % pfn;
        if (r != 0) {
          emit = true;
          float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
          for (int k = j - r; k < j; k++) {
            const float4 p = P[k];
            sx = __fadd_rn(sx, p.x); sy = __fadd_rn(sy, p.y); sz = __fadd_rn(sz, p.z); sw = __fadd_rn(sw, p.w);
          }
          const float cnt = (float)(unsigned int)r;
          out = make_float4(__fdiv_rn(sx, cnt), __fdiv_rn(sy, cnt), __fdiv_rn(sz, cnt), __fdiv_rn(sw, cnt));
        }
      }
      const bool corner = valid && (f == kEdgeJump || f == kEdgePlane);
      const unsigned long long em = __ballot(emit), cm = __ballot(corner);
      if (emit) surf_stage[off + n_surf + __popcll(em & lanes_below(lane))] = out;
      if (corner) {
        const int at = off + n_corn + __popcll(cm & lanes_below(lane));
        corn_stage[at] = P[j];
        corn_sidx[at] = PI[j];
      }
      n_surf += __popcll(em);
      n_corn += __popcll(cm);
      carry = __shfl(run_incl, 63);
    }
    if (lane == 0) {
      per_line[kMaxLines + Lno] = n_surf;
      per_line[2 * kMaxLines + Lno] = n_corn;
    }
  }
}

template <class T>
__device__ __forceinline__ T rd(const uint8_t* p) {
  T v;
  memcpy(&v, p, sizeof(T));
  return v;
}

// pl_surf / pl_corn: lines ascending, positions ascending within a line; the frame table (one frame, stamped with the message's time)
__global__ __launch_bounds__(256) void k_feat_emit(const int* __restrict__ per_line, int n_lines, int n, const float4* __restrict__ surf_stage,
                                                   const float4* __restrict__ corn_stage, const unsigned int* __restrict__ corn_sidx,
                                                   const uint8_t* __restrict__ raw, int int_step, int int_off, int int_kind, double stamp_ms,
                                                   float4* __restrict__ frames, float4* __restrict__ corn, float* __restrict__ corn_int,
                                                   IngestTable* __restrict__ dev, IngestTable* __restrict__ host) {
  __shared__ int s_off[kMaxLines + 1], s_surf[kMaxLines + 1], s_corn[kMaxLines + 1], s_ran;
  if (threadIdx.x == 0) {
    int o = 0, a = 0, b = 0, ran = 0;
    for (int l = 0; l < n_lines; l++) {
      s_off[l] = o; s_surf[l] = a; s_corn[l] = b;
      o += per_line[l]; a += per_line[kMaxLines + l]; b += per_line[2 * kMaxLines + l]; ran += per_line[3 * kMaxLines + l];
    }
    s_off[n_lines] = o; s_surf[n_lines] = a; s_corn[n_lines] = b;
    s_ran = ran;
  }
  __syncthreads();
  const int n_surf = min(s_surf[n_lines], n), n_corn = min(s_corn[n_lines], n);
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_surf) {
    int l = 0;
    while (l + 1 < n_lines && r >= s_surf[l + 1]) l++;
    frames[r] = surf_stage[s_off[l] + (r - s_surf[l])];
  }
  if (r < n_corn) {
    int l = 0;
    while (l + 1 < n_lines && r >= s_corn[l + 1]) l++;
    const int at = s_off[l] + (r - s_corn[l]);
    corn[r] = corn_stage[at];
    float v = 0.f;
    const unsigned int i = corn_sidx[at];
    if (int_kind != 2 && i < (unsigned int)n) {
      const uint8_t* p = raw + (size_t)i * int_step + int_off;
      v = int_kind == 0 ? rd<float>(p) : (float)rd<uint8_t>(p);
    }
    corn_int[r] = v;
  }
  if (r == 0) {
    IngestTable t;
    t.n_kept = n_surf;
    t.n_frames = n_surf > 0 ? 1 : 0;  // (an empty cloud is skipped by the node: laserMapping.cpp:909-914)
    t.n_emitted = n_surf;
    t.unsorted = 0;
    t.first[0] = 1;
    t.last[0] = n_surf;
    t.begin_ms[0] = stamp_ms;
    t.delta[0] = 0.0;
    double tail = 0.0;
    if (n_surf > 0) {
      int l = 0;
      while (l + 1 < n_lines && n_surf - 1 >= s_surf[l + 1]) l++;
      tail = (double)surf_stage[s_off[l] + (n_surf - 1 - s_surf[l])].w;  // points.back().curvature (sync_packages, laserMapping.cpp:452-456)
    }
    t.tail_ms[0] = tail;
    t.n_corn = n_corn;
    t.n_feat_lines = s_ran;
    *dev = t;
    *host = t;
  }
}

}  // namespace

FeatureParams feature_params_default() {
  FeatureParams p{};
  // src/preprocess.cpp:30-33
  p.jump_up_limit = cos(170.0 / 180 * M_PI);
  p.jump_down_limit = cos(8.0 / 180 * M_PI);
  p.cos160 = cos(160.0 / 180 * M_PI);
  p.smallp_intersect = cos(172.5 / 180 * M_PI);
  return p;
}

hipError_t feature_reserve(FeatureBufs* fb, size_t cap) {
  if (fb->cap() >= cap && fb->d_line) return hipSuccess;
  fb->d_lp.reset(); fb->d_lidx.reset(); fb->d_range.reset(); fb->d_dista.reset(); fb->d_inter.reset(); fb->d_ftype.reset(); fb->d_fire.reset();
  fb->d_surf_stage.reset(); fb->d_corn_stage.reset(); fb->d_corn_sidx.reset(); fb->d_corn.reset(); fb->d_corn_int.reset(); fb->d_line.reset(); fb->d_hist.reset();
  hipError_t e;
  if ((e = fb->d_lidx.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_range.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_dista.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_inter.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_ftype.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_fire.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_surf_stage.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_corn_stage.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_corn_sidx.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_corn.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_corn_int.alloc(cap)) != hipSuccess) return e;
  if ((e = fb->d_line.alloc(4 * kMaxLines)) != hipSuccess) return e;
  if ((e = fb->d_hist.alloc((cap / kChunk + 2) * kMaxLines)) != hipSuccess) return e;
  return fb->d_lp.alloc(cap);  // (the one whose size() stands for all of them comes last)
}

void feature_launch(const FeatureBufs& fb, const FeatureParams& p, const float4* pts, const uint8_t* line_of_raw, const unsigned int* kept_idx,
                    const unsigned int* rank, int n, const uint8_t* raw, int int_step, int int_off, int int_kind, double stamp_ms,
                    float4* frames, IngestTable* dev_tab, IngestTable* host_tab, hipStream_t s) {
  const int lines = p.n_scans;
  const int n_chunks = (n + kChunk - 1) / kChunk;
  hipLaunchKernelGGL(k_feat_hist, dim3(n_chunks), dim3(kChunk), 0, s, line_of_raw, kept_idx, rank, n, fb.d_hist.get());
  hipLaunchKernelGGL(k_feat_offsets, dim3(lines), dim3(64), 0, s, fb.d_hist.get(), n_chunks, fb.d_line.get());
  hipLaunchKernelGGL(k_feat_scatter, dim3(n_chunks), dim3(kChunk), 0, s, pts, line_of_raw, kept_idx, rank, n, lines, fb.d_hist.get(), fb.d_line.get(),
                     fb.d_lp.get(), fb.d_lidx.get());
  hipLaunchKernelGGL(k_feat_lines, dim3(lines), dim3(64), 0, s, p, rank, n, fb.d_lp.get(), fb.d_lidx.get(),
                     fb.d_range.get(), fb.d_dista.get(), fb.d_inter.get(), fb.d_ftype.get(), fb.d_fire.get(), fb.d_surf_stage.get(),
                     fb.d_corn_stage.get(), fb.d_corn_sidx.get(), fb.d_line.get());
  hipLaunchKernelGGL(k_feat_emit, dim3((n + 255) / 256), dim3(256), 0, s, fb.d_line.get(), lines, n, fb.d_surf_stage.get(), fb.d_corn_stage.get(),
                     fb.d_corn_sidx.get(), raw, int_step, int_off, int_kind, stamp_ms, frames, fb.d_corn.get(), fb.d_corn_int.get(), dev_tab, host_tab);
}

}  // namespace lii

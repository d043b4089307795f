// LI_Init::LI_Initialization (include/LI_init/LI_init.cpp:586-632) resident on the device: lii_li_init_resident uploads the accumulated
// states once and enqueues a fixed sequence of launches; the host waits once, at the end.
//   k_res_interp_filter / _search / _compact  downsample_interpolate_IMU :82-125 (interpolate = 1; they return at their head otherwise)
//   k_res_head         IMU_time_compensate(0.0, true) :195-221
//   k_res_zero_phase   zero_phase_filt :260-315 of the IMU / LiDAR pair, 24 channels in one workgroup
//   k_res_mid          normalize_acc :494-504, set_IMU_state / set_Lidar_state :27-33, cut_sequence_tail :223-238, the |omega| series and
//                      their running means of xcorr_temporal_init :160-167
//   k_res_xcorr / k_res_argmax   xcorr_temporal_init :168-193 (the device functions of k_xcorr / k_xcorr_argmax, lii_li_init_dev.h)
//   k_res_after_lag    IMU_time_compensate(time_lag_1, false), central_diff :127-158
//   k_res_zero_phase   the second filter; set_states_2nd_filter :35-41 takes ang_acc (both) and the LiDAR's linear_acc from it
//   k_calib_lm<1>, <2> solve_Rotation_only :317-343, solve_Rot_bias_gyro :345-401
//   k_res_stage3_prep  IMU_time_compensate(time_lag_2, false) :395, acc_interpolate :240-258; time_lag_2 is read in device memory
//   k_calib_lm<3>      solve_trans_biasacc_grav :403-492
// VIEWS.  The host chain (lii_li_init.cpp) erases from the front and pops from the back; here the sequences stay where the upload put
// them and ResCtl {ib, lb, n} - start of the IMU view, start of the LiDAR view, their common length - moves.  A launch reads the
// control block at its head, returns there when `status` is set, and its grid is sized by the input length.
// BITS.  Every kernel restates the host function operation for operation (this unit is built with -ffp-contract=off like its
// neighbours); where the host walks a sequence in order - the running means, acc_interpolate's use of the element it has just
// updated - one lane walks it here, over tiles the workgroup stages in LDS.  The zero-phase filter forms the FIR half
// sum_j x[i - j] B[j] (from 0, j ascending) in parallel over i into LDS and keeps the recursive half acc -= y[i - j] A[j] (j = 1 .. 6)
// in six registers of one lane per channel: the additions and their order are butter()'s.
// k_calib_lm restates minimize() of lii_calib.cpp (the trust-region loop Ceres documents) on lane 0 of one workgroup, between calls
// of calib_eval_block - the evaluator k_calib_eval runs.  An accepted candidate is not evaluated a second time: the evaluation that
// priced it is the evaluation at the new point (same parameters, same buffers, same bits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "lii_context.h"
#include "lii_li_init_dev.h"

namespace lii {
namespace {

constexpr int kExt = 60, kNb = 7;
constexpr double kG = 9.81;
__constant__ double r_B[7] = {0.000076, 0.000457, 0.001143, 0.001524, 0.0011, 0.000457, 0.000076};
__constant__ double r_A[7] = {1.0000, -4.182389, 7.491611, -7.313596, 4.089349, -1.238525, 0.158428};

enum ResStatus : int {
  kResOk = 0,
  kResFilter61 = 1,   // fewer than 61 aligned states left to filter (lii_li_init_run's refusal)
  kResAligned200 = 2, // fewer than 200 states after interpolation (lii_li_init_run: n < 200)
  kResRaw6 = 3,       // fewer than 6 raw IMU states behind move_start_time - 3 s (lii_li_init_interpolate)
  kResAlign = 4       // an alignment ran off the end of the LiDAR sequence (the host chain would read an empty sequence)
};

struct ResCtl {
  int ib, lb, n, status;
  int lag, n_aligned, n12, n3;
  int ib12, lb12, ka, kl;
  int pad[4];
  double lag1;
  double means[2];
  double spare;
};
static_assert(sizeof(ResCtl) == 96, "ResCtl layout");
struct ResOut {
  lii_calib_result res;
  double params[3][24];
  int termination[4];
};
constexpr int kSmallDoubles = int((sizeof(ResCtl) + sizeof(ResOut) + 7) / 8);

// first index in [0, count) for which pred holds, else count - what a host `while (k < count && !pred(k)) k++` leaves.  A workgroup of 256.
template <class P>
__device__ int block_find_first(int count, int* s_first, P pred) {
  if (threadIdx.x == 0) *s_first = count;
  __syncthreads();
  for (int i = threadIdx.x; i < count; i += 256)
    if (pred(i)) { atomicMin(s_first, i); break; }
  __syncthreads();
  const int r = *s_first;
  __syncthreads();
  return r;
}

// align() of lii_li_init.cpp:38-46 on views: imu_ts(i) / lid_ts(i) = the stamps of the views' element i (ni / nl of them).
// Returns false when the LiDAR view has no element left (the host would read the front of an empty sequence).
template <class TI, class TL>
__device__ bool align_views(int& ib, int& ni, int& lb, int& nl, int* s_first, TI imu_ts, TL lid_ts) {
  const double t0 = imu_ts(0);
  const int li = block_find_first(nl, s_first, [&](int i) { return !(lid_ts(i) < t0); });
  if (li >= nl) return false;
  const double tl = lid_ts(li);
  const int ii = block_find_first(ni - 1, s_first, [&](int i) { return !(tl > imu_ts(i + 1)); });
  ib += ii; ni -= ii;
  lb += li; nl -= li;
  const int n = min(ni, nl);
  ni = nl = n;
  return true;
}

// ------------------------------------------------------------------------------------------------ downsample_interpolate_IMU
// every workgroup finds the first raw IMU state not older than move_start_time - 3 s (ka) for itself; workgroup 0 leaves ka / kl in the
// control block.  facc[i] = the 5-tap running mean of the accelerations (raw at the two ends), ts[i] = the stamp.
__device__ __forceinline__ void d_res_interp_filter(ResCtl* __restrict__ ctl, int interpolate, const double* __restrict__ raw, int n_imu,
                                                    const double* __restrict__ lid, int n_lid, double mst, double* __restrict__ facc,
                                                    double* __restrict__ ts, int bx) {
  if (!interpolate) return;
  __shared__ int s_first;
  const double t_min = mst - 3.0;
  const int ka = block_find_first(n_imu, &s_first, [&](int i) { return !(raw[(size_t)i * 22 + 21] < t_min); });
  const int size = n_imu - ka;
  if (bx == 0) {
    const int kl = block_find_first(n_lid, &s_first, [&](int i) { return !(lid[(size_t)i * 22 + 21] < t_min); });
    if (threadIdx.x == 0) {
      ctl->ka = ka;
      ctl->kl = kl;
      if (size < 6) ctl->status = kResRaw6;
    }
  }
  const int i = bx * 256 + threadIdx.x;
  if (i >= n_imu) return;
  ts[i] = raw[(size_t)i * 22 + 21];
  const int r = i - ka;
  double acc[3] = {raw[(size_t)i * 22 + 18], raw[(size_t)i * 22 + 19], raw[(size_t)i * 22 + 20]};
  if (r >= 2 && r + 2 < size) {
    acc[0] = acc[1] = acc[2] = 0;
    for (int d = -2; d <= 2; d++)
      for (int a = 0; a < 3; a++) acc[a] += (raw[(size_t)(i + d) * 22 + 18 + a] - acc[a]) / (d + 3);
  }
  for (int a = 0; a < 3; a++) facc[(size_t)i * 3 + a] = acc[a];
}
__global__ __launch_bounds__(256) void k_res_interp_filter(ResCtl* __restrict__ ctl, int interpolate, const double* __restrict__ raw,
                                                           int n_imu, const double* __restrict__ lid, int n_lid, double mst,
                                                           double* __restrict__ facc, double* __restrict__ ts) {
  d_res_interp_filter(ctl, interpolate, raw, n_imu, lid, n_lid, mst, facc, ts, blockIdx.x);
}
// one workgroup per LiDAR state: the first j in ascending order with all[j - 1].t <= t < all[j].t, 256 candidates per step
__device__ __forceinline__ void d_res_interp_search(const ResCtl* __restrict__ ctl, int interpolate, const double* __restrict__ ts, int n_imu,
                                                    const double* __restrict__ lid, int* __restrict__ found, int bx) {
  if (!interpolate || ctl->status) return;
  __shared__ int s_first;
  const int l = bx, ka = ctl->ka, size = n_imu - ka;
  if (l < ctl->kl) {
    if (threadIdx.x == 0) found[l] = -1;
    return;
  }
  const double t = lid[(size_t)l * 22 + 21];
  const double* all = ts + ka;
  if (threadIdx.x == 0) s_first = size;
  __syncthreads();
  int hit = size;
  for (int j0 = 1; j0 < size; j0 += 256) {  // (bounded by the input length; ends at the first step that holds a hit)
    const int j = j0 + threadIdx.x;
    if (j < size && all[j - 1] <= t && all[j] > t) atomicMin(&s_first, j);
    __syncthreads();
    hit = s_first;
    __syncthreads();
    if (hit < size) break;
  }
  if (threadIdx.x == 0) found[l] = hit < size ? ka + hit : -1;
}
__global__ __launch_bounds__(256) void k_res_interp_search(const ResCtl* __restrict__ ctl, int interpolate, const double* __restrict__ ts,
                                                           int n_imu, const double* __restrict__ lid, int* __restrict__ found) {
  d_res_interp_search(ctl, interpolate, ts, n_imu, lid, found, blockIdx.x);
}
// the retained states in their order -> the aligned sequences; one workgroup walks the LiDAR states 256 at a time
__device__ __forceinline__ void d_res_interp_compact(ResCtl* __restrict__ ctl, int interpolate, const double* __restrict__ raw,
                                                     const double* __restrict__ facc, const double* __restrict__ raw_lid,
                                                     const int* __restrict__ found, int n_lid, double* __restrict__ imu,
                                                     double* __restrict__ lid) {
  if (!interpolate || ctl->status) return;
  __shared__ int s_scan[256];
  __shared__ int s_base;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int l0 = 0; l0 < n_lid; l0 += 256) {
    const int l = l0 + threadIdx.x;
    const int j = l < n_lid ? found[l] : -1;
    s_scan[threadIdx.x] = j >= 0 ? 1 : 0;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
      const int v = (int)threadIdx.x >= s ? s_scan[threadIdx.x - s] : 0;
      __syncthreads();
      s_scan[threadIdx.x] += v;
      __syncthreads();
    }
    const int base = s_base;
    if (j >= 0) {
      const int at = base + s_scan[threadIdx.x] - 1;
      const double* P = raw + (size_t)(j - 1) * 22;
      const double* Q = raw + (size_t)j * 22;
      const double* L = raw_lid + (size_t)l * 22;
      const double s = (Q[21] - L[21]) / (Q[21] - P[21]);
      double* o = imu + (size_t)at * 22;
      for (int e = 0; e < 22; e++) o[e] = 0.0;
      o[0] = o[4] = o[8] = 1.0;
      for (int a = 0; a < 3; a++) {
        o[9 + a] = s * P[9 + a] + (1 - s) * Q[9 + a];
        o[18 + a] = s * facc[(size_t)(j - 1) * 3 + a] + (1 - s) * facc[(size_t)j * 3 + a];
      }
      o[21] = L[21];
      double* ol = lid + (size_t)at * 22;
      for (int e = 0; e < 22; e++) ol[e] = L[e];
    }
    __syncthreads();
    if (threadIdx.x == 255) s_base = base + s_scan[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ctl->n_aligned = s_base;
    if (s_base < 200) ctl->status = kResAligned200;
  }
}
__global__ __launch_bounds__(256) void k_res_interp_compact(ResCtl* __restrict__ ctl, int interpolate, const double* __restrict__ raw,
                                                            const double* __restrict__ facc, const double* __restrict__ raw_lid,
                                                            const int* __restrict__ found, int n_lid, double* __restrict__ imu,
                                                            double* __restrict__ lid) {
  d_res_interp_compact(ctl, interpolate, raw, facc, raw_lid, found, n_lid, imu, lid);
}

// ------------------------------------------------------------------------------------------------ the chain
// IMU_time_compensate(0.0, true): discard ten pairs, (stamps - 0.0: unchanged), align
__device__ __forceinline__ void d_res_head(ResCtl* __restrict__ ctl, int interpolate, int n_in, const double* __restrict__ imu,
                                           const double* __restrict__ lid) {
  __shared__ int s_first;
  if (ctl->status) return;
  const int n0 = interpolate ? ctl->n_aligned : n_in;
  int ib = 10, lb = 10, ni = n0 - 10, nl = n0 - 10;
  const bool ok = align_views(ib, ni, lb, nl, &s_first, [&](int i) { return imu[(size_t)(ib + i) * 22 + 21]; },
                              [&](int i) { return lid[(size_t)(lb + i) * 22 + 21]; });
  if (threadIdx.x == 0) {
    ctl->n_aligned = n0;
    ctl->ib = ib; ctl->lb = lb; ctl->n = ni;
    if (!ok) ctl->status = kResAlign;
  }
}
__global__ __launch_bounds__(256) void k_res_head(ResCtl* __restrict__ ctl, int interpolate, int n_in, const double* __restrict__ imu,
                                                  const double* __restrict__ lid) {
  d_res_head(ctl, interpolate, n_in, imu, lid);
}

// zero_phase_filt of the pair: channel c < 12 is member 9 + c of the IMU records, c >= 12 member 9 + c - 12 of the LiDAR records.
// Pass 0 filters the view into tmp (24 doubles per state, time-reversed), pass 1 filters tmp back into the view, reversed again;
// only the channels of `mask` are written back (the second filter: set_states_2nd_filter).  Tiles of kTile padded samples: all lanes
// form the FIR half into LDS, lanes 0 .. 23 run the recursion over the tile, all lanes store it.
constexpr int kTile = 256, kTilePitch = 25;
__device__ __forceinline__ void d_res_zero_phase(ResCtl* __restrict__ ctl, double* __restrict__ imu, double* __restrict__ lid,
                                                 double* __restrict__ tmp, unsigned int mask) {
  __shared__ double s_f[kTile * kTilePitch];
  if (ctl->status) return;
  const int n = ctl->n;
  if (n < 61) {  // butter()'s 60-sample reflection reads in[60] and in[n - 61]
    if (threadIdx.x == 0) ctl->status = kResFilter61;
    return;
  }
  double* base_i = imu + (size_t)ctl->ib * 22 + 9;
  double* base_l = lid + (size_t)ctl->lb * 22 + 9;
  const int m = n + 2 * kExt;
  const int t = threadIdx.x;
  const double a1 = r_A[1], a2 = r_A[2], a3 = r_A[3], a4 = r_A[4], a5 = r_A[5], a6 = r_A[6];
  for (int pass = 0; pass < 2; pass++) {
    // logical sample k of channel c as this pass reads it
    auto in_at = [&](int c, int k) -> double {
      if (pass == 1) return tmp[(size_t)k * 24 + c];
      return c < 12 ? base_i[(size_t)k * 22 + c] : base_l[(size_t)k * 22 + (c - 12)];
    };
    // padded sample i: in[60], ..., in[1], in[0 .. n), in[n - 2], ..., in[n - 61]
    auto x_at = [&](int c, int i) -> double {
      const int k = i < kExt ? kExt - i : (i < kExt + n ? i - kExt : n - 2 - (i - kExt - n));
      return in_at(c, k);
    };
    double y1 = 0, y2 = 0, y3 = 0, y4 = 0, y5 = 0, y6 = 0;  // y[i - 1] .. y[i - 6]; y = x below index 7
    if (t < 24) { y1 = x_at(t, 6); y2 = x_at(t, 5); y3 = x_at(t, 4); y4 = x_at(t, 3); y5 = x_at(t, 2); y6 = x_at(t, 1); }
    for (int i0 = kNb; i0 < m - kExt; i0 += kTile) {
      const int cnt = min(kTile, m - kExt - i0);
      for (int e = t; e < cnt * 24; e += 256) {
        const int c = e % 24, tt = e / 24, i = i0 + tt;
        double acc = 0;
#pragma unroll
        for (int j = 0; j < kNb; j++) acc += x_at(c, i - j) * r_B[j];
        s_f[tt * kTilePitch + c] = acc;
      }
      __syncthreads();
      if (t < 24) {
        // eight steps at a time: their FIR halves come out of LDS together, in front of the dependent chain, and go back behind it
        auto step = [&](double acc) {
          acc -= y1 * a1;
          acc -= y2 * a2;
          acc -= y3 * a3;
          acc -= y4 * a4;
          acc -= y5 * a5;
          acc -= y6 * a6;
          y6 = y5; y5 = y4; y4 = y3; y3 = y2; y2 = y1; y1 = acc;
          return acc;
        };
        int tt = 0;
        for (; tt + 8 <= cnt; tt += 8) {
          double f[8];
#pragma unroll
          for (int u = 0; u < 8; u++) f[u] = s_f[(tt + u) * kTilePitch + t];
#pragma unroll
          for (int u = 0; u < 8; u++) f[u] = step(f[u]);
#pragma unroll
          for (int u = 0; u < 8; u++) s_f[(tt + u) * kTilePitch + t] = f[u];
        }
        for (; tt < cnt; tt++) s_f[tt * kTilePitch + t] = step(s_f[tt * kTilePitch + t]);
      }
      __syncthreads();
      for (int e = t; e < cnt * 24; e += 256) {
        const int c = e % 24, tt = e / 24, i = i0 + tt;
        if (i < kExt) continue;  // the front padding
        const int o = n - 1 - (i - kExt);  // stored time-reversed
        const double v = s_f[tt * kTilePitch + c];
        if (pass == 0) tmp[(size_t)o * 24 + c] = v;
        else if ((mask >> c) & 1u) {
          if (c < 12) base_i[(size_t)o * 22 + c] = v;
          else base_l[(size_t)o * 22 + (c - 12)] = v;
        }
      }
      __syncthreads();
    }
  }
}
__global__ __launch_bounds__(256) void k_res_zero_phase(ResCtl* __restrict__ ctl, double* __restrict__ imu, double* __restrict__ lid,
                                                        double* __restrict__ tmp, unsigned int mask) {
  d_res_zero_phase(ctl, imu, lid, tmp, mask);
}

// normalize_acc; set_IMU_state / set_Lidar_state drop the last element; cut_sequence_tail; a[i] = |w_imu|, b[i] = |w_lidar| of the
// view that is left and their running means, as the host forms them: one lane each, over tiles in LDS
constexpr int kMeanTile = 1024;
__device__ __forceinline__ void d_res_mid(ResCtl* __restrict__ ctl, double* __restrict__ imu, const double* __restrict__ lid,
                                          double* __restrict__ a, double* __restrict__ b) {
  __shared__ int s_first;
  __shared__ double s_nrm;
  __shared__ double s_a[kMeanTile], s_b[kMeanTile];
  if (ctl->status) return;
  int ib = ctl->ib, lb = ctl->lb, n = ctl->n;
  if (threadIdx.x == 0) {
    double mean[3] = {0, 0, 0};
    for (int i = 1; i < 10; i++)
      for (int k = 0; k < 3; k++) mean[k] += (imu[(size_t)(ib + i) * 22 + 18 + k] - mean[k]) / i;
    s_nrm = sqrt(mean[0] * mean[0] + mean[1] * mean[1] + mean[2] * mean[2]);
  }
  __syncthreads();
  const double nrm = s_nrm;
  for (int i = threadIdx.x; i < n; i += 256)
    for (int k = 0; k < 3; k++) {
      double* p = imu + (size_t)(ib + i) * 22 + 18 + k;
      *p = *p / nrm * kG;
    }
  __syncthreads();
  int ni = n - 1 - 20, nl = n - 1 - 20;  // the dropped last element, the tail cut of 20 (n >= 61)
  const bool ok = align_views(ib, ni, lb, nl, &s_first, [&](int i) { return imu[(size_t)(ib + i) * 22 + 21]; },
                              [&](int i) { return lid[(size_t)(lb + i) * 22 + 21]; });
  if (!ok) {
    if (threadIdx.x == 0) ctl->status = kResAlign;
    return;
  }
  n = ni;
  double mean = 0;  // lane 0: ma, lane 1: mb
  for (int i0 = 0; i0 < n; i0 += kMeanTile) {
    const int cnt = min(kMeanTile, n - i0);
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const double va = norm3_at(imu + (size_t)(ib + i0 + i) * 22), vb = norm3_at(lid + (size_t)(lb + i0 + i) * 22);
      s_a[i] = va; s_b[i] = vb;
      a[i0 + i] = va; b[i0 + i] = vb;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      const double* s = threadIdx.x == 0 ? s_a : s_b;
      for (int i = 0; i < cnt; i++) mean += (s[i] - mean) / (i0 + i + 1);
    }
    __syncthreads();
  }
  if (threadIdx.x < 2) ctl->means[threadIdx.x] = mean;
  if (threadIdx.x == 0) { ctl->ib = ib; ctl->lb = lb; ctl->n = n; }
}
__global__ __launch_bounds__(256) void k_res_mid(ResCtl* __restrict__ ctl, double* __restrict__ imu, const double* __restrict__ lid,
                                                 double* __restrict__ a, double* __restrict__ b) {
  d_res_mid(ctl, imu, lid, a, b);
}

__global__ __launch_bounds__(256) void k_res_xcorr(const ResCtl* __restrict__ ctl, const double* __restrict__ a, const double* __restrict__ b,
                                                   double* __restrict__ corr) {
  if (ctl->status) return;
  xcorr_lane(a, b, ctl->means, ctl->n, corr, blockIdx.x * 256 + threadIdx.x);
}
__global__ __launch_bounds__(256) void k_res_argmax(ResCtl* __restrict__ ctl, const double* __restrict__ corr) {
  __shared__ double s_v[256];
  __shared__ int s_k[256];
  if (ctl->status) return;
  xcorr_argmax_block(corr, ctl->n, &ctl->lag, s_v, s_k);
}

// time_lag_1 = lag / (orig_odom_freq * cut_frame_num); IMU_time_compensate(time_lag_1, false); central_diff
__device__ __forceinline__ void d_res_after_lag(ResCtl* __restrict__ ctl, double* __restrict__ imu, double* __restrict__ lid, int freq_cut) {
  __shared__ int s_first;
  if (ctl->status) return;
  int ib = ctl->ib, lb = ctl->lb, n = ctl->n;
  const double lag1 = double(ctl->lag) / double(freq_cut);
  for (int i = threadIdx.x; i + 1 < n; i += 256) imu[(size_t)(ib + i) * 22 + 21] -= lag1;  // the last stamp is spared
  __syncthreads();
  int ni = n, nl = n;
  const bool ok = align_views(ib, ni, lb, nl, &s_first, [&](int i) { return imu[(size_t)(ib + i) * 22 + 21]; },
                              [&](int i) { return lid[(size_t)(lb + i) * 22 + 21]; });
  if (!ok) {
    if (threadIdx.x == 0) { ctl->status = kResAlign; ctl->lag1 = lag1; }
    return;
  }
  n = ni;
  double* I = imu + (size_t)ib * 22;
  double* L = lid + (size_t)lb * 22;
  for (int i = 1 + threadIdx.x; i <= n - 3; i += 256) {  // reads ang_vel / linear_vel / stamps, writes ang_acc / linear_acc
    const double dti = I[(size_t)(i + 1) * 22 + 21] - I[(size_t)(i - 1) * 22 + 21];
    const double dtl = L[(size_t)(i + 1) * 22 + 21] - L[(size_t)(i - 1) * 22 + 21];
    for (int k = 0; k < 3; k++) {
      I[(size_t)i * 22 + 15 + k] = (I[(size_t)(i + 1) * 22 + 9 + k] - I[(size_t)(i - 1) * 22 + 9 + k]) / dti;
      L[(size_t)i * 22 + 15 + k] = (L[(size_t)(i + 1) * 22 + 9 + k] - L[(size_t)(i - 1) * 22 + 9 + k]) / dtl;
      L[(size_t)i * 22 + 18 + k] = (L[(size_t)(i + 1) * 22 + 12 + k] - L[(size_t)(i - 1) * 22 + 12 + k]) / dtl;
    }
  }
  if (threadIdx.x == 0) {
    ctl->ib = ib; ctl->lb = lb; ctl->n = n;
    ctl->ib12 = ib; ctl->lb12 = lb; ctl->n12 = n;
    ctl->lag1 = lag1;
  }
}
__global__ __launch_bounds__(256) void k_res_after_lag(ResCtl* __restrict__ ctl, double* __restrict__ imu, double* __restrict__ lid, int freq_cut) {
  d_res_after_lag(ctl, imu, lid, freq_cut);
}

// IMU_time_compensate(time_lag_2, false) and acc_interpolate, out of place: the stage 1/2 view stays as it is (lii_li_init_resident_fetch),
// the stage-3 sequences are written from index 0 of imu3 / lid3 and copied into the handle's calibration buffers.
constexpr int kAccTile = 512;
template <bool CAL>  // CAL: the copies into the handle's calibration buffers (the batched form leaves them alone)
__device__ __forceinline__ void d_res_stage3_prep(ResCtl* __restrict__ ctl, const ResOut* __restrict__ ro, const double* __restrict__ imu,
                                                  const double* __restrict__ lid, double* __restrict__ imu3, double* __restrict__ lid3,
                                                  double* __restrict__ cal_imu, double* __restrict__ cal_lid) {
  __shared__ int s_first;
  __shared__ double s_ti[kAccTile + 1], s_tl[kAccTile], s_acc[3][kAccTile + 1];
  __shared__ double s_s[kAccTile], s_nt[kAccTile], s_v[3][kAccTile], s_prev[4];
  __shared__ int s_chain[kAccTile];
  if (ctl->status) return;
  const int ib0 = ctl->ib, lb0 = ctl->lb, n0 = ctl->n;
  const double lag2 = ro->res.time_lag_2;
  auto ts_comp = [&](int k) {  // stamp of element k of the stage 1/2 view after `timestamp -= lag` (the last one is spared)
    const double t = imu[(size_t)(ib0 + k) * 22 + 21];
    return k + 1 < n0 ? t - lag2 : t;
  };
  int ib = ib0, lb = lb0, ni = n0, nl = n0;
  const bool ok = align_views(ib, ni, lb, nl, &s_first, [&](int i) { return ts_comp(ib - ib0 + i); },
                              [&](int i) { return lid[(size_t)(lb + i) * 22 + 21]; });
  if (!ok) {
    if (threadIdx.x == 0) ctl->status = kResAlign;
    return;
  }
  const int n = ni;
  for (int e = threadIdx.x; e < n * 22; e += 256) {
    const int i = e / 22, f = e % 22;
    imu3[e] = f == 21 ? ts_comp(ib - ib0 + i) : imu[(size_t)(ib + i) * 22 + f];
    lid3[e] = lid[(size_t)(lb + i) * 22 + f];
  }
  __syncthreads();
  // acc_interpolate: i = 1 .. n - 2 in order.  Step i reads element i + 1 as it was and, where d <= 0, element i - 1 as step i - 1 left
  // it.  Only the acceleration of that branch is a chain: the stamp step i - 1 leaves is t[i - 1] + d[i - 1], whatever came before.  So
  // all lanes form d, s, the new stamp and either the finished value (d > 0) or the addend (1 - s) a[i] (d <= 0) of a tile; then one
  // lane per axis walks the tile with  s * previous + addend  - the host's products and sum, in the host's order.
  for (int i0 = 1; i0 + 1 < n; i0 += kAccTile) {
    const int cnt = min(kAccTile, n - 1 - i0);  // steps i0 .. i0 + cnt - 1; element i0 + cnt is read only
    for (int i = threadIdx.x; i <= cnt; i += 256) {
      s_ti[i] = imu3[(size_t)(i0 + i) * 22 + 21];
      for (int k = 0; k < 3; k++) s_acc[k][i] = imu3[(size_t)(i0 + i) * 22 + 18 + k];
      if (i < cnt) s_tl[i] = lid3[(size_t)(i0 + i) * 22 + 21];
    }
    if (threadIdx.x < 4) s_prev[threadIdx.x] = imu3[(size_t)(i0 - 1) * 22 + 18 + threadIdx.x];  // element i0 - 1 as it stands: acc[3], stamp
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += 256) {
      const double d = s_tl[i] - s_ti[i];
      double sc, v[3];
      if (d > 0) {
        sc = d / (s_ti[i + 1] - s_ti[i]);
        for (int k = 0; k < 3; k++) v[k] = sc * s_acc[k][i + 1] + (1 - sc) * s_acc[k][i];
      } else {
        const double p_t = i == 0 ? s_prev[3] : s_ti[i - 1] + (s_tl[i - 1] - s_ti[i - 1]);
        sc = -d / (s_ti[i] - p_t);
        for (int k = 0; k < 3; k++) v[k] = (1 - sc) * s_acc[k][i];
      }
      s_chain[i] = d > 0 ? 0 : 1;
      s_s[i] = sc;
      s_nt[i] = s_ti[i] + d;
      for (int k = 0; k < 3; k++) s_v[k][i] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int k = threadIdx.x;
      double prev = s_prev[k];
      auto step = [&](int chain, double sc, double v) {
        prev = chain ? sc * prev + v : v;
        return prev;
      };
      int i = 0;
      for (; i + 8 <= cnt; i += 8) {  // eight steps' operands out of LDS in front of the dependent chain
        double sc[8], v[8];
        int ch[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { ch[u] = s_chain[i + u]; sc[u] = s_s[i + u]; v[u] = s_v[k][i + u]; }
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = step(ch[u], sc[u], v[u]);
#pragma unroll
        for (int u = 0; u < 8; u++) s_v[k][i + u] = v[u];
      }
      for (; i < cnt; i++) s_v[k][i] = step(s_chain[i], s_s[i], s_v[k][i]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += 256) {
      imu3[(size_t)(i0 + i) * 22 + 21] = s_nt[i];
      for (int k = 0; k < 3; k++) imu3[(size_t)(i0 + i) * 22 + 18 + k] = s_v[k][i];
    }
    __syncthreads();
  }
  if (CAL)
    for (int e = threadIdx.x; e < n * 22; e += 256) {
      cal_imu[e] = imu3[e];
      cal_lid[e] = lid3[e];
    }
  if (threadIdx.x == 0) ctl->n3 = n;
}
__global__ __launch_bounds__(256) void k_res_stage3_prep(ResCtl* __restrict__ ctl, const ResOut* __restrict__ ro, const double* __restrict__ imu,
                                                         const double* __restrict__ lid, double* __restrict__ imu3, double* __restrict__ lid3,
                                                         double* __restrict__ cal_imu, double* __restrict__ cal_lid) {
  d_res_stage3_prep<true>(ctl, ro, imu, lid, imu3, lid3, cal_imu, cal_lid);
}

// ------------------------------------------------------------------------------------------------ the Levenberg-Marquardt of lii_calib.cpp
struct LmQuat { double w, x, y, z; };
struct LmProblem {
  int stage, dof;
  LmQuat q;
  double v[6];
  double R_LI[9];
  double lo[6], hi[6];
  int bounded[6];
};
struct LmWork {
  LmProblem p, cand;
  double JtJ[81], g[9], cost, scale[9], diag[9];
  double radius, decrease_factor, x_norm, model_change;
  int iter, invalid, reuse_diag, started, term;
};

__device__ void lm_quat_to_rot(const LmQuat& q, double* R) {  // Eigen::Quaternion::toRotationMatrix
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
__device__ LmQuat lm_rot_to_quat(const double* m) {  // Eigen::Quaternion(Matrix3) (Shoemake)
  LmQuat q;
  double t = m[0] + m[4] + m[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (m[7] - m[5]) * t; q.y = (m[2] - m[6]) * t; q.z = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > m[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
    double v[3];
    v[i] = 0.5 * t;
    t = 0.5 / t;
    q.w = (m[3 * k + j] - m[3 * j + k]) * t;
    v[j] = (m[3 * j + i] + m[3 * i + j]) * t;
    v[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    q.x = v[0]; q.y = v[1]; q.z = v[2];
  }
  return q;
}
__device__ LmQuat lm_quat_plus(const LmQuat& q, const double* d) {  // ceres::QuaternionParameterization::Plus
  const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (n <= 0.0) return q;
  const double s = sin(n) / n;
  const double a = cos(n), b = s * d[0], c = s * d[1], e = s * d[2];
  LmQuat r;  // (a,b,c,e) (x) q
  r.w = a * q.w - b * q.x - c * q.y - e * q.z;
  r.x = a * q.x + b * q.w + c * q.z - e * q.y;
  r.y = a * q.y - b * q.z + c * q.w + e * q.x;
  r.z = a * q.z + b * q.y - c * q.x + e * q.w;
  return r;
}
__device__ void lm_plus(const LmProblem& p, const double* delta, LmProblem& c) {
  const LmQuat q = lm_quat_plus(p.q, delta);
  const int nv = p.dof - 3;
  double v[6];
  for (int i = 0; i < nv; i++) {
    double x = p.v[i] + delta[3 + i];
    if (p.bounded[i]) x = fmin(fmax(x, p.lo[i]), p.hi[i]);  // ParameterBlock::Plus projects onto the box
    v[i] = x;
  }
  if (&c != &p) c = p;
  c.q = q;
  for (int i = 0; i < nv; i++) c.v[i] = v[i];
}
__device__ double lm_ambient_norm(const LmProblem& p) {
  double s = p.q.w * p.q.w + p.q.x * p.q.x + p.q.y * p.q.y + p.q.z * p.q.z;
  for (int i = 0; i < p.dof - 3; i++) s += p.v[i] * p.v[i];
  return sqrt(s);
}
__device__ double lm_ambient_dist(const LmProblem& a, const LmProblem& b) {
  double s = (a.q.w - b.q.w) * (a.q.w - b.q.w) + (a.q.x - b.q.x) * (a.q.x - b.q.x) + (a.q.y - b.q.y) * (a.q.y - b.q.y) +
             (a.q.z - b.q.z) * (a.q.z - b.q.z);
  for (int i = 0; i < a.dof - 3; i++) s += (a.v[i] - b.v[i]) * (a.v[i] - b.v[i]);
  return sqrt(s);
}
// max-norm of the projected gradient step  x - Plus(x, -g)  (Ceres' gradient_max_norm); `c` is scratch
__device__ double lm_gradient_max_norm(const LmProblem& p, const double* g, LmProblem& c) {
  double neg[9];
  for (int i = 0; i < p.dof; i++) neg[i] = -g[i];
  lm_plus(p, neg, c);
  double m = fmax(fmax(fabs(p.q.w - c.q.w), fabs(p.q.x - c.q.x)), fmax(fabs(p.q.y - c.q.y), fabs(p.q.z - c.q.z)));
  for (int i = 0; i < p.dof - 3; i++) m = fmax(m, fabs(p.v[i] - c.v[i]));
  return m;
}
// lii::spd_solve of lii_hostmath.h (Cholesky, n <= 9 here)
__device__ bool lm_spd_solve(const double* A, const double* b, int n, double* x) {
  double L[81], y[9];
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      double s = A[i * n + j];
      for (int k = 0; k < j; k++) s -= L[i * n + k] * L[j * n + k];
      if (i == j) {
        if (s <= 0) return false;
        L[i * n + i] = sqrt(s);
      } else {
        L[i * n + j] = s / L[j * n + j];
      }
    }
  for (int i = 0; i < n; i++) {
    double s = b[i];
    for (int k = 0; k < i; k++) s -= L[i * n + k] * y[k];
    y[i] = s / L[i * n + i];
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < n; k++) s -= L[k * n + i] * x[k];
    x[i] = s / L[i * n + i];
  }
  return true;
}
// the parameter vector of lii_calib_eval for the point p (eval() of lii_calib.cpp)
__device__ void lm_params(const LmProblem& p, double* params) {
  lm_quat_to_rot(p.q, params);
  if (p.stage == 2) {
    for (int i = 0; i < 4; i++) params[9 + i] = p.v[i];
  } else if (p.stage == 3) {
    for (int i = 0; i < 6; i++) params[9 + i] = p.v[i];
    for (int i = 0; i < 9; i++) params[15 + i] = p.R_LI[i];
  }
}
// an evaluation becomes the current J^T J / g / cost.  The device tangent is R <- Exp(delta) R; Ceres' quaternion tangent doubles the
// angle: the three rotation columns are scaled by 2.
__device__ void lm_take(LmWork& w, const double* out) {
  const int n = w.p.dof;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const double s = ((i < 3) ? 2.0 : 1.0) * ((j < 3) ? 2.0 : 1.0);
      w.JtJ[i * n + j] = out[i * n + j] * s;
    }
  for (int i = 0; i < n; i++) w.g[i] = i < 3 ? out[n * n + i] * 2.0 : out[n * n + i];
  w.cost = out[n * n + n];
}
// minimize() of lii_calib.cpp:141-223 between two evaluations.  `out` holds the evaluation at the parameters this function left last.
// Returns 1 with the next point's parameters in `params`, or 0 when the loop has ended (w.term says why, w.p / w.cost are final).
__device__ int lm_advance(LmWork& w, const double* out, double* params) {
  const int n = w.p.dof;
  const double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  const double min_relative_decrease = 1e-3, min_diag = 1e-6, max_diag = 1e32, max_radius = 1e16, min_radius = 1e-32;
  const int max_iterations = 50, max_invalid = 5;
  if (!w.started) {  // the evaluation at the projected start point
    w.started = 1;
    lm_take(w, out);
    for (int i = 0; i < n; i++) w.scale[i] = 1.0 / (1.0 + sqrt(w.JtJ[i * n + i]));
    if (lm_gradient_max_norm(w.p, w.g, w.cand) <= gradient_tolerance) { w.term = LII_LM_GRADIENT_AT_START; return 0; }
    w.x_norm = lm_ambient_norm(w.p);
  } else {  // the evaluation at the candidate
    const double cand_cost = out[n * n + n];
    // parameter tolerance, then function tolerance - both on the candidate, before acceptance
    const double step_norm = lm_ambient_dist(w.p, w.cand);
    if (step_norm <= parameter_tolerance * (w.x_norm + parameter_tolerance)) { w.term = LII_LM_PARAMETER_TOLERANCE; return 0; }
    const double cost_change = w.cost - cand_cost;
    if (fabs(cost_change) <= function_tolerance * w.cost) { w.term = LII_LM_FUNCTION_TOLERANCE; return 0; }
    const double rho = cost_change / w.model_change;
    if (rho > min_relative_decrease) {
      w.p = w.cand;
      w.x_norm = lm_ambient_norm(w.p);
      lm_take(w, out);  // the candidate's evaluation is the evaluation at the new point
      w.radius = fmin(max_radius, w.radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * rho - 1.0, 3.0)));
      w.decrease_factor = 2.0;
      w.reuse_diag = 0;
      if (lm_gradient_max_norm(w.p, w.g, w.cand) <= gradient_tolerance) { w.term = LII_LM_GRADIENT_TOLERANCE; return 0; }
    } else {
      w.radius /= w.decrease_factor;
      w.decrease_factor *= 2.0;
    }
  }
  while (w.iter < max_iterations) {  // every pass counts an iteration: bounded by max_iterations
    if (w.radius < min_radius) { w.term = LII_LM_MIN_RADIUS; return 0; }
    w.iter++;
    // scaled system
    double A[81], gs[9], Js[81];
    for (int i = 0; i < n; i++) {
      gs[i] = w.g[i] * w.scale[i];
      for (int j = 0; j < n; j++) Js[i * n + j] = w.JtJ[i * n + j] * w.scale[i] * w.scale[j];
    }
    if (!w.reuse_diag)
      for (int i = 0; i < n; i++) w.diag[i] = fmin(fmax(Js[i * n + i], min_diag), max_diag);
    for (int i = 0; i < n * n; i++) A[i] = Js[i];
    for (int i = 0; i < n; i++) A[i * n + i] += w.diag[i] / w.radius;
    double y[9], step[9];
    const bool ok = lm_spd_solve(A, gs, n, y);
    w.reuse_diag = 1;
    double model_change = 0;
    if (ok) {
      for (int i = 0; i < n; i++) step[i] = -y[i];
      // model_cost_change = -(J s)^T (r + J s / 2) = -s^T g - s^T J^T J s / 2
      double sg = 0, sJs = 0;
      for (int i = 0; i < n; i++) {
        sg += step[i] * gs[i];
        double t = 0;
        for (int j = 0; j < n; j++) t += Js[i * n + j] * step[j];
        sJs += step[i] * t;
      }
      model_change = -sg - 0.5 * sJs;
    }
    if (!ok || !(model_change > 0.0)) {  // invalid step
      if (++w.invalid >= max_invalid) { w.term = LII_LM_INVALID_STEPS; return 0; }
      w.radius /= w.decrease_factor;
      w.decrease_factor *= 2.0;
      continue;
    }
    w.invalid = 0;
    w.model_change = model_change;
    double delta[9];
    for (int i = 0; i < n; i++) delta[i] = step[i] * w.scale[i];
    lm_plus(w.p, delta, w.cand);
    lm_params(w.cand, params);
    return 1;
  }
  w.term = LII_LM_MAX_ITERATIONS;
  return 0;
}

// One workgroup runs lii_calib_solve_stage: prologue (:227-242), minimize(), epilogue (:243-265) on the result block in device memory.
// mode 0: n records from index 0 of imu / lidar (lii_calib_solve_stage_dev); mode 1: the stage 1/2 view of the control block;
// mode 2: ctl->n3 records from index 0 (the stage-3 copies).
template <int STAGE>
__device__ __forceinline__ void d_calib_lm(const ResCtl* __restrict__ ctl, int mode, const double* __restrict__ imu,
                                           const double* __restrict__ lidar, int n, ResOut* __restrict__ ro) {
  constexpr int DOF = STAGE == 1 ? 3 : (STAGE == 2 ? 7 : 9);
  constexpr int NOUT = DOF * DOF + DOF + 1;
  constexpr int kMaxEvals = 51;  // the start point and one candidate per iteration (max_iterations = 50)
  __shared__ double sh[kEvalLds];
  __shared__ LmWork w;
  __shared__ double s_params[24], s_out[NOUT];
  __shared__ int s_go;
  if (mode != 0) {
    if (ctl->status) return;
    if (mode == 1) { imu += (size_t)ctl->ib * 22; lidar += (size_t)ctl->lb * 22; n = ctl->n; }
    else n = ctl->n3;
  }
  if (threadIdx.x == 0) {
    LmProblem& p = w.p;
    p.stage = STAGE;
    p.dof = DOF;
    for (int i = 0; i < 6; i++) { p.v[i] = 0; p.bounded[i] = 0; p.lo[i] = p.hi[i] = 0; }
    for (int i = 0; i < 9; i++) p.R_LI[i] = 0;
    if (STAGE == 1) {
      p.q = LmQuat{1, 0, 0, 0};  // LI_init.cpp:318-322
    } else if (STAGE == 2) {
      p.q = lm_rot_to_quat(ro->res.R_LI);  // Eigen::Quaterniond quat(Rot_Lidar_wrt_IMU), :346
    } else {
      p.q = LmQuat{1, 0, 0, 0};  // Rot_Init = I, :404-411
      for (int i = 0; i < 9; i++) p.R_LI[i] = ro->res.R_LI[i];
      for (int i = 0; i < 3; i++) { p.bounded[i] = 1; p.lo[i] = -0.01; p.hi[i] = 0.01; }  // :458-461
    }
    w.radius = 1e4;
    w.decrease_factor = 2.0;
    w.iter = w.invalid = w.reuse_diag = w.started = 0;
    w.term = LII_LM_MAX_ITERATIONS;
    w.cost = 0;
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    lm_plus(w.p, zero, w.p);  // Ceres projects the initial point onto the bounds
    for (int i = 0; i < 24; i++) s_params[i] = 0;
    lm_params(w.p, s_params);
  }
  __syncthreads();
  for (int e = 0; e < kMaxEvals; e++) {
    calib_eval_block<STAGE>(imu, lidar, n, s_params, sh, s_out);
    __syncthreads();
    if (threadIdx.x == 0) s_go = lm_advance(w, s_out, s_params);
    __syncthreads();
    if (!s_go) break;
  }
  if (threadIdx.x == 0) {
    lii_calib_result* io = &ro->res;
    io->iterations[STAGE - 1] = w.iter;
    io->final_cost[STAGE - 1] = w.cost;
    ro->termination[STAGE - 1] = w.term;
    double P[24];
    for (int i = 0; i < 24; i++) P[i] = 0;
    lm_params(w.p, P);
    for (int i = 0; i < 24; i++) ro->params[STAGE - 1][i] = P[i];
    const double* R = P;  // quat_to_rot(p.q)
    if (STAGE == 1) {
      for (int i = 0; i < 9; i++) io->R_LI[i] = R[i];
    } else if (STAGE == 2) {
      for (int i = 0; i < 9; i++) io->R_LI[i] = R[i];
      for (int i = 0; i < 3; i++) io->gyro_bias[i] = w.p.v[i];
      io->time_lag_2 = w.p.v[3];
    } else {
      const double g[3] = {0, 0, -9.81};
      double t[3];
      mat3_vec(R, g, t);                    // Grav_L0 = R_GL0 * STD_GRAV (:469)
      for (int i = 0; i < 3; i++) io->grav_L0[i] = t[i];
      mat3_vec(w.p.R_LI, w.p.v, t);         // acc_bias = R_LI * b_aL (:472)
      for (int i = 0; i < 3; i++) io->acc_bias[i] = t[i];
      mat3_vec(w.p.R_LI, w.p.v + 3, t);     // T_LI = -R_LI * T_IL (:475)
      for (int i = 0; i < 3; i++) io->T_LI[i] = -t[i];
    }
  }
}
template <int STAGE>
__global__ __launch_bounds__(256) void k_calib_lm(const ResCtl* __restrict__ ctl, int mode, const double* __restrict__ imu,
                                                  const double* __restrict__ lidar, int n, ResOut* __restrict__ ro) {
  d_calib_lm<STAGE>(ctl, mode, imu, lidar, n, ro);
}

void launch_calib_lm(int stage, const ResCtl* ctl, int mode, const double* imu, const double* lidar, int n, ResOut* ro, hipStream_t s) {
  if (stage == 1) hipLaunchKernelGGL(k_calib_lm<1>, dim3(1), dim3(256), 0, s, ctl, mode, imu, lidar, n, ro);
  else if (stage == 2) hipLaunchKernelGGL(k_calib_lm<2>, dim3(1), dim3(256), 0, s, ctl, mode, imu, lidar, n, ro);
  else hipLaunchKernelGGL(k_calib_lm<3>, dim3(1), dim3(256), 0, s, ctl, mode, imu, lidar, n, ro);
}

constexpr int kResidentLaunches = 14;

// the parts of lii_context::CalibState::Resident::d_seq for a capacity of c records
struct SeqLayout {
  double *imu, *lid, *imu3, *lid3, *tmp, *a, *b, *corr, *raw_lid;
  int* found;
  static size_t doubles(size_t c) { return c * (22 * 5 + 24 + 2 + 2) + c / 2 + 8; }
  SeqLayout(double* d, size_t c) {
    imu = d; lid = imu + 22 * c; imu3 = lid + 22 * c; lid3 = imu3 + 22 * c; tmp = lid3 + 22 * c;
    a = tmp + 24 * c; b = a + c; corr = b + c; raw_lid = corr + 2 * c;
    found = reinterpret_cast<int*>(raw_lid + 22 * c);
  }
};

// ------------------------------------------------------------------------------------------------ K windows of one upload
// lii_li_init_windows: window w = blockIdx.y runs the chain above on its slice of the upload, in areas of its own - its control and
// result block, a WinLayout sized by the longest window and, in the raw form, its filtered accelerations and stamps.  Every launch
// calls the device function the single form's kernel calls, on the window's pointers: same operations in the same order, and every
// order of addition depends on the window's own lengths alone.  Nothing is shared between windows but the read-only upload.
struct WinLayout {  // SeqLayout without the raw LiDAR copy (the upload is read in place)
  double *imu, *lid, *imu3, *lid3, *tmp, *a, *b, *corr;
  int* found;
  __host__ __device__ static size_t doubles(size_t c) { return c * (22 * 4 + 24 + 2 + 2) + c / 2 + 8; }
  __host__ __device__ WinLayout(double* d, size_t c) {
    imu = d; lid = imu + 22 * c; imu3 = lid + 22 * c; lid3 = imu3 + 22 * c; tmp = lid3 + 22 * c;
    a = tmp + 24 * c; b = a + c; corr = b + c;
    found = reinterpret_cast<int*>(corr + 2 * c);
  }
};
struct WinArgs {
  const lii_li_init_window* win;  // K descriptors
  double* small;                  // K x kSmallDoubles: ResCtl | ResOut
  double* seq;                    // K x WinLayout::doubles(cap)
  double* fts;                    // raw form: K x 4 cap_raw (facc: 3 per state, then ts)
  const double *src_imu, *src_lid;  // the upload
  int cap, cap_raw, interpolate, freq_cut;
};
struct Win {
  lii_li_init_window d;
  ResCtl* ctl;
  ResOut* ro;
  WinLayout L;
  double *facc, *ts;
  const double *raw, *raw_lid;
  __device__ Win(const WinArgs& A, int w)
      : d(A.win[w]), ctl(reinterpret_cast<ResCtl*>(A.small + (size_t)w * kSmallDoubles)),
        ro(reinterpret_cast<ResOut*>(A.small + (size_t)w * kSmallDoubles + sizeof(ResCtl) / 8)),
        L(A.seq + (size_t)w * WinLayout::doubles(size_t(A.cap)), size_t(A.cap)),
        facc(A.fts ? A.fts + (size_t)w * 4 * A.cap_raw : nullptr), ts(A.fts ? facc + (size_t)3 * A.cap_raw : nullptr),
        raw(A.src_imu + (size_t)d.imu_begin * 22), raw_lid(A.src_lid + (size_t)d.lidar_begin * 22) {}
};
// aligned form: the window's slice of the upload -> its own sequences (the chain works in place); grid: 22 * cap elements x K
__global__ __launch_bounds__(256) void k_win_gather(WinArgs A) {
  if (A.interpolate) return;
  const Win W(A, blockIdx.y);
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= W.d.lidar_count * 22) return;
  W.L.imu[e] = W.raw[e];
  W.L.lid[e] = W.raw_lid[e];
}
// the three kernels of more than one workgroup: the grid is the longest window's, a workgroup beyond its own window's returns
__global__ __launch_bounds__(256) void k_win_interp_filter(WinArgs A) {
  const Win W(A, blockIdx.y);
  if ((int)blockIdx.x * 256 >= max(W.d.imu_count, 1)) return;
  d_res_interp_filter(W.ctl, A.interpolate, W.raw, W.d.imu_count, W.raw_lid, W.d.lidar_count, W.d.move_start_time, W.facc, W.ts, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_win_interp_search(WinArgs A) {
  const Win W(A, blockIdx.y);
  if ((int)blockIdx.x >= W.d.lidar_count) return;
  d_res_interp_search(W.ctl, A.interpolate, W.ts, W.d.imu_count, W.raw_lid, W.L.found, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_win_xcorr(WinArgs A) {
  const Win W(A, blockIdx.y);
  if ((int)blockIdx.x * 256 >= 2 * W.d.lidar_count - 1 || W.ctl->status) return;
  xcorr_lane(W.L.a, W.L.b, W.ctl->means, W.ctl->n, W.L.corr, blockIdx.x * 256 + threadIdx.x);
}
// the kernels of one workgroup: 1 x K
__global__ __launch_bounds__(256) void k_win_interp_compact(WinArgs A) {
  const Win W(A, blockIdx.y);
  d_res_interp_compact(W.ctl, A.interpolate, W.raw, W.facc, W.raw_lid, W.L.found, W.d.lidar_count, W.L.imu, W.L.lid);
}
__global__ __launch_bounds__(256) void k_win_head(WinArgs A) {
  const Win W(A, blockIdx.y);
  d_res_head(W.ctl, A.interpolate, W.d.lidar_count, W.L.imu, W.L.lid);
}
__global__ __launch_bounds__(256) void k_win_zero_phase(WinArgs A, unsigned int mask) {
  const Win W(A, blockIdx.y);
  d_res_zero_phase(W.ctl, W.L.imu, W.L.lid, W.L.tmp, mask);
}
__global__ __launch_bounds__(256) void k_win_mid(WinArgs A) {
  const Win W(A, blockIdx.y);
  d_res_mid(W.ctl, W.L.imu, W.L.lid, W.L.a, W.L.b);
}
__global__ __launch_bounds__(256) void k_win_argmax(WinArgs A) {
  __shared__ double s_v[256];
  __shared__ int s_k[256];
  const Win W(A, blockIdx.y);
  if (W.ctl->status) return;
  xcorr_argmax_block(W.L.corr, W.ctl->n, &W.ctl->lag, s_v, s_k);
}
__global__ __launch_bounds__(256) void k_win_after_lag(WinArgs A) {
  const Win W(A, blockIdx.y);
  d_res_after_lag(W.ctl, W.L.imu, W.L.lid, A.freq_cut);
}
__global__ __launch_bounds__(256) void k_win_stage3_prep(WinArgs A) {  // the stage-3 sequences stay in the window's area
  const Win W(A, blockIdx.y);
  d_res_stage3_prep<false>(W.ctl, W.ro, W.L.imu, W.L.lid, W.L.imu3, W.L.lid3, nullptr, nullptr);
}
template <int STAGE>
__global__ __launch_bounds__(256) void k_win_calib_lm(WinArgs A) {
  const Win W(A, blockIdx.y);
  if (STAGE == 3) d_calib_lm<STAGE>(W.ctl, 2, W.L.imu3, W.L.lid3, 0, W.ro);
  else d_calib_lm<STAGE>(W.ctl, 1, W.L.imu, W.L.lid, 0, W.ro);
}
constexpr int kWindowsLaunches = 15;
constexpr int kWindowsMax = 4096;
constexpr size_t kWindowsScratchMax = size_t(4) << 30;  // bytes of device scratch one call may ask for
static_assert(kSmallDoubles == 113, "liinit_hip.h states the per-window bytes");
static_assert(sizeof(lii_li_init_window) == 24, "lii_li_init_window layout");
static_assert(kResFilter61 == LII_WIN_FILTER61 && kResAligned200 == LII_WIN_ALIGNED200 && kResRaw6 == LII_WIN_RAW6 &&
              kResAlign == LII_WIN_NO_OVERLAP, "lii_li_init_window_result::status is the ResStatus");

// what lii_li_init_resident reports of a run that ended with status kResOk (launches / host_waits are the caller's)
void fill_report(const ResCtl& c, const ResOut& o, lii_li_init_report* rep) {
  rep->n_aligned = c.n_aligned;
  rep->n_stage12 = c.n12;
  rep->n_stage3 = c.n3;
  rep->lag_samples = c.lag;
  for (int k = 0; k < 3; k++) rep->termination[k] = o.termination[k];
  rep->time_lag_1 = c.lag1;
  rep->total_time_lag = c.lag1 + o.res.time_lag_2;
  std::memcpy(rep->params, o.params, sizeof(o.params));
}

int ensure_small(lii_handle h) {
  auto& r = h->cal.res;
  if (!r.d_small) HIPCHK(h, r.d_small.alloc(kSmallDoubles));
  return LII_OK;
}
ResCtl* ctl_of(lii_handle h) { return reinterpret_cast<ResCtl*>(h->cal.res.d_small.get()); }
ResOut* out_of(lii_handle h) { return reinterpret_cast<ResOut*>(h->cal.res.d_small.get() + sizeof(ResCtl) / 8); }

}  // namespace
}  // namespace lii

using namespace lii;
using lii_impl::fail;

extern "C" {

int lii_li_init_resident(lii_handle h, const lii_li_init_job* job, lii_calib_result* out, lii_li_init_report* rep) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !job || !out) return fail(h, LII_ERR_INVALID, "lii_li_init_resident: NULL argument");
  if (job->struct_size != sizeof(lii_li_init_job) || (rep && rep->struct_size != sizeof(lii_li_init_report)))
    return fail(h, LII_ERR_INVALID, "lii_li_init_resident: bad struct_size");
  if (job->interpolate != 0 && job->interpolate != 1) return fail(h, LII_ERR_INVALID, "lii_li_init_resident: interpolate must be 0 or 1");
  if (!job->imu || !job->lidar || job->orig_odom_freq < 1 || job->cut_frame_num < 1)
    return fail(h, LII_ERR_INVALID, "lii_li_init_resident: bad arguments");
  if (job->interpolate == 0 && (job->n_imu < 200 || job->n_imu != job->n_lidar))
    return fail(h, LII_ERR_INVALID, "lii_li_init_resident: the aligned form takes n_imu == n_lidar >= 200 states");
  if (job->interpolate == 1 && (job->n_imu < 6 || job->n_lidar < 1))
    return fail(h, LII_ERR_INVALID, "lii_li_init_resident: the raw form takes n_imu >= 6 and n_lidar >= 1 states");
  if (lii_internal_in_wait_hook(h)) return fail(h, LII_ERR_STATE, "lii_li_init_resident: not from inside lii_scan_job::while_waiting");
  auto& r = h->cal.res;
  const int itp = job->interpolate, n_in = job->n_lidar, n_raw = itp ? job->n_imu : 0;
  // buffers: geometric growth, nothing released in the steady state
  int rc = ensure_small(h);
  if (rc != LII_OK) return rc;
  if (n_in > r.cap_n) {
    const int cap = std::max(n_in, 2 * r.cap_n);
    r.cap_n = 0;
    r.have_run = false;
    HIPCHK(h, r.d_seq.grow(SeqLayout::doubles(size_t(cap))));
    r.cap_n = cap;
  }
  if (n_raw > r.cap_raw) {
    const int cap = std::max(n_raw, 2 * r.cap_raw);
    r.cap_raw = 0;
    HIPCHK(h, r.d_raw.grow(size_t(cap) * 26));
    r.cap_raw = cap;
  }
  if (n_in > int(h->cal.d_cal_imu.size() / 22) || n_in > int(h->cal.d_cal_lidar.size() / 22)) {
    const size_t cap = std::max(size_t(n_in), 2 * (h->cal.d_cal_imu.size() / 22));
    h->cal.n_cal = 0;
    HIPCHK(h, h->cal.d_cal_imu.grow(cap * 22));
    HIPCHK(h, h->cal.d_cal_lidar.grow(cap * 22));
  }
  const SeqLayout L(r.d_seq, size_t(r.cap_n));
  double* raw_imu = r.d_raw;
  double* facc = raw_imu ? raw_imu + size_t(r.cap_raw) * 22 : nullptr;
  double* ts = raw_imu ? facc + size_t(r.cap_raw) * 3 : nullptr;
  ResCtl* ctl = ctl_of(h);
  ResOut* ro = out_of(h);
  hipStream_t s = h->stream;
  r.have_run = false;

  // the one upload
  HIPCHK(h, hipMemsetAsync(r.d_small, 0, sizeof(double) * kSmallDoubles, s));
  if (itp) {
    HIPCHK(h, hipMemcpyAsync(raw_imu, job->imu, sizeof(lii_calib_state) * size_t(job->n_imu), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(L.raw_lid, job->lidar, sizeof(lii_calib_state) * size_t(n_in), hipMemcpyHostToDevice, s));
  } else {
    HIPCHK(h, hipMemcpyAsync(L.imu, job->imu, sizeof(lii_calib_state) * size_t(n_in), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(L.lid, job->lidar, sizeof(lii_calib_state) * size_t(n_in), hipMemcpyHostToDevice, s));
  }
  const dim3 one(1), wg(256);
  const unsigned int all_channels = 0xFFFFFFu;
  const unsigned int second_filter = (7u << 6) | (7u << 18) | (7u << 21);  // IMU ang_acc; LiDAR ang_acc, linear_acc
  int launches = 0;
  hipLaunchKernelGGL(k_res_interp_filter, dim3(std::max(1, (n_raw + 255) / 256)), wg, 0, s, ctl, itp, raw_imu, n_raw, L.raw_lid, n_in,
                     job->move_start_time, facc, ts); launches++;
  hipLaunchKernelGGL(k_res_interp_search, dim3(itp ? n_in : 1), wg, 0, s, ctl, itp, ts, n_raw, L.raw_lid, L.found); launches++;
  hipLaunchKernelGGL(k_res_interp_compact, one, wg, 0, s, ctl, itp, raw_imu, facc, L.raw_lid, L.found, n_in, L.imu, L.lid); launches++;
  hipLaunchKernelGGL(k_res_head, one, wg, 0, s, ctl, itp, n_in, L.imu, L.lid); launches++;
  hipLaunchKernelGGL(k_res_zero_phase, one, wg, 0, s, ctl, L.imu, L.lid, L.tmp, all_channels); launches++;
  hipLaunchKernelGGL(k_res_mid, one, wg, 0, s, ctl, L.imu, L.lid, L.a, L.b); launches++;
  hipLaunchKernelGGL(k_res_xcorr, dim3((2 * n_in - 1 + 255) / 256), wg, 0, s, ctl, L.a, L.b, L.corr); launches++;
  hipLaunchKernelGGL(k_res_argmax, one, wg, 0, s, ctl, L.corr); launches++;
  hipLaunchKernelGGL(k_res_after_lag, one, wg, 0, s, ctl, L.imu, L.lid, job->orig_odom_freq * job->cut_frame_num); launches++;
  hipLaunchKernelGGL(k_res_zero_phase, one, wg, 0, s, ctl, L.imu, L.lid, L.tmp, second_filter); launches++;
  launch_calib_lm(1, ctl, 1, L.imu, L.lid, 0, ro, s); launches++;
  launch_calib_lm(2, ctl, 1, L.imu, L.lid, 0, ro, s); launches++;
  hipLaunchKernelGGL(k_res_stage3_prep, one, wg, 0, s, ctl, ro, L.imu, L.lid, L.imu3, L.lid3, h->cal.d_cal_imu.get(), h->cal.d_cal_lidar.get()); launches++;
  launch_calib_lm(3, ctl, 2, L.imu3, L.lid3, 0, ro, s); launches++;
  static_assert(sizeof(ResCtl) % 8 == 0, "the result block follows the control block");
  static_assert(kSmallDoubles <= kLiInitBackDoubles, "PinnedScratch::li_init_back holds the control and the result block");
  double* back = h->h_small->li_init_back;
  HIPCHK(h, hipMemcpyAsync(back, r.d_small, sizeof(double) * kSmallDoubles, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));  // the one wait
  HIPCHK(h, hipGetLastError());
  ResCtl c;
  ResOut o;
  std::memcpy(&c, back, sizeof(c));
  std::memcpy(&o, back + sizeof(ResCtl) / 8, sizeof(o));
  if (c.status == kResFilter61) return fail(h, LII_ERR_INVALID, "lii_li_init_run: fewer than 61 aligned states left to filter");
  if (c.status == kResAligned200) return fail(h, LII_ERR_INVALID, "lii_li_init_resident: fewer than 200 aligned states after interpolation");
  if (c.status == kResRaw6) return fail(h, LII_ERR_INVALID, "lii_li_init_resident: fewer than 6 raw IMU states behind move_start_time - 3 s");
  if (c.status != kResOk) return fail(h, LII_ERR_INVALID, "lii_li_init_resident: the sequences do not overlap in time");
  *out = o.res;
  h->cal.n_cal = c.n3;
  r.have_run = true;
  r.ib12 = c.ib12; r.lb12 = c.lb12; r.n12 = c.n12; r.n3 = c.n3;
  if (rep) {
    fill_report(c, o, rep);
    rep->launches = launches;
    rep->host_waits = 1;
  }
  static_assert(kResidentLaunches == 14, "lii_li_init_report::launches");
  return LII_OK;
}

int lii_li_init_windows(lii_handle h, const lii_li_init_job* job, const lii_li_init_window* windows, int32_t n_windows,
                        lii_li_init_window_result* out, uint32_t out_stride) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !job || !windows || !out) return fail(h, LII_ERR_INVALID, "lii_li_init_windows: NULL argument");
  if (job->struct_size != sizeof(lii_li_init_job) || out_stride != sizeof(lii_li_init_window_result))
    return fail(h, LII_ERR_INVALID, "lii_li_init_windows: bad struct_size or out_stride");
  if (job->interpolate != 0 && job->interpolate != 1) return fail(h, LII_ERR_INVALID, "lii_li_init_windows: interpolate must be 0 or 1");
  if (!job->imu || !job->lidar || job->n_imu < 1 || job->n_lidar < 1 || job->orig_odom_freq < 1 || job->cut_frame_num < 1)
    return fail(h, LII_ERR_INVALID, "lii_li_init_windows: bad arguments");
  if (n_windows < 1 || n_windows > kWindowsMax) return fail(h, LII_ERR_INVALID, "lii_li_init_windows: n_windows must be 1 .. 4096");
  const int itp = job->interpolate, K = n_windows;
  int cap = 0, cap_raw = 0;
  for (int w = 0; w < K; w++) {
    const lii_li_init_window& d = windows[w];
    if (d.imu_begin < 0 || d.imu_count < 0 || d.lidar_begin < 0 || d.lidar_count < 0 || d.imu_count > job->n_imu - d.imu_begin ||
        d.lidar_count > job->n_lidar - d.lidar_begin)
      return fail(h, LII_ERR_INVALID, "lii_li_init_windows: a window lies outside the job's sequences");
    if (!itp && (d.imu_begin != d.lidar_begin || d.imu_count != d.lidar_count || d.lidar_count < 200))
      return fail(h, LII_ERR_INVALID, "lii_li_init_windows: an aligned window takes imu range == lidar range, 200 states or more");
    if (itp && (d.imu_count < 6 || d.lidar_count < 1))
      return fail(h, LII_ERR_INVALID, "lii_li_init_windows: a raw window takes imu_count >= 6 and lidar_count >= 1");
    cap = std::max(cap, d.lidar_count);
    if (itp) cap_raw = std::max(cap_raw, d.imu_count);
  }
  if (lii_internal_in_wait_hook(h)) return fail(h, LII_ERR_STATE, "lii_li_init_windows: not from inside lii_scan_job::while_waiting");
  const size_t n_src = (size_t(job->n_imu) + size_t(job->n_lidar)) * 22;
  const size_t n_seq = size_t(K) * WinLayout::doubles(size_t(cap)), n_fts = size_t(K) * 4 * size_t(cap_raw);
  const size_t n_small = size_t(K) * kSmallDoubles;
  const size_t bytes = 8 * (n_src + n_seq + n_fts + n_small) + sizeof(lii_li_init_window) * size_t(K);
  if (bytes > kWindowsScratchMax) return fail(h, LII_ERR_CAPACITY, "lii_li_init_windows: the windows' scratch would exceed 4 GiB");
  // buffers: geometric growth (never beyond the limit), nothing released in the steady state
  auto& r = h->cal.win;
  auto room = [&](auto& buf, size_t n, size_t elem) -> hipError_t {
    if (n <= buf.size()) return hipSuccess;
    r.allocations++;
    return buf.grow(std::max(n, std::min(2 * buf.size(), kWindowsScratchMax / elem)));
  };
  HIPCHK(h, room(r.d_src, n_src, 8));
  HIPCHK(h, room(r.d_seq, n_seq, 8));
  HIPCHK(h, room(r.d_fts, n_fts, 8));
  HIPCHK(h, room(r.d_small, n_small, 8));
  HIPCHK(h, room(r.d_win, size_t(K), sizeof(lii_li_init_window)));
  if (n_small > r.h_back.size()) {
    r.allocations++;
    HIPCHK(h, r.h_back.at_least(n_small, hipHostMallocDefault));
  }
  hipStream_t s = h->stream;
  double* src_imu = r.d_src;
  double* src_lid = src_imu + size_t(job->n_imu) * 22;
  // the one upload
  HIPCHK(h, hipMemsetAsync(r.d_small, 0, sizeof(double) * n_small, s));
  HIPCHK(h, hipMemcpyAsync(src_imu, job->imu, sizeof(lii_calib_state) * size_t(job->n_imu), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(src_lid, job->lidar, sizeof(lii_calib_state) * size_t(job->n_lidar), hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(r.d_win, windows, sizeof(lii_li_init_window) * size_t(K), hipMemcpyHostToDevice, s));
  WinArgs A;
  A.win = r.d_win; A.small = r.d_small; A.seq = r.d_seq; A.fts = itp ? r.d_fts.get() : nullptr;
  A.src_imu = src_imu; A.src_lid = src_lid;
  A.cap = cap; A.cap_raw = cap_raw; A.interpolate = itp; A.freq_cut = job->orig_odom_freq * job->cut_frame_num;
  const unsigned int uk = (unsigned int)K;
  const dim3 one(1, uk), wg(256);
  const unsigned int all_channels = 0xFFFFFFu;
  const unsigned int second_filter = (7u << 6) | (7u << 18) | (7u << 21);  // IMU ang_acc; LiDAR ang_acc, linear_acc
  int launches = 0;
  hipLaunchKernelGGL(k_win_gather, dim3(itp ? 1 : (cap * 22 + 255) / 256, uk), wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_interp_filter, dim3(std::max(1, (cap_raw + 255) / 256), uk), wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_interp_search, dim3(itp ? cap : 1, uk), wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_interp_compact, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_head, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_zero_phase, one, wg, 0, s, A, all_channels); launches++;
  hipLaunchKernelGGL(k_win_mid, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_xcorr, dim3((2 * cap - 1 + 255) / 256, uk), wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_argmax, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_after_lag, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_zero_phase, one, wg, 0, s, A, second_filter); launches++;
  hipLaunchKernelGGL(k_win_calib_lm<1>, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_calib_lm<2>, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_stage3_prep, one, wg, 0, s, A); launches++;
  hipLaunchKernelGGL(k_win_calib_lm<3>, one, wg, 0, s, A); launches++;
  double* back = r.h_back;
  HIPCHK(h, hipMemcpyAsync(back, r.d_small, sizeof(double) * n_small, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));  // the one wait
  HIPCHK(h, hipGetLastError());
  static_assert(kWindowsLaunches == 15, "lii_li_init_window_result::rep.launches");
  for (int w = 0; w < K; w++) {
    ResCtl c;
    ResOut o;
    std::memcpy(&c, back + size_t(w) * kSmallDoubles, sizeof(c));
    std::memcpy(&o, back + size_t(w) * kSmallDoubles + sizeof(ResCtl) / 8, sizeof(o));
    lii_li_init_window_result& q = out[w];
    std::memset(&q, 0, sizeof(q));
    q.status = c.status;
    if (c.status != kResOk) continue;
    q.res = o.res;
    q.rep.struct_size = sizeof(lii_li_init_report);
    fill_report(c, o, &q.rep);
    q.rep.launches = launches;
    q.rep.host_waits = 1;
  }
  return LII_OK;
}

int lii_li_init_windows_scratch(lii_handle h, uint64_t* bytes, int64_t* allocations) {
  if (!h) return fail(h, LII_ERR_INVALID, "lii_li_init_windows_scratch: NULL handle");
  const auto& r = h->cal.win;
  if (bytes) *bytes = 8 * uint64_t(r.d_src.size() + r.d_seq.size() + r.d_fts.size() + r.d_small.size()) + sizeof(lii_li_init_window) * uint64_t(r.d_win.size());
  if (allocations) *allocations = r.allocations;
  return LII_OK;
}

int lii_li_init_resident_fetch(lii_handle h, int32_t which, lii_calib_state* imu, lii_calib_state* lidar, int32_t capacity, int32_t* n) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !n || (which != 1 && which != 2) || capacity < 0 || (!imu) != (!lidar))
    return fail(h, LII_ERR_INVALID, "lii_li_init_resident_fetch: bad arguments");
  if (lii_internal_in_wait_hook(h)) return fail(h, LII_ERR_STATE, "lii_li_init_resident_fetch: not from inside lii_scan_job::while_waiting");
  auto& r = h->cal.res;
  if (!r.have_run) return fail(h, LII_ERR_STATE, "lii_li_init_resident_fetch: no resident run yet");
  const int cnt = which == 1 ? r.n12 : r.n3;
  *n = cnt;
  if (!imu) return LII_OK;
  if (capacity < cnt) return fail(h, LII_ERR_CAPACITY, "lii_li_init_resident_fetch: capacity below the number of states");
  const SeqLayout L(r.d_seq, size_t(r.cap_n));
  const double* si = which == 1 ? L.imu + size_t(r.ib12) * 22 : L.imu3;
  const double* sl = which == 1 ? L.lid + size_t(r.lb12) * 22 : L.lid3;
  HIPCHK(h, hipMemcpyAsync(imu, si, sizeof(lii_calib_state) * size_t(cnt), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(lidar, sl, sizeof(lii_calib_state) * size_t(cnt), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return LII_OK;
}

int lii_calib_solve_stage_dev(lii_handle h, int32_t stage, lii_calib_result* io) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !io || stage < 1 || stage > 3) return fail(h, LII_ERR_INVALID, "lii_calib_solve_stage_dev: bad arguments");
  if (lii_internal_in_wait_hook(h)) return fail(h, LII_ERR_STATE, "lii_calib_solve_stage_dev: not from inside lii_scan_job::while_waiting");
  if (h->cal.n_cal <= 0) return fail(h, LII_ERR_STATE, "lii_calib_solve_stage_dev: no buffers uploaded");
  const int rc = ensure_small(h);
  if (rc != LII_OK) return rc;
  ResOut* ro = out_of(h);
  lii_calib_result* stage_io = &h->h_small->calib_stage;
  *stage_io = *io;
  HIPCHK(h, hipMemcpyAsync(&ro->res, stage_io, sizeof(lii_calib_result), hipMemcpyHostToDevice, h->stream));
  launch_calib_lm(stage, nullptr, 0, h->cal.d_cal_imu, h->cal.d_cal_lidar, h->cal.n_cal, ro, h->stream);
  HIPCHK(h, hipMemcpyAsync(stage_io, &ro->res, sizeof(lii_calib_result), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipGetLastError());
  *io = *stage_io;
  return LII_OK;
}

}  // extern "C"

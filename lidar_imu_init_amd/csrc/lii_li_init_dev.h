// Device functions the two LI-Init units share (lii_li_init_dev.hip: the stand-alone kernels behind lii_calib_eval, lii_xcorr_lag;
// lii_li_init_resident.hip: the resident chain and the device Levenberg-Marquardt).  One text per piece of arithmetic, so that both
// users produce the same bits at the same inputs.  Both units are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "lii_device.h"

namespace lii {

__device__ __forceinline__ double norm3_at(const double* __restrict__ rec) {
  return sqrt(rec[9] * rec[9] + rec[10] * rec[10] + rec[11] * rec[11]);
}

// LI_Init::xcorr_temporal_init (include/LI_init/LI_init.cpp:160-193): corr[k] for lag = k - (n - 1), products summed in ascending i
__device__ __forceinline__ void xcorr_lane(const double* __restrict__ a, const double* __restrict__ b, const double* __restrict__ means,
                                           int n, double* __restrict__ corr, int k) {
  if (k >= 2 * n - 1) return;
  const int lag = k - (n - 1);
  const double ma = means[0], mb = means[1];
  const int i0 = max(0, -lag), i1 = min(n, n - lag);
  double c = 0;
  for (int i = i0; i < i1; i++) c += (a[i] - ma) * (b[i + lag] - mb);
  corr[k] = c;
}
// first maximum in ascending lag order (the reference: `if (c > best)`), result = lag_IMU_wtr_Lidar = -lag; a workgroup of 256 lanes
__device__ __forceinline__ void xcorr_argmax_block(const double* __restrict__ corr, int n, int* __restrict__ out_lag, double* s_v, int* s_k) {
  const int m = 2 * n - 1;
  double best = -1.7976931348623157e308;
  int bk = 0x7FFFFFFF;
  for (int k = threadIdx.x; k < m; k += 256) {
    const double v = corr[k];
    if (v > best) { best = v; bk = k; }  // a lane walks its lags in ascending order: strict '>' keeps its first maximum
  }
  s_v[threadIdx.x] = best;
  s_k[threadIdx.x] = bk;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double v = s_v[threadIdx.x + s];
      const int k = s_k[threadIdx.x + s];
      if (v > s_v[threadIdx.x] || (v == s_v[threadIdx.x] && k < s_k[threadIdx.x])) { s_v[threadIdx.x] = v; s_k[threadIdx.x] = k; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out_lag = s_k[0] == 0x7FFFFFFF ? 0 : -(s_k[0] - (n - 1));
}

// ------------------------------------------------------------------------------------------------
// LI-Init residual / Jacobian evaluators (include/LI_init/LI_init.h:91-205).  Records are 22 doubles:
// rot_end[9], ang_vel[3], linear_vel[3], ang_acc[3], linear_acc[3], timestamp.
// Tangent convention R <- Exp(delta) R  (Appendix B of SURVEY.md):
//   stage 1/2: r = R w_L - w_I [- (dT + t_d) a_I + b_g];  dr/ddelta = -[R w_L]x, dr/db_g = I, dr/dt_d = -alpha_I
//   stage 3:   r = R_LL0 R_LI^T a_I - R_LL0 b_a + R_GL0 g - a_L - R_LL0 ([w]x^2 + [alpha]x) T_IL
//              dr/ddelta_G = -[R_GL0 g]x, dr/db_a = -R_LL0, dr/dT_IL = -R_LL0 ([w]x^2 + [alpha]x)
// Output: dof*dof + dof + 1 doubles (J^T J row-major, J^T r, 0.5 sum r^2), reduced on one workgroup of 256 lanes.
constexpr int kEvalChunk = 32;                  // outputs that cross the workgroup per pass of the reduction
constexpr int kEvalLds = kEvalChunk * 128;      // doubles of LDS the reduction needs (32 KiB)

// Lane l sums records l, l + 256, ... in ascending order; then the tree over the 256 lanes pairs t with t + s for s = 128 ... 1
// (tests/li_init_shapes.py derives its bound from that pairing).  The tree moves kEvalChunk outputs per step: s = 128 and s = 64
// through LDS (the upper half writes, a barrier, the lower half adds), s = 32 ... 1 inside the first wavefront by lane shifts.
// `params` may be global memory or LDS; `out` (written by lane 0) likewise - the caller places a barrier before anybody reads it.
template <int STAGE>
__device__ __forceinline__ void calib_eval_block(const double* __restrict__ imu, const double* __restrict__ lidar, int n,
                                                 const double* params, double* sh, double* out) {
  constexpr int DOF = STAGE == 1 ? 3 : (STAGE == 2 ? 7 : 9);
  constexpr int NOUT = DOF * DOF + DOF + 1;
  double acc[NOUT];
#pragma unroll
  for (int k = 0; k < NOUT; k++) acc[k] = 0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double* I = imu + 22 * (size_t)i;
    const double* L = lidar + 22 * (size_t)i;
    double r[3];
    double J[3][DOF];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
      for (int b = 0; b < DOF; b++) J[a][b] = 0;
    if (STAGE == 1 || STAGE == 2) {
      const double* R = params;
      double Rw[3];
      mat3_vec(R, L + 9, Rw);
#pragma unroll
      for (int a = 0; a < 3; a++) r[a] = Rw[a] - I[9 + a];
      // -[Rw]x
      J[0][1] = Rw[2]; J[0][2] = -Rw[1];
      J[1][0] = -Rw[2]; J[1][2] = Rw[0];
      J[2][0] = Rw[1]; J[2][1] = -Rw[0];
      if (STAGE == 2) {
        const double* bg = params + 9;
        double td = params[12];
        double dT = L[21] - I[21];
#pragma unroll
        for (int a = 0; a < 3; a++) {
          r[a] = r[a] - (dT + td) * I[15 + a] + bg[a];
          J[a][(3 + a) % DOF] = 1.0;
          J[a][6 % DOF] = -I[15 + a];
        }
      }
    } else {
      const double* RG = params;        // R_GL0
      const double* ba = params + 9;    // bias_aL
      const double* Til = params + 12;  // T_IL
      const double* RLI = params + 15;  // R_LI (fixed)
      const double* RLL0 = L;           // rot_end
      const double g[3] = {0, 0, -9.81};  // STD_GRAV (LI_init.h:27)
      double aI_L[3], t1[3], Rg[3];
      mat3t_vec(RLI, I + 18, aI_L);  // R_LI^T a_I
      mat3_vec(RLL0, aI_L, t1);      // R_LL0 R_LI^T a_I
      mat3_vec(RG, g, Rg);
      const double* w = L + 9;
      const double* al = L + 15;
      double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
      double A[9] = {0, -al[2], al[1], al[2], 0, -al[0], -al[1], al[0], 0};
      double M[9], RM[9];
      mat3_mul(W, W, M);
#pragma unroll
      for (int e = 0; e < 9; e++) M[e] += A[e];
      mat3_mul(RLL0, M, RM);
      double Rb[3], RMt[3];
      mat3_vec(RLL0, ba, Rb);
      mat3_vec(RM, Til, RMt);
#pragma unroll
      for (int a = 0; a < 3; a++) r[a] = t1[a] - Rb[a] + Rg[a] - L[18 + a] - RMt[a];
      J[0][1] = Rg[2]; J[0][2] = -Rg[1];
      J[1][0] = -Rg[2]; J[1][2] = Rg[0];
      J[2][0] = Rg[1]; J[2][1] = -Rg[0];
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
          J[a][(3 + b) % DOF] = -RLL0[3 * a + b];
          J[a][(6 + b) % DOF] = -RM[3 * a + b];
        }
    }
#pragma unroll
    for (int a = 0; a < DOF; a++) {
#pragma unroll
      for (int b = 0; b < DOF; b++) acc[a * DOF + b] += J[0][a] * J[0][b] + J[1][a] * J[1][b] + J[2][a] * J[2][b];
      acc[DOF * DOF + a] += J[0][a] * r[0] + J[1][a] * r[1] + J[2][a] * r[2];
    }
    acc[DOF * DOF + DOF] += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  }
  const int t = threadIdx.x;
#pragma unroll
  for (int c0 = 0; c0 < NOUT; c0 += kEvalChunk) {
    if (t >= 128) {
#pragma unroll
      for (int k = c0; k < c0 + kEvalChunk && k < NOUT; k++) sh[(k - c0) * 128 + (t - 128)] = acc[k];
    }
    __syncthreads();
    if (t < 128) {
#pragma unroll
      for (int k = c0; k < c0 + kEvalChunk && k < NOUT; k++) acc[k] += sh[(k - c0) * 128 + t];
    }
    __syncthreads();
    if (t >= 64 && t < 128) {
#pragma unroll
      for (int k = c0; k < c0 + kEvalChunk && k < NOUT; k++) sh[(k - c0) * 64 + (t - 64)] = acc[k];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
      for (int k = c0; k < c0 + kEvalChunk && k < NOUT; k++) acc[k] += sh[(k - c0) * 64 + t];
    }
    __syncthreads();
  }
  if (t < 64) {  // the first wavefront: lane t takes lane t + s's sum; what the lanes >= s hold from here on is not used
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
      for (int k = 0; k < NOUT; k++) acc[k] += __shfl_down(acc[k], s, 64);
    }
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < NOUT; k++) out[k] = acc[k];
    }
  }
}

}  // namespace lii

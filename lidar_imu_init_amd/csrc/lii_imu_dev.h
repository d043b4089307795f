// Device code that the propagation kernels of lii_imu.hip share with the de-skew launch that carries a propagation
// (lii_scan.hip: k_deskew_cv_prop): the covariance step P <- F P F^T + Q over the non-zero blocks of F_x, the constant-velocity
// propagation built on it, and the pull of the update's control block out of pinned host memory.
// Both units are built without FMA contraction (csrc/Makefile: the reference's x86-64 build has none either); a kernel that calls
// these from a unit that contracts would not produce the bits of the others.
#pragma once
#include <hip/hip_runtime.h>

#include "lii_device.h"

namespace lii {

// sum_k F[r][k] M[k] over the non-zero entries of row r of F_x, in ascending k (M[k] = Mb[k * sk]):
//   rows 0-2    E (cols 0-2), a15 I (cols 15-17)                          :338-339 / :229-230
//   rows 3-5    I, dt I (cols 12-14)                                      :340 / :231
//   rows 12-14  B (cols 0-2), I, Cm (cols 18-20), dt I (cols 21-23)       :341-343   (B == nullptr: the CV model has no such rows)
__device__ __forceinline__ double f_row(int r, const double* __restrict__ Mb, int sk, const double* __restrict__ E, double a15, double dt,
                                        const double* __restrict__ B, const double* __restrict__ Cm) {
  if (r < 3) return E[3 * r] * Mb[0] + E[3 * r + 1] * Mb[sk] + E[3 * r + 2] * Mb[2 * sk] + a15 * Mb[(15 + r) * sk];
  if (r < 6) return Mb[r * sk] + dt * Mb[(r + 9) * sk];
  if (B && r >= 12 && r < 15) {
    const int i = r - 12;
    double s = B[3 * i] * Mb[0] + B[3 * i + 1] * Mb[sk] + B[3 * i + 2] * Mb[2 * sk];
    s += Mb[r * sk];
    s += Cm[3 * i] * Mb[18 * sk];
    s += Cm[3 * i + 1] * Mb[19 * sk];
    s += Cm[3 * i + 2] * Mb[20 * sk];
    s += dt * Mb[(21 + i) * sk];
    return s;
  }
  return Mb[r * sk];
}
// P <- F P F^T + Q (:352 / :238), P and T in LDS, every lane of a 256-lane workgroup calls it.  qd: the diagonal of cov_w; Qa: its
// (12,12) block when that block is full (:348), else nullptr.
__device__ __forceinline__ void cov_step(double* __restrict__ P, double* __restrict__ T, const double* __restrict__ E, double a15, double dt,
                                         const double* __restrict__ B, const double* __restrict__ Cm, const double* __restrict__ qd,
                                         const double* __restrict__ Qa) {
  for (int e = threadIdx.x; e < 576; e += 256) {  // T = F P
    const int r = e / 24, c = e - 24 * r;
    T[e] = f_row(r, P + c, 24, E, a15, dt, B, Cm);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 576; e += 256) {  // P = T F^T + Q:  (T F^T)[r][c] = sum_k F[c][k] T[r][k]
    const int r = e / 24, c = e - 24 * r;
    double q = r == c ? qd[r] : 0.0;
    if (Qa && r >= 12 && r < 15 && c >= 12 && c < 15) q = Qa[3 * (r - 12) + (c - 12)];
    P[e] = f_row(c, T + 24 * r, 1, E, a15, dt, B, Cm) + q;
  }
  __syncthreads();
}

__device__ __forceinline__ void pull_words(const uint4* __restrict__ src, uint4* __restrict__ dst, int from, int to, int lane, int lanes) {
  for (int i0 = from + lane; i0 < to; i0 += lanes * 4) {  // four PCIe reads in flight per lane
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = i0 + lanes * u < to ? src[i0 + lanes * u] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (i0 + lanes * u < to) dst[i0 + lanes * u] = v[u];
  }
}

// The end rotation of the constant-velocity model, rot_end * Exp(bias_g, dt) (:228, :241; in the CV model bias_g is the angular
// velocity).  cv_propagate_lds below takes the same two steps - exp_so3, then mat3_mul - on the same numbers: the same bits.
__device__ __forceinline__ void cv_end_rotation(const double* __restrict__ rot, const double* __restrict__ bias_g, double dt, double* __restrict__ out) {
  double E[9];
  exp_so3(bias_g, dt, E);
  mat3_mul(rot, E, out);
}

// LDS of one constant-velocity propagation: the state without its covariance, P, the scratch of cov_step, the two rotations, cov_w's diagonal
struct CvPropLds {
  double x[36], P[576], T[576], E[18], qd[24];  // E: Exp(bias_g, dt) | Exp(bias_g, -dt)
};
// Forward_propagation_without_imu, src/IMU_Processing.hpp:226-244, on a state that sits in LDS (L.x, L.P): every lane of a 256-lane
// workgroup calls it; on return L.x / L.P hold the propagated state and every lane may read them.
__device__ __forceinline__ void cv_propagate_lds(CvPropLds& L, double dt, const double* __restrict__ cov_gyr_scale, const double* __restrict__ cov_acc_scale) {
  const int tid = threadIdx.x;
  if (tid < 2) {  // Exp(bias_g, dt) and Exp(bias_g, -dt): in the CV model bias_g is the angular velocity (:226-229)
    double E[9];
    exp_so3(L.x + 27, tid == 0 ? dt : -dt, E);
#pragma unroll
    for (int e = 0; e < 9; e++) L.E[9 * tid + e] = E[e];
  }
  if (tid >= 64 && tid < 64 + 24) {  // :234-235
    const int r = tid - 64;
    double q = 0.0;
    if (r >= 15 && r < 18) q = cov_gyr_scale[r - 15] * dt * dt;
    else if (r >= 12 && r < 15) q = cov_acc_scale[r - 12] * dt * dt;
    L.qd[r] = q;
  }
  __syncthreads();
  cov_step(L.P, L.T, L.E + 9, dt, dt, nullptr, nullptr, L.qd, nullptr);
  if (tid == 0) {
    double Rn[9];
    mat3_mul(L.x, L.E, Rn);  // :241 (cv_end_rotation's two steps: lane 0 formed L.E[0..8] above)
#pragma unroll
    for (int e = 0; e < 9; e++) L.x[e] = Rn[e];
#pragma unroll
    for (int c = 0; c < 3; c++) L.x[9 + c] += L.x[24 + c] * dt;  // :244
  }
  __syncthreads();
}

}  // namespace lii

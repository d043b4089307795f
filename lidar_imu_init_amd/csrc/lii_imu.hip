// IMU processing of libliinit_hip for gfx950: the forward half of ImuProcess::Process on the device.  Reference code replaced:
//   k_imu_propagate  propagation_and_undist, src/IMU_Processing.hpp:292-382 (state, 24 x 24 covariance, IMUpose table, carry)
//   k_cv_propagate   Forward_propagation_without_imu, :212-244 (constant-velocity model of the LO phase)
// The back half - the de-skew over the IMUpose table, :390-414 - is k_deskew_imu* of lii_scan.hip, which reads the table this
// file leaves in device memory.
//
// STRUCTURE OF THE LAUNCH ("IMU forward propagation").  One launch of two workgroups per scan, never one per sample:
//   workgroup 0  the POSE chain: the ~20 dependent steps of 3 x 3 arithmetic that the de-skew waits for - IMUpose table, propagated
//                pose / velocity, the new carry - and, beside it, the pull of the update's control block out of pinned host memory
//                (what the extra workgroup of k_deskew_imu does on the host-fed path);
//   workgroup 1  the COVARIANCE chain: P <- F P F^T + Q over the same steps with P resident in LDS.  It needs nothing of the pose
//                chain but R_imu before every step, which it forms for itself (nine doubles per step, the same instructions: the same
//                bits), so neither workgroup ever waits for the other and the launch lasts max(pose, covariance) instead of their sum.  The de-skew
//                launch behind it on the stream still waits for BOTH workgroups, i.e. for the longer chain (the covariance's).
// What is serial in both chains is little: everything of a step that depends on its two samples alone - the mid-point rates, dt,
// Exp(w, dt), Exp(w, -dt): two sincos each - is computed by ONE LANE PER STEP up front, all steps at once; the chains then only
// multiply 3 x 3 matrices.  F_x = I + (blocks in rows 0-2, 3-5, 12-14): F P touches nine rows, (F P) F^T nine columns - each element
// of the result is a sum of at most eight products, one element per lane and phase, instead of two dense 24^3 products.
// This unit is built without FMA contraction (csrc/Makefile): the reference's x86-64 build has none either, and the sums below
// follow the order of its dense products over the non-zero terms.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "lii_device.h"
#include "lii_imu_dev.h"
#include "lii_launch.h"

namespace lii {

namespace {
constexpr double kGravity = 9.81;  // G_m_s2, include/common_lib.h:25
constexpr int kMaxSteps = 64;      // steps of one scan (n_imu <= 63: at most 64 poses)

// What a step needs from its two samples alone (lane `i` fills step i; :304-332).  v[0] = last_imu_, v[1 ..] = the scan's samples.
struct StepTab {
  int exec[kMaxSteps];          // 0: `continue` of :307
  double dt[kMaxSteps];
  double w[kMaxSteps * 3];      // angvel_avr - bias_g
  double a[kMaxSteps * 3];      // acc_avr / IMU_mean_acc_norm * G_m_s2 - bias_a
  double Ef[kMaxSteps * 9];     // Exp(angvel_avr, dt)
  double Em[kMaxSteps * 9];     // Exp(angvel_avr, -dt)   (covariance chain only)
};

template <bool COV>
__device__ __forceinline__ void fill_steps(StepTab& tb, const double* __restrict__ v /* (n + 1) x 7, LDS */, int n_steps, double last_end,
                                           const double* __restrict__ bias_g, const double* __restrict__ bias_a, double mean_acc_norm) {
  const int i = threadIdx.x;
  if (i < n_steps) {
    const double* head = v + 7 * i;
    const double* tail = v + 7 * (i + 1);
    const int exec = tail[0] < last_end ? 0 : 1;
    double w[3], a[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      w[c] = 0.5 * (head[1 + c] + tail[1 + c]);
      a[c] = 0.5 * (head[4 + c] + tail[4 + c]);
      w[c] -= bias_g[c];
      a[c] = a[c] / mean_acc_norm * kGravity - bias_a[c];
    }
    const double dt = head[0] < last_end ? tail[0] - last_end : tail[0] - head[0];  // :325-328
    double E[9];
    exp_so3(w, dt, E);
    tb.exec[i] = exec;
    tb.dt[i] = dt;
#pragma unroll
    for (int c = 0; c < 3; c++) { tb.w[3 * i + c] = w[c]; tb.a[3 * i + c] = a[c]; }
#pragma unroll
    for (int e = 0; e < 9; e++) tb.Ef[9 * i + e] = E[e];
    if (COV) {
      exp_so3(w, -dt, E);
#pragma unroll
      for (int e = 0; e < 9; e++) tb.Em[9 * i + e] = E[e];
    }
  }
}

}  // namespace

__global__ __launch_bounds__(256) void k_imu_propagate(ImuPropArgs io) {
  __shared__ double s_v[(kMaxSteps + 1) * 7];  // last_imu_ | the scan's samples
  __shared__ double s_x[36];                   // the state without its covariance
  __shared__ double s_carry[16];
  __shared__ StepTab tb;
  const int tid = threadIdx.x;
  const int n = io.n_imu;  // steps: (v[i], v[i + 1]), i < n
  // ---- both workgroups: the inputs (pinned host memory / device memory) -> LDS in one round trip
  for (int e = tid; e < 7 * n; e += 256) s_v[7 + e] = io.samples[e];
  if (tid < 36) s_x[tid] = io.st_in[tid];
  if (tid >= 64 && tid < 64 + 15) s_carry[tid - 64] = io.carry_in[tid - 64];
  __syncthreads();
  if (tid < 7) s_v[tid] = s_carry[tid];
  __syncthreads();
  const double last_end = s_carry[13];
  const double* bias_g = s_x + 27;
  const double* bias_a = s_x + 30;
  if (blockIdx.x == 0) {
    // ============================================================ the pose chain
    fill_steps<false>(tb, s_v, n, last_end, bias_g, bias_a, io.noise[18]);
    __syncthreads();
    if (tid >= 64) {  // three wavefronts bring the update's control block over (everything behind the two states, which this launch writes)
      if (io.ctrl_vec > 0) pull_words(io.ctrl_src, io.ctrl_dst, io.ctrl_from, io.ctrl_vec, tid - 64, 192);
      return;
    }
    if (tid != 0) return;
    double pcl_end_time = io.pcl_end_time;
    if (io.scan) {  // :288 - the sweep ends with the point of the largest time stamp (a sorted scan: its last)
      const float t_last = io.sorted ? io.scan[io.n_scan - 1].w : ord2f((unsigned)io.extent[1]);
      pcl_end_time = io.pcl_beg_time + t_last / double(1000);
    }
    const double imu_end_time = s_v[7 * n];
    double R[9], vel[3], pos[3], acc_imu[3] = {0, 0, 0}, w_last[3] = {0, 0, 0};
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = s_x[e];
#pragma unroll
    for (int c = 0; c < 3; c++) { pos[c] = s_x[9 + c]; vel[c] = s_x[24 + c]; }
    const double* grav = s_x + 33;
    double acc_s_last[3] = {s_carry[7], s_carry[8], s_carry[9]}, angvel_last[3] = {s_carry[10], s_carry[11], s_carry[12]};
    int K = 0;
    auto set_pose = [&](double t, const double* acc, const double* gyr) {  // set_pose6d, include/common_lib.h:183-199
      double* p = io.poses + 22 * K;
      p[0] = t;
#pragma unroll
      for (int c = 0; c < 3; c++) { p[1 + c] = acc[c]; p[4 + c] = gyr[c]; p[7 + c] = vel[c]; p[10 + c] = pos[c]; }
#pragma unroll
      for (int e = 0; e < 9; e++) p[13 + e] = R[e];
      K++;
    };
    set_pose(0.0, acc_s_last, angvel_last);  // :294
    for (int i = 0; i < n; i++) {
      if (!tb.exec[i]) continue;
      const double dt = tb.dt[i];
      double Rn[9], Ra[3];
      mat3_mul(R, tb.Ef + 9 * i, Rn);  // :355
#pragma unroll
      for (int e = 0; e < 9; e++) R[e] = Rn[e];
      const double a[3] = {tb.a[3 * i], tb.a[3 * i + 1], tb.a[3 * i + 2]};
      mat3_vec(R, a, Ra);
#pragma unroll
      for (int c = 0; c < 3; c++) {
        acc_imu[c] = Ra[c] + grav[c];                                       // :358
        pos[c] = pos[c] + vel[c] * dt + 0.5 * acc_imu[c] * dt * dt;         // :361
        vel[c] = vel[c] + acc_imu[c] * dt;                                  // :364
        w_last[c] = tb.w[3 * i + c];
        angvel_last[c] = w_last[c];                                         // :367
        acc_s_last[c] = acc_imu[c];                                         // :368
      }
      set_pose(s_v[7 * (i + 1)] - io.pcl_beg_time, acc_imu, w_last);        // :369-370
    }
    // ---- the prediction at the frame end (:374-378)
    const double note = pcl_end_time > imu_end_time ? 1.0 : -1.0;
    const double dt = note * (pcl_end_time - imu_end_time);
    const double w_end[3] = {note * w_last[0], note * w_last[1], note * w_last[2]};
    double E[9], Rend[9], x[36];
    exp_so3(w_end, dt, E);
    mat3_mul(R, E, Rend);
#pragma unroll
    for (int e = 0; e < 36; e++) x[e] = s_x[e];
#pragma unroll
    for (int e = 0; e < 9; e++) x[e] = Rend[e];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      x[24 + c] = vel[c] + note * acc_imu[c] * dt;
      x[9 + c] = pos[c] + note * vel[c] * dt + note * 0.5 * acc_imu[c] * dt * dt;
    }
#pragma unroll
    for (int e = 0; e < 36; e++) {
      io.st_out[e] = x[e];
      if (io.prop_out) io.prop_out[e] = x[e];
      if (io.host_out) io.host_out[e] = x[e];
    }
    // ---- the carry (:367-368, :381-382)
    double cn[15];
#pragma unroll
    for (int e = 0; e < 7; e++) cn[e] = s_v[7 * n + e];
#pragma unroll
    for (int c = 0; c < 3; c++) { cn[7 + c] = acc_s_last[c]; cn[10 + c] = angvel_last[c]; }
    cn[13] = pcl_end_time;
    cn[14] = 0.0;
#pragma unroll
    for (int e = 0; e < 15; e++) {
      io.carry_out[e] = cn[e];
      if (io.host_out) io.host_out[kStateDoubles + e] = cn[e];
    }
    *io.n_poses = K;
    if (io.host_out) io.host_out[kStateDoubles + 15] = double(K);
    return;
  }
  // ============================================================== the covariance chain
  __shared__ double s_P[576], s_T[576];
  __shared__ double s_R[kMaxSteps * 9];                            // R_imu BEFORE step i
  __shared__ double s_B[kMaxSteps * 9], s_C[kMaxSteps * 9], s_Qa[kMaxSteps * 9];
  __shared__ double s_qd[24];
  for (int e = tid; e < 576; e += 256) s_P[e] = io.st_in[36 + e];
  fill_steps<true>(tb, s_v, n, last_end, bias_g, bias_a, io.noise[18]);
  __syncthreads();
  if (tid == 0) {  // the rotation chain, as workgroup 0 forms it (:355)
    double R[9];
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = s_x[e];
    for (int i = 0; i < n; i++) {
#pragma unroll
      for (int e = 0; e < 9; e++) s_R[9 * i + e] = R[e];
      if (!tb.exec[i]) continue;
      double Rn[9];
      mat3_mul(R, tb.Ef + 9 * i, Rn);
#pragma unroll
      for (int e = 0; e < 9; e++) R[e] = Rn[e];
    }
  }
  __syncthreads();
  if (tid < n && tb.exec[tid]) {  // the blocks of F_x and cov_w that hold R_imu (:341-342, :348), one lane per step
    const int i = tid;
    const double dt = tb.dt[i];
    const double* R = s_R + 9 * i;
    const double ax = tb.a[3 * i], ay = tb.a[3 * i + 1], az = tb.a[3 * i + 2];
    const double Ks[9] = {0.0, -az, ay, az, 0.0, -ax, -ay, ax, 0.0};  // SKEW_SYM_MATRX(acc_avr)
    double RK[9], RD[9], Rt[9], RDRt[9];
    mat3_mul(R, Ks, RK);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) { RD[3 * r + c] = R[3 * r + c] * io.noise[3 + c]; Rt[3 * r + c] = R[3 * c + r]; }
    mat3_mul(RD, Rt, RDRt);
#pragma unroll
    for (int e = 0; e < 9; e++) {
      s_B[9 * i + e] = -RK[e] * dt;
      s_C[9 * i + e] = -R[e] * dt;
      s_Qa[9 * i + e] = RDRt[e] * dt * dt;
    }
  }
  __syncthreads();
  for (int i = 0; i < n; i++) {
    if (!tb.exec[i]) continue;  // (uniform)
    const double dt = tb.dt[i];
    if (tid < 24) {  // the diagonal of cov_w (:345-350)
      const int g = tid / 3, c = tid - 3 * g;
      double q = 0.0;
      if (g == 0) q = io.noise[0 + c] * dt * dt;         // cov_gyr
      else if (g == 2) q = io.noise[12 + c] * dt * dt;   // cov_R_LI
      else if (g == 3) q = io.noise[15 + c] * dt * dt;   // cov_T_LI
      else if (g == 5) q = io.noise[6 + c] * dt * dt;    // cov_bias_gyr
      else if (g == 6) q = io.noise[9 + c] * dt * dt;    // cov_bias_acc
      s_qd[tid] = q;
    }
    // (the first barrier inside cov_step also orders s_qd in front of its readers)
    cov_step(s_P, s_T, tb.Em + 9 * i, -dt, dt, s_B + 9 * i, s_C + 9 * i, s_qd, s_Qa + 9 * i);
  }
  for (int e = tid; e < 576; e += 256) {
    io.st_out[36 + e] = s_P[e];
    if (io.host_out) io.host_out[36 + e] = s_P[e];
  }
}

// Forward_propagation_without_imu, src/IMU_Processing.hpp:212-244, without its de-skew (k_deskew_cv): one workgroup.  The arithmetic
// is cv_propagate_lds (lii_imu_dev.h), which the extra workgroup of k_deskew_cv_prop (lii_scan.hip) runs as well.
__global__ __launch_bounds__(256) void k_cv_propagate(CvPropArgs io) {
  __shared__ CvPropLds L;
  const int tid = threadIdx.x;
  if (tid < 36) L.x[tid] = io.st_in[tid];
  for (int e = tid; e < 576; e += 256) L.P[e] = io.st_in[36 + e];
  __syncthreads();
  cv_propagate_lds(L, io.dt, io.cov_gyr_scale, io.cov_acc_scale);
  if (tid < 36) { io.st_out[tid] = L.x[tid]; if (io.host_out) io.host_out[tid] = L.x[tid]; }
  for (int e = tid; e < 576; e += 256) { io.st_out[36 + e] = L.P[e]; if (io.host_out) io.host_out[36 + e] = L.P[e]; }
}

void launch_imu_propagate(const ImuPropArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_imu_propagate, dim3(2), dim3(256), 0, s, a); }
void launch_cv_propagate(const CvPropArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_cv_propagate, dim3(1), dim3(256), 0, s, a); }

}  // namespace lii

// libliinit_hip — IMU processing (host side): lii_imu_noise_defaults / lii_imu_set_noise / lii_imu_set_carry / lii_imu_get_carry,
// lii_imu_propagate, lii_cv_propagate, lii_scan_register_imu, lii_scan_register_cv.  Kernels: lii_imu.hip, and k_deskew_cv_prop of lii_scan.hip.  Reference: ImuProcess::Process,
// src/IMU_Processing.hpp:419-461 (its forward half; the de-skew is lii_undistort_* / k_deskew_*).  The prologue of
// lii_scan_register_imu lives with the routine it shares with lii_scan_register (lii_capi_register.cpp: imu_prologue).
#include "lii_context.h"

using namespace lii_impl;

namespace lii_impl {

int imu_buffers(lii_handle h) {
  if (h->imu.d_buf) return LII_OK;
  HIPCHK(h, h->imu.d_buf.alloc(2 * lii::kImuCarryDoubles + 8 + kStateDoubles));
  HIPCHK(h, hipMemsetAsync(h->imu.d_buf, 0, sizeof(double) * h->imu.d_buf.size(), h->stream));
  HIPCHK(h, h->imu.h_in.alloc(kStateDoubles + 64 * 7, hipHostMallocDefault));
  HIPCHK(h, h->imu.h_out.alloc(kStateDoubles + lii::kImuCarryDoubles, hipHostMallocMapped));
  return LII_OK;
}

}  // namespace lii_impl

namespace {

// what every entry point that propagates checks first (include/liinit_hip.h, "Rules")
int check_feed(lii_handle h, const char* who, const lii_imu_sample* imu, int32_t n_imu) {
  if (!imu || n_imu < 1) return fail(h, LII_ERR_INVALID, std::string(who) + ": no IMU samples (the reference returns untouched when meas.imu is empty)");
  static_assert(kImuSamplesMax == 63, "the message names the limit");
  if (n_imu > kImuSamplesMax) return fail(h, LII_ERR_CAPACITY, std::string(who) + ": more than 63 IMU samples (64 poses) in one scan");
  if (!h->imu.have_noise) return fail(h, LII_ERR_STATE, std::string(who) + ": no noise block (lii_imu_set_noise)");
  if (!h->imu.have_carry) return fail(h, LII_ERR_STATE, std::string(who) + ": no carry (lii_imu_set_carry)");
  if (h->net.comm || h->net.n_ranks > 1) return fail(h, LII_ERR_STATE, std::string(who) + ": single rank only for now (a communicator is attached)");
  return LII_OK;
}

}  // namespace

extern "C" {

// ImuProcess::ImuProcess(), src/IMU_Processing.hpp:97-102; mean_acc_norm: main() installs initialization/mean_acc_norm (lii_params_defaults)
int lii_imu_noise_defaults(lii_imu_noise* out) {
  if (!out) return LII_ERR_INVALID;
  std::memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(lii_imu_noise);
  for (int a = 0; a < 3; a++) {
    out->cov_acc[a] = 0.1;
    out->cov_gyr[a] = 0.1;
    out->cov_R_LI[a] = 0.00001;
    out->cov_T_LI[a] = 0.0001;
    out->cov_bias_gyr[a] = 0.0001;
    out->cov_bias_acc[a] = 0.0001;
  }
  lii_params p;
  const int rc = lii_params_defaults(&p);
  if (rc != LII_OK) return rc;
  out->mean_acc_norm = p.mean_acc_norm;
  return LII_OK;
}

int lii_imu_set_noise(lii_handle h, const lii_imu_noise* noise) {
  if (!h || !noise || noise->struct_size != sizeof(lii_imu_noise)) return fail(h, LII_ERR_INVALID, "lii_imu_set_noise: bad arguments");
  if (!(noise->mean_acc_norm > 0)) return fail(h, LII_ERR_INVALID, "lii_imu_set_noise: mean_acc_norm must be positive");
  h->imu.noise = *noise;
  h->imu.have_noise = true;
  return LII_OK;
}

int lii_imu_set_carry(lii_handle h, const lii_imu_carry* carry) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !carry) return fail(h, LII_ERR_INVALID, "lii_imu_set_carry: bad arguments");
  static_assert(sizeof(lii_imu_carry) == 14 * sizeof(double) && sizeof(lii_imu_sample) == 7 * sizeof(double), "carry layout");
  int rc = imu_buffers(h);
  if (rc != LII_OK) return rc;
  // (synchronous: set on the hand-over scans only; the copy is ordered behind a propagation still under way)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(h->imu.d_carry(h->imu.carry_sel), carry, sizeof(lii_imu_carry), hipMemcpyHostToDevice));
  h->imu.have_carry = true;
  return LII_OK;
}

int lii_imu_get_carry(lii_handle h, lii_imu_carry* out) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !out) return fail(h, LII_ERR_INVALID, "lii_imu_get_carry: bad arguments");
  if (!h->imu.have_carry) return fail(h, LII_ERR_STATE, "lii_imu_get_carry: no carry (lii_imu_set_carry)");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(out, h->imu.d_carry(h->imu.carry_sel), sizeof(lii_imu_carry), hipMemcpyDeviceToHost));
  return LII_OK;
}

int lii_imu_propagate(lii_handle h, const lii_imu_sample* imu, int32_t n_imu, double pcl_beg_time, double pcl_end_time, lii_state* state,
                      lii_pose6d* poses_out, int32_t capacity, int32_t* n_poses) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !state || !poses_out || !n_poses) return fail(h, LII_ERR_INVALID, "lii_imu_propagate: bad arguments");
  int rc = check_feed(h, "lii_imu_propagate", imu, n_imu);
  if (rc != LII_OK) return rc;
  if (capacity < n_imu + 1) return fail(h, LII_ERR_CAPACITY, "lii_imu_propagate: poses_out holds fewer than n_imu + 1 records");
  rc = imu_buffers(h);
  if (rc != LII_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (the staging buffers below and the pose table on the device are free)
  std::memcpy(h->imu.h_in, state, sizeof(lii_state));
  std::memcpy(h->imu.h_in + kStateDoubles, imu, sizeof(lii_imu_sample) * size_t(n_imu));
  lii::ImuPropArgs a = {};
  a.st_in = h->imu.h_in;
  a.samples = h->imu.h_in + kStateDoubles;
  a.n_imu = n_imu;
  std::memcpy(a.noise, h->imu.noise.cov_gyr, sizeof(a.noise));
  a.pcl_beg_time = pcl_beg_time;
  a.pcl_end_time = pcl_end_time;
  a.carry_in = h->imu.d_carry(h->imu.carry_sel);
  a.carry_out = h->imu.d_carry(h->imu.carry_sel ^ 1);
  a.poses = h->d_poses;
  a.n_poses = h->imu.d_n_poses();
  a.st_out = h->imu.d_state();
  a.host_out = h->imu.h_out;
  launch_imu_propagate(a, h->stream);
  HIPCHK(h, hipGetLastError());
  h->imu.carry_sel ^= 1;  // (only behind a launch that went out: a failed one leaves the current carry the current one)
  lii_pose6d* stage = h->h_small->imu_poses;  // (pinned, kImuSamplesMax + 1 poses: check_feed; this call ends with a synchronisation)
  HIPCHK(h, hipMemcpyAsync(stage, h->d_poses, sizeof(lii_pose6d) * size_t(n_imu + 1), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int K = int(h->imu.h_out[kStateDoubles + 15]);
  if (K < 1 || K > n_imu + 1) return fail(h, LII_ERR_HIP, "lii_imu_propagate: the launch left no pose count");
  std::memcpy(state, h->imu.h_out.get(), sizeof(lii_state));
  std::memcpy(poses_out, stage, sizeof(lii_pose6d) * size_t(K));
  *n_poses = K;
  return LII_OK;
}

int lii_cv_propagate(lii_handle h, double dt, const double cov_gyr_scale[3], const double cov_acc_scale[3], lii_state* state) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !cov_gyr_scale || !cov_acc_scale || !state) return fail(h, LII_ERR_INVALID, "lii_cv_propagate: bad arguments");
  if (h->net.comm || h->net.n_ranks > 1) return fail(h, LII_ERR_STATE, "lii_cv_propagate: single rank only for now (a communicator is attached)");
  int rc = imu_buffers(h);
  if (rc != LII_OK) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::memcpy(h->imu.h_in, state, sizeof(lii_state));
  lii::CvPropArgs a = {};
  a.st_in = h->imu.h_in;
  a.dt = dt;
  std::memcpy(a.cov_gyr_scale, cov_gyr_scale, 24);
  std::memcpy(a.cov_acc_scale, cov_acc_scale, 24);
  a.st_out = h->imu.d_state();
  a.host_out = h->imu.h_out;
  launch_cv_propagate(a, h->stream);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::memcpy(state, h->imu.h_out.get(), sizeof(lii_state));
  return LII_OK;
}

int lii_scan_register_imu(lii_handle h, const lii_scan_job* job, const lii_imu_sample* imu, int32_t n_imu, double pcl_beg_time, lii_state* state,
                          lii_state* state_propagated_out, lii_iekf_report* report) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !job || !state) return fail(h, LII_ERR_INVALID, "lii_scan_register_imu: bad arguments");
  if (job->struct_size != sizeof(lii_scan_job) && job->struct_size != 72u && job->struct_size != 56u && job->struct_size != 48u)
    return fail(h, LII_ERR_INVALID, "lii_scan_register_imu: bad job size");
  if (job->undistort != 1 || job->imu_poses != nullptr || job->n_imu_poses != 0)
    return fail(h, LII_ERR_INVALID, "lii_scan_register_imu: the job must say undistort = 1, imu_poses = NULL, n_imu_poses = 0 (the pose table is formed on the device)");
  const int rc = check_feed(h, "lii_scan_register_imu", imu, n_imu);
  if (rc != LII_OK) return rc;
  if (h->host_solve) return fail(h, LII_ERR_STATE, "lii_scan_register_imu: not available under LII_TEST=host_solve (the host-driven loop has no device-resident control block)");
  ImuFeed feed = {imu, n_imu, pcl_beg_time, state_propagated_out};
  return scan_register_job(h, job, state, nullptr, report, &feed);
}

// Process() with imu_en == false (src/IMU_Processing.hpp:212-266) + the per-scan sequence: the propagation rides in the de-skew launch
int lii_scan_register_cv(lii_handle h, const lii_scan_job* job, double dt, const double cov_gyr_scale[3], const double cov_acc_scale[3], lii_state* state,
                         lii_state* state_propagated_out, lii_iekf_report* report) {
  lii_internal_prearm_cancel(h);  // (a pre-armed de-skew launch waiting on the stream is told to end: this entry point uses the stream)
  if (!h || !job || !state || !cov_gyr_scale || !cov_acc_scale) return fail(h, LII_ERR_INVALID, "lii_scan_register_cv: bad arguments");
  if (job->struct_size != sizeof(lii_scan_job) && job->struct_size != 72u && job->struct_size != 56u && job->struct_size != 48u)
    return fail(h, LII_ERR_INVALID, "lii_scan_register_cv: bad job size");
  if (job->undistort != 2 || job->imu_poses != nullptr || job->n_imu_poses != 0)
    return fail(h, LII_ERR_INVALID, "lii_scan_register_cv: the job must say undistort = 2, imu_poses = NULL, n_imu_poses = 0");
  if (!std::isfinite(dt)) return fail(h, LII_ERR_INVALID, "lii_scan_register_cv: dt is not finite");
  if (h->net.comm || h->net.n_ranks > 1) return fail(h, LII_ERR_STATE, "lii_scan_register_cv: single rank only for now (a communicator is attached)");
  if (h->host_solve) return fail(h, LII_ERR_STATE, "lii_scan_register_cv: not available under LII_TEST=host_solve (the host-driven loop has no device-resident control block)");
  if (h->no_fast_prologue) {
    // LII_TEST=no_fast: no launch carries anything along - k_cv_propagate, then lii_scan_register's general path (the same device code on the
    // same numbers: the same results).  A copy is propagated: `state` changes only with a successful update.
    const bool have_scan = (job->scan_dev != nullptr && job->n_scan_dev > 0) || h->n_scan > 0 || lii_internal_scan_is_deferred(h);
    if (!have_scan) return fail(h, LII_ERR_STATE, "lii_scan_register_cv: no scan (lii_scan_upload / lii_frame_select / lii_scan_job::scan_dev)");
    std::vector<lii_state> st(2, *state);
    int rc = lii_cv_propagate(h, dt, cov_gyr_scale, cov_acc_scale, &st[0]);
    if (rc != LII_OK) return rc;
    st[1] = st[0];
    lii_scan_job plain = {};
    std::memcpy(&plain, job, job->struct_size);
    if (plain.struct_size >= 72u) { plain.next_scan_dev = nullptr; plain.next_n_scan = 0; }
    rc = scan_register_job(h, &plain, &st[1], &st[0], report, nullptr);
    if (rc != LII_OK) return rc;
    *state = st[1];
    if (state_propagated_out) *state_propagated_out = st[0];
    return LII_OK;
  }
  CvFeed cv = {dt, cov_gyr_scale, cov_acc_scale, state_propagated_out};
  return scan_register_job(h, job, state, nullptr, report, nullptr, &cv);
}

}  // extern "C"

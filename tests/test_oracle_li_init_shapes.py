"""CPU companion of tests/test_gpu_li_init_shapes.py: what its references and bounds rest on, checked without a GPU.

  * the mpmath reference (li_init_shapes.mp_terms: residuals of the three cost functors, finite-difference Jacobians at a step
    of 1e-20, 60 digits) against the numpy oracle's analytic Jacobians - a check of the reference, not of the kernel;
  * the float64 numpy oracle within a quarter of the derived bound at n = 1, 65, 257, all stages and parameter points: the
    inputs do not cancel so much that the bound's per-term count c would be meaningless;
  * the inputs of the cross-correlation cases put the winner where the GPU test says they do;
  * the synthetic solver problem is recovered by the oracle, and by how much.
"""
import numpy as np
import pytest

import li_init_shapes as S

CASES = [(stage, n, k) for stage in (1, 2, 3) for n in S.MP_SIZES for k in range(3)]


@pytest.mark.parametrize("stage,n,k", CASES)
def test_oracle_within_a_quarter_of_the_bound(stage, n, k):
    """The oracle's float64 terms of every sample, summed in the kernel's order (one lane per residue mod 256, then the tree over
    256 lanes - the order the bound's ceil(n / 256) + 8 counts), stay within a quarter of the bound.

    LI.normal_equations on the whole set does NOT stay within a quarter, in any stage, once n > 1: it adds the n samples one
    after the other, where the bound counts ceil(n / 256) + 8 additions.  Measured, whole set / same terms in the kernel's order
    (range over the three parameter points):
                  n = 1                       n = 65                      n = 257
      stage 1     0.05 - 0.13 / 0.05 - 0.13   0.21 - 0.29 / 0.02 - 0.05   0.09 - 0.51 / 0.04 - 0.06
      stage 2     0.07 - 0.19 / 0.07 - 0.19   0.15 - 0.20 / 0.03 - 0.06   0.32 - 0.46 / 0.03 - 0.06
      stage 3     0.05 - 0.11 / 0.05 - 0.11   0.35 - 0.51 / 0.04 - 0.04   1.23 - 1.30 / 0.04 - 0.06
    The worst entries are sums of n terms of one sign (stage 3: the gravity block, n EQUAL terms whose roundings share a sign;
    stages 1 / 2: the diagonal of J^T J), where a serial sum's error grows with n whatever the inputs are: it is the oracle's
    order of additions, not cancellation in the inputs, so other inputs do not change it.  The whole-set call is printed and
    held to a quarter of the same bound with n - 1 additions in place of ceil(n / 256) + 8."""
    from oracle import li_init_np as LI
    imu, lid, (R, v, R_LI), exact, mag = S.reference(stage, n, k)
    in_order = S.kernel_order_sum(S.oracle_sample_terms(stage, R, v, R_LI, imu, lid))
    ratio = S.worst_ratio(stage, n, in_order, exact, mag)
    whole = S.flat(*LI.normal_equations(stage, R, v, imu, lid, R_LI))
    ratio_whole = S.worst_ratio(stage, n, whole, exact, mag)
    print(f"stage {stage} n {n} point {k}: oracle / bound = {ratio:.3f} (kernel's order), {ratio_whole:.3f} (serial over n)")
    assert ratio <= 0.25
    serial = (n - 1 + S.C_ROUNDINGS[stage]) / (-(-n // 256) + 8 + S.C_ROUNDINGS[stage])  # the same bound with n - 1 additions
    assert ratio_whole <= 0.25 * max(1.0, serial)


@pytest.mark.parametrize("stage", (1, 2, 3))
def test_reference_jacobian_against_the_analytic_one(stage):
    """J^T J, J^T r and the cost from the finite-difference reference equal the oracle's analytic ones to float64 accuracy
    (1e-13 of the largest entry: n = 65 serial float64 additions), and the difference quotient does not depend on its step."""
    from oracle import li_init_np as LI
    imu, lid, (R, v, R_LI), exact, _ = S.reference(stage, 65, 0)
    got = S.flat(*LI.normal_equations(stage, R, v, imu, lid, R_LI))
    want = np.array([float(e) for e in exact])
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    sl = slice(0, 3)
    _, J20 = S.mp_sample_terms(stage, R, v, R_LI, imu.slice(sl), lid.slice(sl), step="1e-20")
    _, J15 = S.mp_sample_terms(stage, R, v, R_LI, imu.slice(sl), lid.slice(sl), step="1e-15")
    d = max(abs(a - b) for Ja, Jb in zip(J20, J15) for ra, rb in zip(Ja, Jb) for a, b in zip(ra, rb))
    assert d < 1e-25  # truncation ~ step^2


def test_inputs_are_what_the_issue_asks():
    imu, lid = S.random_pair(257, seed=11)
    dT = lid.t - imu.t
    assert np.all(np.abs(dT) >= 0.01) and np.all(np.abs(dT) <= 0.05) and (dT > 0).any() and (dT < 0).any()
    assert np.allclose(np.einsum("nij,nkj->nik", lid.rot_end, lid.rot_end), np.eye(3), atol=1e-14)
    assert np.allclose(np.linalg.det(lid.rot_end), 1.0)
    tds = [p[1][3] for p in S.param_points(2)]
    assert min(tds) < 0 < max(tds)
    for stage in (1, 2, 3):
        for R, v, R_LI in S.param_points(stage):
            assert np.arccos((np.trace(R) - 1) / 2) > 0.3  # not the near-identity rotation
    for n_seq, n in S.ZERO_PHASE_CASES:
        b = S.filter_batch(n_seq, n)
        ch = b[:, :, 9:21].transpose(0, 2, 1).reshape(-1, n)
        assert len({c.tobytes() for c in ch}) == n_seq * 12  # every sequence and channel its own signal


def test_cross_correlation_cases_put_the_winner_where_intended():
    """The oracle (np.correlate + argmax) and the library's order of additions (ascending i, strict >) agree on every case, and
    the boundary cases win at k = 255, 256, 257, 511, 512."""
    from oracle import li_init_np as LI
    n = S.BOUNDARY_N
    for k in S.BOUNDARY_K:
        a, b = S.windowed_pair(n, k - (n - 1))
        lag = LI.xcorr_temporal_init(a, b, 50.0)[1]
        assert (n - 1) - lag == k and S.xcorr_host_order(a, b) == (lag, k)
    a, b = S.plateau_pair()
    assert LI.xcorr_temporal_init(a, b, 50.0)[1] == n - 1 == S.xcorr_host_order(a, b)[0]
    assert LI.xcorr_temporal_init(b, a, 50.0)[1] == n - 1 == S.xcorr_host_order(b, a)[0]
    a, b = S.plateau_pair(peak=True)  # a plateau below a peak, in both roles: >= 256 lags tie strictly under a unique maximum
    for x, y in ((a, b), (b, a)):
        corr = S.xcorr_values_host_order(x, y)
        values, counts = np.unique(corr, return_counts=True)
        assert counts.max() >= 256 and values[np.argmax(counts)] < corr.max() and np.sum(corr == corr.max()) == 1
        # lanes of the 256-lane argmax meet in its tree with equal values: lane t's best over k = t, t + 256, t + 512
        lane_best = np.array([corr[t::256].max() for t in range(256)])
        assert np.sum(lane_best == values[np.argmax(counts)]) >= 64
        assert LI.xcorr_temporal_init(x, y, 50.0)[1] == S.xcorr_host_order(x, y)[0] != n - 1
    for nn, shift in S.ROLLED_CASES:
        if nn <= 129:
            a, b = S.rolled_pair(nn, shift, seed=4)
            assert LI.xcorr_temporal_init(a, b, 50.0)[1] == S.xcorr_host_order(a, b)[0]


def test_oracle_recovers_the_synthetic_calibration():
    """Measured (n = 700, noise 1e-3): rotation 2.0e-4 rad, b_g 7.0e-5, t_d 8.2e-7 s, T_LI 3.3e-5 m, acc_bias 9.5e-4,
    grav_L0 4.9e-4; 4 / 3 / 4 iterations.  Bounds here: ten times the noise (the estimate averages 700 samples; acc_bias
    and gravity are the weakly separated pair)."""
    o = S.oracle_solution()
    print("oracle recovery error:", o["err"], "iterations:", [o[s]["iterations"] for s in ("s1", "s2", "s3")])
    assert all(e < 1e-2 for e in o["err"].values())
    assert o["err"]["rot_rad"] < 1e-3 and o["err"]["t_d"] < 1e-4


def test_short_accumulation_lengths():
    """The second zero-phase filter of the short li_init_run cases sees 61 states (shift 108: under the device filter's 62, the
    least the host filter can read) and 58 (shift 112: the oracle's filter indexes out of bounds)."""
    from oracle import li_init_np as LI
    imu, lid = S.short_accumulation(108)
    out = LI.li_initialization(imu, lid, 10, 5, solve=False)
    assert out["lag_frames"] == -108 and len(out["imu_meas"]) == 61
    imu, lid = S.short_accumulation(112)
    with pytest.raises(IndexError):
        LI.li_initialization(imu, lid, 10, 5, solve=False)

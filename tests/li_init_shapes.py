"""Inputs, an independent high-precision reference and the derived error bound shared by tests/test_oracle_li_init_shapes.py
(CPU) and tests/test_gpu_li_init_shapes.py (GPU) - the LI-Init device code at sizes and inputs beyond the reference's one run.

The reference (mp_terms) is written from the three cost functors of include/LI_init/LI_init.h:91-205 in mpmath at 60 digits:
the residual is evaluated directly, its Jacobian is a central difference of that residual in the tangent convention
R <- Exp(delta) R at a step of 1e-20 (truncation ~1e-40 relative), and the sums are formed at the same precision.  It shares
no analytic Jacobian with the kernel or with oracle/li_init_np.py.

The bound per output entry of k_calib_eval (bound()):

    |got - exact| <= (ceil(n / 256) + 8 + c) * 2^-53 * sum_i mag_i

  ceil(n / 256)  a lane's serial sum over its samples (i = lane, lane + 256, ...)
  8              the depth of the tree over 256 lanes
  c              the roundings inside one sample's term, counted on the kernel's longest chain, first order: a product
                 carries the relative errors of both factors plus its own rounding, and the three products of a term
                 (a = 0, 1, 2) are joined by two additions.
                   R v (mat3_vec): multiply, add, add = 3
                   stage 1: r = R w_L - w_I = 3 + 1 = 4; J = -[R w_L]x = 3; the longest term is the cost
                            0.5 (r.r): 4 + 4 + 1 + 2 = 11                                                       c = 11
                   stage 2: (dT + t_d) alpha = 1 + 1 + 1 = 3; r = (R w_L - w_I) - that + b_g = max(4, 3) + 1 + 1 = 6;
                            cost: 6 + 6 + 1 + 2 = 15                                                            c = 15
                   stage 3: W W = 3, + A = 4, R_LL0 M = 7 (= J's longest entry), (R_LL0 M) T_IL = 10;
                            r = t1 - R b_a + R g - a_L - RM T: four more = 14; cost: 14 + 14 + 1 + 2 = 31       c = 31
                 (the multiplication by 0.5 is exact.)
  mag_i          sample i's contribution to the entry with the three products taken in magnitude, from the reference:
                 sum_a |J_ak| |J_al|, sum_a |J_ak| |r_a|, 0.5 sum_a r_a^2.  The three products are taken in magnitude because
                 they cancel by construction where the Jacobian holds a rotation (stage 3: R_LL0^T R_LL0 = I, so the
                 off-diagonal entries of that block are rounding noise about zero for every proper rotation).  Cancellation
                 INSIDE r is not covered by c; the CPU test shows the float64 oracle's terms, added in the kernel's order,
                 within a quarter of the bound on these very inputs, which is the guard against inputs that cancel too much.
"""
import math

import numpy as np

EVAL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4099)
MP_SIZES = (1, 65, 257)
C_ROUNDINGS = {1: 11, 2: 15, 3: 31}
DOF = {1: 3, 2: 7, 3: 9}
U = 2.0 ** -53


def _LI():
    from oracle import li_init_np as LI
    return LI


def rand_rot(rng):
    q = rng.normal(size=4)
    return _LI().quat_to_rot(q / np.linalg.norm(q))


def random_pair(n, seed):
    """A seeded IMU / LiDAR CalibSeq pair of n samples: proper random rot_end, order-1 vectors, IMU stamps 0.01 - 0.05 s off the
    LiDAR's with both signs (dT of stage 2 non-zero and different per sample)."""
    LI = _LI()
    rng = np.random.default_rng([seed, n])
    imu, lid = LI.CalibSeq(n), LI.CalibSeq(n)
    for s in (imu, lid):
        s.rot_end = np.stack([rand_rot(rng) for _ in range(n)])
        for f in LI.CalibSeq.FIELDS4:
            setattr(s, f, rng.normal(0, 1.0, (n, 3)))
    lid.t = 100.0 + 0.02 * np.arange(n) + rng.uniform(-0.002, 0.002, n)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 if n == 1 else rng.choice([-1.0, 1.0]))
    imu.t = lid.t + sign * rng.uniform(0.01, 0.05, n)
    return imu, lid


def param_points(stage, seed=5):
    """Three seeded parameter points of a stage: (R, v, R_LI or None); random rotations, non-zero b_g, t_d of both signs."""
    rng = np.random.default_rng([seed, stage])
    pts = []
    for k in range(3):
        R = rand_rot(rng)
        if stage == 1:
            pts.append((R, np.zeros(0), None))
        elif stage == 2:
            td = (0.03, -0.02, 0.011)[k]
            pts.append((R, np.r_[rng.normal(0, 0.05, 3), td], None))
        else:
            pts.append((R, np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)], rand_rot(rng)))
    return pts


def pack_params(stage, R, v, R_LI):
    p = np.r_[R.reshape(-1), v]
    return np.r_[p, R_LI.reshape(-1)] if stage == 3 else p


# ------------------------------------------------------------------------------------------------ mpmath reference
def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath


def _mv(M, v):
    return [M[a][0] * v[0] + M[a][1] * v[1] + M[a][2] * v[2] for a in range(3)]


def _mm(A, B):
    return [[A[a][0] * B[0][b] + A[a][1] * B[1][b] + A[a][2] * B[2][b] for b in range(3)] for a in range(3)]


def _skew(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def _exp_axis(mp, k, h):
    """Exp(h e_k): Rodrigues with the unit axis e_k."""
    e = [mp.mpf(0)] * 3
    e[k] = mp.mpf(1)
    K = _skew(e)
    K2 = _mm(K, K)
    s, c = mp.sin(h), 1 - mp.cos(h)
    return [[(1 if a == b else 0) + s * K[a][b] + c * K2[a][b] for b in range(3)] for a in range(3)]


def _mpf_mat(mp, M):
    return [[mp.mpf(float(M[a, b])) for b in range(3)] for a in range(3)]


def _mpf_vec(mp, v):
    return [mp.mpf(float(x)) for x in v]


def _residual(mp, stage, R, v, R_LI, I, L):
    """The functor's residual for one sample (I / L: dicts of mpf members).  LI_init.h:103, :141-142, :182-189."""
    if stage == 1:
        Rw = _mv(R, L["ang_vel"])
        return [Rw[a] - I["ang_vel"][a] for a in range(3)]
    if stage == 2:
        Rw = _mv(R, L["ang_vel"])
        deltaT_LI = L["t"] - I["t"]  # LI_init.cpp:358: Lidar timeStamp - IMU timeStamp
        return [Rw[a] - I["ang_vel"][a] - (deltaT_LI + v[3]) * I["ang_acc"][a] + v[a] for a in range(3)]
    R_LL0 = L["rot_end"]
    if "Jacob_trans" not in L:  # the functor's known quantities: they depend on the sample and the fixed R_LI alone
        R_LI_T = [[R_LI[b][a] for b in range(3)] for a in range(3)]
        W, A = _skew(L["ang_vel"]), _skew(L["ang_acc"])
        WW = _mm(W, W)
        L["Jacob_trans"] = [[WW[a][b] + A[a][b] for b in range(3)] for a in range(3)]
        L["t1"] = _mv(R_LL0, _mv(R_LI_T, I["linear_acc"]))
    Jt, t1 = L["Jacob_trans"], L["t1"]
    t2 = _mv(R_LL0, v[0:3])
    t3 = _mv(R, [mp.mpf(0), mp.mpf(0), mp.mpf(-9.81)])  # STD_GRAV = V3D(0, 0, -G_m_s2) with the double 9.81 (LI_init.h:27)
    t5 = _mv(R_LL0, _mv(Jt, v[3:6]))
    return [t1[a] - t2[a] + t3[a] - L["linear_acc"][a] - t5[a] for a in range(3)]


def mp_sample_terms(stage, R, v, R_LI, imu, lid, step="1e-20"):
    """Per-sample residuals r (n x 3) and finite-difference Jacobians J (n x 3 x dof) as nested lists of mpf."""
    mp = _mp()
    dof = DOF[stage]
    h = mp.mpf(step)
    Rm = _mpf_mat(mp, R)
    vm = _mpf_vec(mp, v)
    RLIm = _mpf_mat(mp, R_LI) if R_LI is not None else None
    Rp = [_mm(_exp_axis(mp, k, h), Rm) for k in range(3)]
    Rn = [_mm(_exp_axis(mp, k, -h), Rm) for k in range(3)]
    rs, Js = [], []
    for i in range(len(imu)):
        I = dict(ang_vel=_mpf_vec(mp, imu.ang_vel[i]), ang_acc=_mpf_vec(mp, imu.ang_acc[i]),
                 linear_acc=_mpf_vec(mp, imu.linear_acc[i]), t=mp.mpf(float(imu.t[i])))
        L = dict(ang_vel=_mpf_vec(mp, lid.ang_vel[i]), ang_acc=_mpf_vec(mp, lid.ang_acc[i]),
                 linear_acc=_mpf_vec(mp, lid.linear_acc[i]), t=mp.mpf(float(lid.t[i])), rot_end=_mpf_mat(mp, lid.rot_end[i]))
        r = _residual(mp, stage, Rm, vm, RLIm, I, L)
        J = [[None] * dof for _ in range(3)]
        for k in range(dof):
            if k < 3:
                rp = _residual(mp, stage, Rp[k], vm, RLIm, I, L)
                rn = _residual(mp, stage, Rn[k], vm, RLIm, I, L)
            else:
                vp, vn = list(vm), list(vm)
                vp[k - 3] = vm[k - 3] + h
                vn[k - 3] = vm[k - 3] - h
                rp = _residual(mp, stage, Rm, vp, RLIm, I, L)
                rn = _residual(mp, stage, Rm, vn, RLIm, I, L)
            for a in range(3):
                J[a][k] = (rp[a] - rn[a]) / (2 * h)
        rs.append(r)
        Js.append(J)
    return rs, Js


def mp_terms(stage, R, v, R_LI, imu, lid):
    """The exact outputs (J^T J flattened row-major, J^T r, cost - the kernel's output order) and sum_i mag_i per entry, both
    as lists of mpf of length dof * dof + dof + 1."""
    mp = _mp()
    dof = DOF[stage]
    rs, Js = mp_sample_terms(stage, R, v, R_LI, imu, lid)
    nout = dof * dof + dof + 1
    exact, mag = [mp.mpf(0)] * nout, [mp.mpf(0)] * nout
    for r, J in zip(rs, Js):
        for k in range(dof):
            for l in range(dof):
                p = [J[a][k] * J[a][l] for a in range(3)]
                exact[k * dof + l] += mp.fsum(p)
                mag[k * dof + l] += mp.fsum(abs(x) for x in p)
            p = [J[a][k] * r[a] for a in range(3)]
            exact[dof * dof + k] += mp.fsum(p)
            mag[dof * dof + k] += mp.fsum(abs(x) for x in p)
        c = mp.fsum(x * x for x in r) / 2
        exact[nout - 1] += c
        mag[nout - 1] += c
    return exact, mag


def bound(stage, n, mag):
    """The derived bound per entry (module docstring), as mpf."""
    return [(math.ceil(n / 256) + 8 + C_ROUNDINGS[stage]) * U * m for m in mag]


def worst_ratio(stage, n, got_flat, exact, mag):
    """max over entries of |got - exact| / bound (entries whose bound is zero must be exact: ratio 0 or inf)."""
    mp = _mp()
    worst = 0.0
    for g, e, b in zip(got_flat, exact, bound(stage, n, mag)):
        err = abs(mp.mpf(float(g)) - e)
        if b == 0:
            ratio = 0.0 if err == 0 else float("inf")
        else:
            ratio = float(err / b)
        worst = max(worst, ratio)
    return worst


def flat(JtJ, Jtr, cost):
    return np.r_[np.asarray(JtJ).reshape(-1), np.asarray(Jtr).reshape(-1), cost]


def oracle_sample_terms(stage, R, v, R_LI, imu, lid):
    """(n, nout): the float64 numpy oracle's outputs of every single sample."""
    LI = _LI()
    return np.stack([flat(*LI.normal_equations(stage, R, v, imu.slice(slice(i, i + 1)), lid.slice(slice(i, i + 1)), R_LI))
                     for i in range(len(imu))])


def kernel_order_sum(terms):
    """float64 sum over axis 0 in k_calib_eval's order: lane l adds samples l, l + 256, ...; then the tree 128, 64, ..., 1."""
    acc = np.zeros((256,) + terms.shape[1:])
    for i in range(len(terms)):
        acc[i % 256] += terms[i]
    s = 128
    while s > 0:
        acc[:s] += acc[s:2 * s]
        s //= 2
    return acc[0]


_cache = {}


def reference(stage, n, k):
    """(imu, lid, (R, v, R_LI), exact, mag) of size n at parameter point k - computed once per process and left unchanged."""
    key = (stage, n, k)
    if key not in _cache:
        imu, lid = random_pair(n, seed=11)
        pt = param_points(stage)[k]
        exact, mag = mp_terms(stage, pt[0], pt[1], pt[2], imu, lid)
        _cache[key] = (imu, lid, pt, exact, mag)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ solver problem
def solver_problem(n=700, seed=21, noise=1e-3):
    """One synthetic calibration with known truth: LiDAR records from a smooth random angular-velocity history, IMU records
    derived through the three functors' models from chosen R_LI, b_g, t_d, T_IL, b_a and gravity, plus noise."""
    LI = _LI()
    rng = np.random.default_rng(seed)
    t = 50.0 + 0.02 * np.arange(n)

    def smooth(amp, k=4):
        f = rng.uniform(0.1, 0.9, (k, 3))
        ph = rng.uniform(0, 2 * np.pi, (k, 3))
        a = rng.normal(0, amp / np.sqrt(k), (k, 3))
        val = sum(a[j] * np.sin(2 * np.pi * f[j] * t[:, None] + ph[j]) for j in range(k))
        der = sum(a[j] * 2 * np.pi * f[j] * np.cos(2 * np.pi * f[j] * t[:, None] + ph[j]) for j in range(k))
        return val, der

    from harness import synth
    truth = dict(R_LI=synth.rot_zyx(np.deg2rad(10.0), np.deg2rad(-20.0), np.deg2rad(60.0)), b_g=np.array([0.012, -0.007, 0.004]),
                 t_d=0.006, T_IL=np.array([0.11, -0.07, 0.23]), b_aL=np.array([0.004, -0.006, 0.003]),
                 R_GL0=synth.rot_zyx(np.deg2rad(4.0), np.deg2rad(-7.0), np.deg2rad(15.0)))
    imu, lid = LI.CalibSeq(n), LI.CalibSeq(n)
    lid.t = t.copy()
    imu.t = t + rng.uniform(-0.004, 0.004, n)        # dT = L.t - I.t of both signs
    lid.ang_vel, lid.ang_acc = smooth(0.8)
    lid.linear_acc, _ = smooth(1.5)
    eul, _ = smooth(0.5)
    lid.rot_end = synth.rot_zyx_batch(eul[:, 0], eul[:, 1], eul[:, 2])
    R = truth["R_LI"]
    imu.ang_acc = lid.ang_acc @ R.T
    dT = lid.t - imu.t
    # stage 1/2 model: 0 = R w_L - w_I - (dT + t_d) alpha_I + b_g
    imu.ang_vel = lid.ang_vel @ R.T - (dT + truth["t_d"])[:, None] * imu.ang_acc + truth["b_g"] + rng.normal(0, noise, (n, 3))
    # stage 3 model: 0 = R_LL0 R_LI^T a_I - R_LL0 b_a + R_GL0 g - a_L - R_LL0 ([w]x^2 + [alpha]x) T_IL
    Rg = truth["R_GL0"] @ LI.STD_GRAV
    M = np.stack([LI.skew(w) @ LI.skew(w) + LI.skew(a) for w, a in zip(lid.ang_vel, lid.ang_acc)])
    inner = truth["b_aL"] + np.einsum("nji,nj->ni", lid.rot_end, lid.linear_acc - Rg) + M @ truth["T_IL"]
    imu.linear_acc = inner @ R.T + rng.normal(0, noise, (n, 3))
    truth["grav_L0"] = Rg
    truth["acc_bias"] = R @ truth["b_aL"]
    truth["T_LI"] = -R @ truth["T_IL"]
    return imu, lid, truth


def recovery_errors(truth, R_LI, gyro_bias, time_lag_2, T_LI, acc_bias, grav_L0):
    """Distance of a solution from the chosen truth, per quantity."""
    R_LI = np.asarray(R_LI).reshape(3, 3)
    ang = np.arccos(np.clip((np.trace(truth["R_LI"].T @ R_LI) - 1) / 2, -1, 1))
    return dict(rot_rad=float(ang), b_g=float(np.abs(np.asarray(gyro_bias) - truth["b_g"]).max()),
                t_d=float(abs(time_lag_2 - truth["t_d"])), T_LI=float(np.abs(np.asarray(T_LI) - truth["T_LI"]).max()),
                acc_bias=float(np.abs(np.asarray(acc_bias) - truth["acc_bias"]).max()),
                grav_L0=float(np.abs(np.asarray(grav_L0) - truth["grav_L0"]).max()))


_solved = {}


def oracle_solution():
    """The numpy oracle's stages 1 -> 2 -> 3 on solver_problem(), solved once per process."""
    if not _solved:
        LI = _LI()
        imu, lid, truth = solver_problem()
        s1 = LI.solve_stage1(imu, lid)
        s2 = LI.solve_stage2(imu, lid, s1["R_LI"])
        s3 = LI.solve_stage3(imu, lid, s2["R_LI"])
        _solved.update(imu=imu, lid=lid, truth=truth, s1=s1, s2=s2, s3=s3,
                       err=recovery_errors(truth, s2["R_LI"], s2["gyro_bias"], s2["time_lag_2"], s3["T_LI"], s3["acc_bias"], s3["grav_L0"]))
    return _solved


# ------------------------------------------------------------------------------------------------ filter / correlation inputs
ZERO_PHASE_CASES = ((1, 63), (5, 128), (6, 62), (11, 128), (16, 500))   # (n_seq, n): 12 / 60 / 72 / 132 / 192 lanes


def filter_batch(n_seq, n, seed=31):
    """(n_seq, n, 22): every sequence and channel a different smooth + noise signal with its own offset; random rot_end, stamps."""
    rng = np.random.default_rng([seed, n_seq, n])
    b = rng.normal(0, 1.0, (n_seq, n, 22))
    x = np.arange(n)[None, :, None]
    sq = np.arange(n_seq)[:, None, None]
    ch = np.arange(12)[None, None, :]
    b[:, :, 9:21] = np.sin(0.05 * (1 + ch + 12 * sq) * x / (1 + 0.1 * sq) + ch) + 0.1 * b[:, :, 9:21] + (ch - 5.0) + 3.0 * sq
    return b


def seq_from_records(rec):
    LI = _LI()
    s = LI.CalibSeq(len(rec))
    s.rot_end = rec[:, 0:9].reshape(-1, 3, 3).copy()
    s.ang_vel, s.linear_vel = rec[:, 9:12].copy(), rec[:, 12:15].copy()
    s.ang_acc, s.linear_acc = rec[:, 15:18].copy(), rec[:, 18:21].copy()
    s.t = rec[:, 21].copy()
    return s


def rolled_pair(n, shift, seed):
    """Seeded noise and a rolled copy of it plus a little noise (as tests/test_gpu_calib.py does at n = 900)."""
    LI = _LI()
    rng = np.random.default_rng([seed, n, shift + 5000])
    a, b = LI.CalibSeq(n), LI.CalibSeq(n)
    a.ang_vel = rng.normal(0, 0.5, (n, 3))
    b.ang_vel = np.roll(a.ang_vel, shift, axis=0) + rng.normal(0, 0.01, (n, 3))
    return a, b


ROLLED_CASES = ((1, 0), (2, 0), (2, 1), (3, 1), (3, -1), (128, 9), (128, -30), (129, -9), (129, 64), (257, 100), (257, -128),
                (1000, 301), (1000, -77))
# n = 300: 599 lags, the winner k = (n - 1) + lag placed on the argmax kernel's stride boundaries
BOUNDARY_N = 300
BOUNDARY_K = (255, 256, 257, 511, 512)


def windowed_pair(n, lag, seed=41):
    """b[i + lag] = a[i] without wrap-around (two windows of one longer noise series): corr peaks at `lag` alone."""
    LI = _LI()
    rng = np.random.default_rng([seed, n, lag + 5000])
    m = abs(lag)
    base = rng.normal(0, 0.5, (n + 2 * m, 3))
    a, b = LI.CalibSeq(n), LI.CalibSeq(n)
    a.ang_vel = base[m:m + n].copy()
    b.ang_vel = base[m - lag:m - lag + n].copy()
    return a, b


def plateau_pair(n=300, seed=43, peak=False):
    """LiDAR |omega| = |(3, 4, 0)| = 5 exactly: the running mean stays 5 and every correlation is zero.
    peak = True: the first two LiDAR samples become |omega| = 9 and 1.  One changed sample would make the mean 5 + 4 / 300, which
    is inexact, and nothing would tie; with 9, 1, 5, 5, ... the running mean goes 9 -> 5 -> 5 exactly, the centred series is
    (4, -4, 0, 0, ...), corr(lag) = 4 a'[-lag] - 4 a'[1 - lag] for lag <= 0 and exactly 0 for every lag >= 2: 298 tied lags
    (k = 301 .. 598) under a unique positive peak, and lanes of the argmax kernel that meet in its tree holding equal values."""
    LI = _LI()
    rng = np.random.default_rng(seed)
    a, b = LI.CalibSeq(n), LI.CalibSeq(n)
    a.ang_vel = rng.normal(0, 0.5, (n, 3))
    b.ang_vel = np.tile([3.0, 4.0, 0.0], (n, 1))
    if peak:
        b.ang_vel[0] = [9.0, 0.0, 0.0]
        b.ang_vel[1] = [1.0, 0.0, 0.0]
    return a, b


def xcorr_values_host_order(imu, lidar):
    """The 2n - 1 correlations of LI_Init::xcorr_temporal_init with the products summed in ascending i (LI_init.cpp:160-193), the
    order the library keeps; index k <-> lag = k - (n - 1)."""
    a = np.linalg.norm(imu.ang_vel, axis=1)
    b = np.linalg.norm(lidar.ang_vel, axis=1)
    n = len(a)
    ma = mb = 0.0
    for i in range(n):
        ma += (a[i] - ma) / (i + 1)
        mb += (b[i] - mb) / (i + 1)
    corr = np.zeros(2 * n - 1)
    for k in range(2 * n - 1):
        lag = k - (n - 1)
        i0, i1 = max(0, -lag), min(n, n - lag)
        c = 0.0
        for x in (a[i0:i1] - ma) * (b[i0 + lag:i1 + lag] - mb):
            c += x
        corr[k] = c
    return corr


def xcorr_host_order(imu, lidar):
    """(lag_IMU_wtr_Lidar, k of the winner) of those correlations under the reference's strict `>`: the first maximum."""
    corr = xcorr_values_host_order(imu, lidar)
    k = int(np.argmax(corr))  # numpy's argmax returns the first of equal maxima
    return -(k - (len(corr) // 2)), k


# ------------------------------------------------------------------------------------------------ whole-initialisation inputs
def synthetic_accumulation(n_states, seed=51, rate=20.0):
    """Aligned IMU / LiDAR records as lii_li_init_interpolate leaves them, from harness/synth: LiDAR states on the true
    trajectory (attitude, body rate, velocity, with the noise an odometry would have) and a simulated 200 Hz IMU with a known
    extrinsic, biases and clock offset.  Returns (imu22, lidar22) of about n_states records."""
    import ctypes as C

    import lidar_imu_init_amd as lii
    from harness import synth
    from lidar_imu_init_amd import calib_state_array
    rng = np.random.default_rng(seed)
    traj = synth.Trajectory()
    dt = 1.0 / rate
    ts = dt * np.arange(1, n_states + 1)
    lid = calib_state_array(n_states)
    lid[:, 0:9] = traj.R(ts).reshape(-1, 9)
    lid[:, 9:12] = traj.omega_body(ts - dt / 2) + rng.normal(0, 0.01, (n_states, 3))
    lid[:, 12:15] = traj.vel(ts) + rng.normal(0, 0.01, (n_states, 3))
    lid[:, 21] = ts
    R_LI = synth.rot_zyx(np.deg2rad(-1.0), np.deg2rad(-0.3), np.deg2rad(88.0))
    t_imu, gyro, accel = synth.simulate_imu(traj, -0.5, ts[-1] + 0.5, 200.0, R_LI, np.array([-0.02, 0.02, 0.17]),
                                            np.array([0.002, 0.0007, -0.0004]), np.array([0.006, -0.007, 0.008]), 0.015, seed=seed)
    imu_all = calib_state_array(len(t_imu))
    imu_all[:, 9:12], imu_all[:, 18:21], imu_all[:, 21] = gyro, accel, t_imu
    oi, ol = calib_state_array(n_states), calib_state_array(n_states)
    cnt = C.c_int32(0)
    rc = lii.load_library().lii_li_init_interpolate(imu_all.ctypes.data_as(C.c_void_p), len(imu_all), lid.ctypes.data_as(C.c_void_p),
                                                    n_states, 2.5, oi.ctypes.data_as(C.c_void_p), ol.ctypes.data_as(C.c_void_p),
                                                    C.byref(cnt))
    assert rc == 0
    return oi[:cnt.value].copy(), ol[:cnt.value].copy()


def short_accumulation(shift, n=200, seed=61):
    """200 aligned states at 50 Hz whose |omega| holds one bump, `shift` samples later on the LiDAR than on the IMU: the
    cross-correlation finds that lag and the time compensation that follows leaves 169 - shift states for the second
    zero-phase filter (the oracle's count: 61 at shift = 108, 58 at shift = 112)."""
    LI = _LI()
    rng = np.random.default_rng(seed)
    t = 10.0 + 0.02 * np.arange(n)
    imu, lid = LI.CalibSeq(n), LI.CalibSeq(n)
    imu.t, lid.t = t.copy(), t + 0.001
    x = np.arange(n)
    for s, c in ((imu, 60), (lid, 60 + shift)):
        s.ang_vel = 0.05 * rng.normal(0, 1, (n, 3)) + np.outer(np.exp(-0.5 * ((x - c) / 6.0) ** 2), [0.8, -0.5, 0.6])
        s.linear_vel = 0.1 * rng.normal(0, 1, (n, 3))
        s.linear_acc = 0.1 * rng.normal(0, 1, (n, 3)) + [0, 0, 9.8]
    return imu, lid

"""lii_pose_refine / lii_pose_refine_dev on the device: the iterated update on the six pose states at K candidate poses in one call,
against its numpy restatement on the oracle's pass (pose_refine_cases.refine6_np, pinned to the oracle's 24-state update by
tests/test_pose_refine_host.py) and against the serial chain of lii_iekf_update calls it replaces; and the rules of the call - pose k's
bits do not depend on its batch, its call or its form; bad and empty members do not disturb their neighbours; the handle's registration
state is left alone; argument and state errors write nothing; relocalize(batched=True) finds what relocalize() finds.

Hall map of small_world, the `tiny` scan (2 048 points) through scan_upload + downsample_skip.  Where the kernels change path: a workgroup
holds 64 consecutive points of one pose (65 points: one full workgroup and one of a single pair; 2 000: the last holds 16), the solve sums
four poses per workgroup (K = 1, 2, 63, 65), and a launch of up to 2 048 workgroups searches with four wavefronts per workgroup, a larger
one with one (32 workgroups per pose at 2 048 points: K = 64 is the last of the first kind, K = 65 the first of the second).

Bounds: the project's own update tolerance (tests/test_gpu_register.py) - 1e-6 m, 1e-7 rad - and 1e-6 max|cov| for the covariance.
"""
import ctypes as C

import numpy as np
import pytest

import pose_refine_cases as prc
import pose_score_cases as psc

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -5  # LII_ERR_INVALID, LII_ERR_STATE


def _code(f):
    import lidar_imu_init_amd as lii
    try:
        f()
        return 0
    except lii.LIIError as e:
        return e.code


@pytest.fixture(scope="module")
def world(oracle, small_world):
    import lidar_imu_init_amd as lii
    _, map_pts = small_world
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    tree = oracle.Tree("oracle")
    tree.build(map_pts)
    yield dict(reg=reg, tree=tree, scan=psc.tiny_scan(small_world), poses=prc.all_poses(small_world), refs={})
    reg.close()


def _load(reg, scan):
    reg.scan_upload(scan)
    assert reg.downsample_skip() == len(scan)


def _ref(world, oracle, k, n, max_it, updates, prior=None):
    """refine6_np of parity pose k on the first n points: computed once, shared, never changed."""
    key = (k, n, max_it, updates, prior is not None)
    if key not in world["refs"]:
        r_li, t_li, R, p = world["poses"][k]
        info = {}
        st, its, eff = prc.refine6_np(oracle, world["tree"], world["scan"][:n], psc.state_at(oracle, R, p, r_li, t_li), max_it, updates, prior=prior, info=info)
        world["refs"][key] = (st, its, eff, info)
    return world["refs"][key]


def _hold(oracle, tag, rec, ref):
    """One record against refine6_np: the figures are printed before anything is asserted."""
    st, its, eff, info = ref
    dp, dth = prc.pose_errors(oracle, st, rec["pose"])
    cov = oracle.StateView(st).cov[:6, :6]
    dc = float(np.abs(rec["cov"] - cov).max())
    print(f"{tag}: iterations {int(rec['iterations'])} (ref {its}) searches {int(rec['searches'])} effect {int(rec['effect_num'])} (ref {eff}) "
          f"|dp| {dp:.2e} |dtheta| {dth:.2e} |dcov| {dc:.2e} of {np.abs(cov).max():.2e} total_residual {float(rec['total_residual']):.6f} "
          f"(ref {info['total_residual']:.6f}) flags {int(rec['flags'])}")
    assert int(rec["iterations"]) == sum(its)
    assert int(rec["effect_num"]) == eff
    assert dp <= prc.TOL_P and dth <= prc.TOL_R
    assert dc <= prc.TOL_COV * np.abs(cov).max()
    assert int(rec["searches"]) == info["searches"]
    assert int(rec["flags"]) == (prc.CONVERGED if info["converged"] else 0)
    # every residual follows the pose: a point at most 30 m out moves by TOL_P + 30 TOL_R, and its world coordinates round to floats
    # (2e-6 at 30 m, three of them)
    assert abs(float(rec["total_residual"]) - info["total_residual"]) <= max(eff, 1) * (prc.TOL_P + 30 * prc.TOL_R + 6e-6)


def _batches(world):
    """The 24 poses by base state: [(first index, r_li, t_li, R (K, 3, 3), p (K, 3))]."""
    poses = world["poses"]
    return [(0, poses[0][0], poses[0][1], np.stack([q[2] for q in poses[:23]]), np.stack([q[3] for q in poses[:23]])),
            (23, poses[23][0], poses[23][1], poses[23][2][None], poses[23][3][None])]


@pytest.mark.parametrize("max_it,updates", prc.SCHEDULES)
def test_oracle_parity(world, oracle, max_it, updates):
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"]
    assert len(scan) == 2048
    _load(reg, scan)
    seen = 0
    for first, r_li, t_li, R, p in _batches(world):
        base = lii.State(psc.state_at(oracle, R[0], p[0], r_li, t_li))
        rec = reg.pose_refine(base, (R, p), max_iterations=max_it, updates=updates)
        assert rec.dtype == lii.api.POSE_REFINED_DTYPE and len(rec) == len(R)
        for k in range(len(R)):
            _hold(oracle, f"pose {first + k} ({max_it}, {updates}) n 2048", rec[k], _ref(world, oracle, first + k, 2048, max_it, updates))
            seen += 1
    assert seen == 24
    # the 65-point prefix: one full workgroup of 64 pairs and one of a single pair
    _load(reg, scan[:65])
    _, r_li, t_li, R, p = _batches(world)[0]
    sub = [0, 1, 4, 8]
    rec = reg.pose_refine(lii.State(psc.state_at(oracle, R[0], p[0])), (R[sub], p[sub]), max_iterations=max_it, updates=updates)
    for j, k in enumerate(sub):
        _hold(oracle, f"pose {k} ({max_it}, {updates}) n 65", rec[j], _ref(world, oracle, k, 65, max_it, updates))


@pytest.mark.parametrize("max_it,updates", prc.SCHEDULES)
def test_explicit_prior(world, oracle, max_it, updates):
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"]
    _load(reg, scan)
    prior = prc.dense_prior()
    assert np.all(np.linalg.eigvalsh(prior) > 0) and np.abs(prior - np.diag(np.diag(prior))).max() > 1e-5
    _, _, _, R, p = _batches(world)[0]
    sub = [0, 1, 8]
    base = lii.State(psc.state_at(oracle, R[0], p[0]))
    rec = reg.pose_refine(base, (R[sub], p[sub]), max_iterations=max_it, updates=updates, prior_cov=prior)
    for j, k in enumerate(sub):
        _hold(oracle, f"pose {k} ({max_it}, {updates}) dense prior", rec[j], _ref(world, oracle, k, 2048, max_it, updates, prior=prior))
    # ... and the prior in base's pose block with prior_cov left out is the same call
    base.cov[:6, :6] = prior
    again = reg.pose_refine(base, (R[sub], p[sub]), max_iterations=max_it, updates=updates)
    assert np.array_equal(again.view(np.uint8), rec.view(np.uint8))


@pytest.mark.parametrize("max_it,updates", prc.SCHEDULES)
def test_agreement_with_the_serial_chain(world, oracle, small_world, max_it, updates):
    """`updates` consecutive lii_iekf_update(imu_en = 0) calls on a second handle, pose by pose - what Registrar.relocalize runs."""
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"]
    _load(reg, scan)
    serial = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    serial.map_build(small_world[1])
    _load(serial, scan)
    for first, r_li, t_li, R, p in _batches(world):
        base = lii.State(psc.state_at(oracle, R[0], p[0], r_li, t_li))
        rec = reg.pose_refine(base, (R, p), max_iterations=max_it, updates=updates)
        for k in range(len(R)):
            st = lii.State(psc.state_at(oracle, R[k], p[k], r_li, t_li))
            its, eff = 0, 0
            for _ in range(updates):
                rep = serial.iekf_update(st, st.copy(), max_iterations=max_it, imu_en=False)
                its, eff = its + rep["iterations"], rep["effect_num"]
            dp, dth = prc.pose_errors(oracle, st.pod, rec[k]["pose"])
            dc = float(np.abs(rec[k]["cov"] - st.cov[:6, :6]).max())
            print(f"pose {first + k} ({max_it}, {updates}) against the serial chain: iterations {int(rec[k]['iterations'])} / {its} effect "
                  f"{int(rec[k]['effect_num'])} / {eff} |dp| {dp:.2e} |dtheta| {dth:.2e} |dcov| {dc:.2e}")
            assert int(rec[k]["iterations"]) == its and int(rec[k]["effect_num"]) == eff
            assert dp <= prc.TOL_P and dth <= prc.TOL_R and dc <= prc.TOL_COV * np.abs(st.cov[:6, :6]).max()
    serial.close()


def _grid_pool():
    """405 distinct poses cut from a grid around the perturbed pose: +-1 m at 0.25 m, yaw -20 .. 20 degrees at 10."""
    import lidar_imu_init_amd as lii
    Rp, pp = psc.perturbed(False)
    R, p = lii.pose_grid(Rp, pp, 1.0, 0.25, -np.deg2rad(20.0), np.deg2rad(25.0), np.deg2rad(10.0))
    assert len(R) == 405
    return lii.api.poses_array((R, p))


def _dev_array(reg, addr, shape, dtype):
    """device memory -> numpy, through the runtime the library itself uses"""
    hip = C.CDLL(reg.L._name)
    out = np.zeros(shape, dtype)
    reg.synchronize()
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(int(addr)), C.c_size_t(out.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("n_down", [2048, 2000])
def test_determinism(world, oracle, n_down):
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"][:n_down]
    _load(reg, scan)
    base = lii.State(psc.state_at(oracle, psc.TRUE_R, psc.TRUE_P))
    pool = _grid_pool()[:257]
    alone = np.concatenate([reg.pose_refine(base, pool[k:k + 1]) for k in range(257)])
    assert (alone["effect_num"] > 0).all() and (alone["flags"] & prc.BAD_POSE == 0).all()
    assert len({r.tobytes() for r in alone}) == 257  # (distinct poses, distinct records: a mix-up would show)
    d_P, d_out = reg.dev_alloc(pool.nbytes), reg.dev_alloc(257 * 408)
    for K in (1, 2, 63, 64, 65, 257):
        P = pool[:K]
        first = reg.pose_refine(base, P)
        assert np.array_equal(first.view(np.uint8), alone[:K].view(np.uint8)), (K, "a member of a batch against the pose alone")
        back = np.ascontiguousarray(reg.pose_refine(base, P[::-1])[::-1])
        assert np.array_equal(back.view(np.uint8), first.view(np.uint8)), (K, "the reversed batch")
        assert np.array_equal(reg.pose_refine(base, P).view(np.uint8), first.view(np.uint8)), (K, "a second call")
        reg.dev_upload(d_P, P)
        reg.dev_upload(d_out, np.zeros(K, prc.RECORD_DTYPE))
        reg.pose_refine_dev(base, d_P, K, d_out)
        assert np.array_equal(_dev_array(reg, d_out, (K,), prc.RECORD_DTYPE).view(np.uint8), first.view(np.uint8)), (K, "the device form")


def test_degenerate_members(world, oracle):
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"][:2000]
    _load(reg, scan)
    base = lii.State(psc.state_at(oracle, psc.TRUE_R, psc.TRUE_P))
    P = _grid_pool()[100:107].copy()
    good = {k: reg.pose_refine(base, P[k:k + 1])[0].tobytes() for k in (0, 2, 4, 6)}
    P[1, 5] = np.nan                                 # a NaN entry of the rotation
    P[3] = np.r_[np.eye(3).reshape(-1), 500.0, 0.0, 0.0]  # every point outside the map
    P[5, 9] = np.inf                                 # an Inf position
    for max_it, updates in prc.SCHEDULES:
        rec = reg.pose_refine(base, P, max_iterations=max_it, updates=updates)
        for k in (1, 5):
            assert int(rec[k]["flags"]) == prc.BAD_POSE
            assert rec[k]["pose"].tobytes() == P[k].tobytes() and np.array_equal(rec[k]["cov"], base.cov[:6, :6])
            assert (int(rec[k]["effect_num"]), int(rec[k]["iterations"]), int(rec[k]["searches"]), float(rec[k]["total_residual"])) == (0, 0, 0, 0.0)
        assert rec[3]["pose"].tobytes() == P[3].tobytes() and rec[3]["cov"].tobytes() == np.ascontiguousarray(base.cov[:6, :6]).tobytes()
        assert (int(rec[3]["effect_num"]), int(rec[3]["iterations"]), int(rec[3]["searches"])) == (0, 2 * updates, 2 * updates)
        assert int(rec[3]["flags"]) == prc.CONVERGED and float(rec[3]["total_residual"]) == 0.0
        if (max_it, updates) == (4, 2):
            for k, want in good.items():
                assert rec[k].tobytes() == want, k
        else:
            assert all(int(rec[k]["effect_num"]) > 0 for k in good)


def test_round_trip(world, oracle):
    """The covariance of a record is a prior the call takes again: exactly symmetric, as base's pose block and as prior_cov; and
    relocalize(batched=True) runs on its own result - a coarse grid, then a fine one around the winner."""
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"]
    _load(reg, scan)
    _, _, _, R, p = _batches(world)[0]
    sub = [1, 2, 4, 8]
    base = lii.State(psc.state_at(oracle, R[0], p[0]))
    first = reg.pose_refine(base, (R[sub], p[sub]))
    for r in first:
        assert np.array_equal(r["cov"].view(np.uint64), np.ascontiguousarray(r["cov"].T).view(np.uint64)), "a record's cov is exactly symmetric"
        assert np.all(np.linalg.eigvalsh(r["cov"]) > 0)
    # base carries the pose and the cov of an earlier record; the prior is left out
    carried = base.copy()
    carried.rot_end[:] = first[2]["pose"][:9].reshape(3, 3)
    carried.pos_end[:] = first[2]["pose"][9:]
    carried.cov[:6, :6] = first[2]["cov"]
    again = reg.pose_refine(carried, first["pose"], max_iterations=4, updates=2)
    # ... and the same cov as prior_cov: the same call
    as_arg = reg.pose_refine(base, first["pose"], max_iterations=4, updates=2, prior_cov=first[2]["cov"])
    assert np.array_equal(again.view(np.uint8), as_arg.view(np.uint8))
    for j in range(len(sub)):
        st0 = psc.state_at(oracle, first[j]["pose"][:9].reshape(3, 3), first[j]["pose"][9:])
        info = {}
        st, its, eff = prc.refine6_np(oracle, world["tree"], scan, st0, 4, 2, prior=first[2]["cov"], info=info)
        _hold(oracle, f"record {j} refined again from record 2's cov", again[j], (st, its, eff, info))
        assert np.array_equal(again[j]["cov"].view(np.uint64), np.ascontiguousarray(again[j]["cov"].T).view(np.uint64))
    # relocalize(batched=True) on its own result: each stage is held to the serial path from the same base and grid - the same winning
    # node, the same pose and covariance block within the bounds above (what the refinement reaches is the update's business, not this call's)
    Rp, pp = psc.perturbed(False)
    base1 = lii.State(psc.state_at(oracle, Rp, pp))
    grid1 = lii.pose_grid(Rp, pp, 1.0, 0.5, -np.deg2rad(10.0), np.deg2rad(15.0), np.deg2rad(10.0))
    stage = 0
    for base_s, grid in ((base1, grid1), (None, None)):
        if base_s is None:  # the fine grid around the batched winner, from the state the batched path returned
            base_s = best_b
            grid = lii.pose_grid(best_b.rot_end, best_b.pos_end, 0.2, 0.1, -np.deg2rad(2.0), np.deg2rad(3.0), np.deg2rad(2.0))
        best_b, info_b = reg.relocalize(base_s, grid, top=3, max_iterations=4, updates=2, batched=True)
        best_s, info_s = reg.relocalize(base_s, grid, top=3, max_iterations=4, updates=2)
        dp, dth = prc.pose_errors(oracle, best_s.pod, best_b.pod[:12])
        dc = float(np.abs(best_b.cov[:6, :6] - best_s.cov[:6, :6]).max())
        err = float(np.linalg.norm(best_b.pos_end - psc.TRUE_P))
        print(f"stage {stage}: batched best {info_b['best']} tried {info_b['tried']}; serial best {info_s['best']} tried {info_s['tried']}; |dp| {dp:.2e} "
              f"|dtheta| {dth:.2e} |dcov| {dc:.2e} of {np.abs(best_s.cov[:6, :6]).max():.2e}; {err * 1e3:.2f} mm from the truth")
        assert info_b["best"] == info_s["best"] and info_b["tried"] == info_s["tried"]
        assert dp <= prc.TOL_P and dth <= prc.TOL_R and dc <= prc.TOL_COV * np.abs(best_s.cov[:6, :6]).max()
        assert np.array_equal(best_b.cov[:6, :6], best_b.cov[:6, :6].T) and np.all(np.linalg.eigvalsh(best_b.cov[:6, :6]) > 0)
        stage += 1


def test_observer(world, oracle):
    """A registration, then the call, then everything a caller can see of the registration state - against the same sequence without
    the call.  The point-noise weights can be read under model 1 alone, where the call is refused: they are held across the refusal."""
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"]
    n = len(scan)
    Rw, pw = psc.perturbed(False)
    st0 = psc.state_at(oracle, Rw, pw)
    P = _grid_pool()[:64]

    def run(refine, noise):
        _load(reg, scan)
        if noise:
            reg.set_point_noise()
        try:
            st = lii.State(st0)
            reg.iekf_update(st, st.copy(), max_iterations=4, imu_en=False)
            unfinished = reg.last_unfinished_queries()
            weights = reg.point_noise_download() if noise else np.zeros(0, np.float32)
            if refine:
                rc = _code(lambda: reg.pose_refine(lii.State(st0), P))
                assert rc == (STATE if noise else 0)
                assert reg.last_unfinished_queries() == unfinished
                if noise:
                    assert np.array_equal(reg.point_noise_download().view(np.uint32), weights.view(np.uint32))
            nb, cnt, sel = reg.neighbors(n)
            sums = reg.iekf_iterate(st, False, False)  # the cached planes and the sticky selection
            rep = reg.iekf_update(st, st.copy(), max_iterations=4, imu_en=False)
        finally:
            if noise:
                reg.clear_point_noise()
        return nb, cnt, sel, unfinished, sums, st.pod.copy(), (rep["iterations"], rep["effect_num"]), weights

    for noise in (False, True):
        plain, called = run(False, noise), run(True, noise)
        assert np.array_equal(plain[0].view(np.uint32), called[0].view(np.uint32)) and np.array_equal(plain[1], called[1])
        assert np.array_equal(plain[2], called[2]) and plain[3] == called[3]
        assert np.array_equal(plain[4].view(np.uint64), called[4].view(np.uint64)), "all 91 sums of the pass on cached planes"
        assert np.array_equal(plain[5].view(np.uint64), called[5].view(np.uint64)) and plain[6] == called[6]
        assert np.array_equal(plain[7].view(np.uint32), called[7].view(np.uint32))
        assert int(plain[4][90]) > 0.9 * n


def test_argument_and_state_errors(world, oracle, small_world):
    import lidar_imu_init_amd as lii
    reg, scan = world["reg"], world["scan"][:2000]
    _load(reg, scan)
    base = lii.State(psc.state_at(oracle, psc.TRUE_R, psc.TRUE_P))
    K = 5
    P = _grid_pool()[:K].copy()
    L, h = reg.L, reg.h
    out = np.zeros(K, prc.RECORD_DTYPE)
    out.view(np.uint8)[:] = 0xA5
    out0 = out.copy()
    d_P, d_out = reg.dev_alloc(2100 * 96), reg.dev_alloc(2100 * 408)
    reg.dev_upload(d_P, P)
    reg.dev_upload(d_out, out0)

    def both(handle=reg, base_p=base, prior=None, poses=True, k=K, max_it=4, updates=2, dst=True):
        b = base_p.pod.ctypes.data if base_p is not None else None
        pr = np.ascontiguousarray(prior, np.float64).ctypes.data if prior is not None else None
        rc_h = handle.L.lii_pose_refine(handle.h, b, pr, P.ctypes.data if poses else None, k, max_it, updates, out.ctypes.data if dst else None)
        rc_d = handle.L.lii_pose_refine_dev(handle.h, b, pr, d_P if poses else None, k, max_it, updates, d_out if dst else None)
        return rc_h, rc_d

    def untouched():
        return np.array_equal(out.view(np.uint8), out0.view(np.uint8)) and np.array_equal(_dev_array(reg, d_out, (K,), prc.RECORD_DTYPE).view(np.uint8), out0.view(np.uint8))

    # LII_ERR_INVALID: NULL arguments, n_poses, max_iterations outside 1 .. 16, updates outside 1 .. 8
    assert both(base_p=None) == (INVALID, INVALID) and both(poses=False) == (INVALID, INVALID) and both(dst=False) == (INVALID, INVALID)
    assert both(k=0) == (INVALID, INVALID) and both(k=-3) == (INVALID, INVALID)
    assert both(max_it=0) == (INVALID, INVALID) and both(max_it=17) == (INVALID, INVALID)
    assert both(updates=0) == (INVALID, INVALID) and both(updates=9) == (INVALID, INVALID)
    # ... a prior that is not finite, not symmetric, not positive definite - as an argument, and as base's pose block
    bad_priors = []
    for edit in (lambda M: M.__setitem__((2, 2), np.nan), lambda M: M.__setitem__((0, 4), np.inf), lambda M: M.__setitem__((1, 3), M[1, 3] + 1e-9),
                 lambda M: M.__setitem__((5, 5), 0.0), lambda M: M.__setitem__((4, 4), -1e-4)):
        M = prc.dense_prior()
        edit(M)
        bad_priors.append(M)
    singular = np.ones((6, 6))  # symmetric, finite, rank 1
    for M in bad_priors + [singular, np.zeros((6, 6))]:
        assert both(prior=M) == (INVALID, INVALID)
        b2 = base.copy()
        b2.cov[:6, :6] = M
        assert both(base_p=b2) == (INVALID, INVALID)
    # ... n_poses * n_down above 2^22 pairs (2 000 points: 2 097 poses fit, 2 098 do not), refused before any pointer is used
    assert 2097 * 2000 <= 2 ** 22 < 2098 * 2000
    assert both(k=2098) == (INVALID, INVALID) and both(k=65_537) == (INVALID, INVALID)
    assert untouched()
    # the limits themselves are served: 16 iterations, 8 updates, and 2 097 poses (one round)
    assert both(max_it=16, updates=8) == (0, 0)
    assert (out["iterations"] >= 16).all() and (out["iterations"] <= 128).all()
    assert np.array_equal(_dev_array(reg, d_out, (K,), prc.RECORD_DTYPE).view(np.uint8), out.view(np.uint8))
    many = np.tile(P, (420, 1))[:2097]
    got = np.zeros(2097, prc.RECORD_DTYPE)
    assert L.lii_pose_refine(h, base.pod.ctypes.data, None, many.ctypes.data, 2097, 1, 1, got.ctypes.data) == 0
    assert all(got[j].tobytes() == got[j % K].tobytes() for j in range(0, 2097, 97)) and (got["iterations"] == 1).all()
    out[:] = out0
    reg.dev_upload(d_out, out0)
    # LII_ERR_STATE: the per-point noise model on
    reg.set_point_noise()
    try:
        assert both() == (STATE, STATE)
    finally:
        reg.clear_point_noise()
    # LII_ERR_STATE: no down-sampled cloud; no map
    r2 = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    assert both(handle=r2) == (STATE, STATE)  # neither
    r2.map_build(small_world[1])
    assert both(handle=r2) == (STATE, STATE)  # a map, no cloud
    r2.close()
    r3 = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    _load(r3, scan)
    assert both(handle=r3) == (STATE, STATE)  # a cloud, no map
    # LII_ERR_STATE: from inside lii_scan_job::while_waiting
    r3.map_build(small_world[1])
    seen = []
    st = lii.State(psc.state_at(oracle, *psc.perturbed(False)))
    r3.scan_upload(scan)
    r3.scan_register(st, st.copy(), leaf=0.0, max_iterations=2, while_waiting=lambda: seen.append(both(handle=r3)))
    assert seen == [(STATE, STATE)]
    assert untouched()
    assert _code(lambda: r3.pose_refine(base, P)) == 0  # ... and behind the call it is served again
    r3.close()


def test_relocalize_batched(oracle, small_world):
    """The case of tests/test_gpu_relocalize.py cut to the 512 grid nodes nearest the truth: batched=True goes through one pose_refine
    call and ends at the node and the pose the serial path ends at."""
    import lidar_imu_init_amd as lii
    hall, map_pts = small_world
    scan = psc.tiny_scan(small_world)
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    _load(reg, scan)
    guess = lii.State(psc.state_at(oracle, psc.GUESS_R, psc.GUESS_P))
    R, p = lii.pose_grid(psc.GUESS_R, psc.GUESS_P, 4.0, 0.5, 0.0, 2 * np.pi, np.deg2rad(10.0))
    inside = np.all((p[:, :2] > hall.lo[:2] + 0.3) & (p[:, :2] < hall.hi[:2] - 0.3), axis=1)
    R, p = R[inside], p[inside]
    near = np.argsort(np.linalg.norm(p - psc.TRUE_P, axis=1), kind="stable")[:512]
    R, p = R[near], p[near]
    serial, info_s = reg.relocalize(guess, (R, p), top=3, max_iterations=4, updates=2)
    before = reg.neighbors(len(scan))
    batched, info_b = reg.relocalize(guess, (R, p), top=3, max_iterations=4, updates=2, batched=True)
    after = reg.neighbors(len(scan))
    assert all(np.array_equal(a, b) for a, b in zip(before, after))  # the batched path leaves the registration state alone
    dp, dth = prc.pose_errors(oracle, serial.pod, batched.pod[:12])
    err = float(np.linalg.norm(batched.pos_end - psc.TRUE_P))
    print(f"serial tried {info_s['tried']} best {info_s['best']}; batched tried {info_b['tried']} best {info_b['best']}; "
          f"|dp| {dp:.2e} |dtheta| {dth:.2e}; {err * 1e3:.2f} mm from the truth")
    assert info_b["best"] == info_s["best"] and np.array_equal(info_b["order"], info_s["order"])
    assert [k for k, _ in info_b["tried"]] == [k for k, _ in info_s["tried"]]
    assert dp <= prc.TOL_P and dth <= prc.TOL_R
    assert np.abs(batched.cov[:6, :6] - serial.cov[:6, :6]).max() <= prc.TOL_COV * np.abs(serial.cov[:6, :6]).max()
    assert np.array_equal(batched.pod[12:36], guess.pod[12:36]) and np.array_equal(batched.cov[6:, 6:], guess.cov[6:, 6:])
    assert err < 0.01
    reg.close()

"""The 24-state solve (k_reduce_solve / k_iekf_solve, lii_iekf.hip) must give THE SAME BITS as the library that recorded
tests/golden/solve_bits/cases.npz (tools/record_solve_bits.py; recorded with the commit before the elimination took its pivot
column by DPP row broadcast and boxplus was spread over lanes).  Both changes re-schedule the arithmetic and keep every
expression as it was, so nothing is tolerated: np.array_equal on the final lii_state (all 612 doubles), normal_eq, iterations,
searches, effect_num and last_solve_info of every case.  The solver does not depend on the cloud's size: the small map and the
`tiny` / `vlp16` scans of test_gpu_register.py.
Cases: LIO and LO with max_iterations 1, 2, 4, 5 (a stop by the iteration bound and by the second re-match, each with the
covariance); the LIO-regime prior; the vanishing-pivot prior (the fallback with row exchanges must be reported); a rotation
update below the 1e-5 branch of Exp; lii_scan_register with the launch plan on (three calls: the later ones run a learnt plan)."""
import os

import numpy as np
import pytest

from conftest import make_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_bits", "cases.npz")
FIELDS = ("state", "normal_eq", "iterations", "searches", "effect_num", "last_solve_info")


def _scan(small_world, sensor, seed):
    from harness import synth
    hall, _ = small_world
    R = synth.rot_zyx(0.03, -0.02, 0.4)
    p = np.array([0.8, -0.6, 0.1])
    return synth.make_scan(hall, sensor, R, p, noise=0.02, seed=seed), R, p


def _record(reg, s, rep):
    return dict(state=s.pod.copy(), normal_eq=np.array(rep["normal_eq"], np.float64), iterations=np.int64(rep["iterations"]),
                searches=np.int64(rep["searches"]), effect_num=np.int64(rep["effect_num"]), last_solve_info=np.int64(reg.last_solve_info()))


def _update(reg, scan, cur, prop, max_it, imu_en):
    reg.scan_upload(scan)
    reg.downsample_skip()
    s = cur.copy()
    rep = reg.iekf_update(s, prop, max_iterations=max_it, imu_en=imu_en)
    return _record(reg, s, rep)


def run_cases(oracle, small_world):
    """Every case's result with the library that is loaded: {name: {field: array}} (the recorder and the test share it)."""
    import lidar_imu_init_amd as lii
    from harness import synth
    hall, map_pts = small_world
    out = {}
    reg = lii.Registrar(max_scan_points=150_000, max_map_points=400_000, filter_size_map=0.15)
    try:
        reg.map_build(map_pts)
        # LIO / LO, stopped by the iteration bound (1, 2) or by the second re-match (4, 5)
        for imu_en, sensor in ((True, "vlp16"), (False, "tiny")):
            scan, R, p = _scan(small_world, sensor, seed=11)
            R_LI = synth.rot_zyx(0.01, 0.02, -0.015) if imu_en else np.eye(3)
            T_LI = np.array([0.03, -0.02, 0.05]) if imu_en else np.zeros(3)
            Rw = R @ R_LI.T
            st_true = make_state(oracle, Rw, p - Rw @ T_LI, R_LI, T_LI)
            st0 = lii.State(oracle.state_boxplus(st_true, np.r_[0.006, -0.004, 0.008, 0.04, -0.03, 0.02, np.zeros(18)]))
            for max_it in (1, 2, 4, 5):
                out[f"{'lio' if imu_en else 'lo'}_it{max_it}"] = _update(reg, scan, st0, st0, max_it, imu_en)
        # the covariance of a running LIO filter (test_update_with_lio_regime_covariance)
        scan, R, p = _scan(small_world, "vlp16", seed=21)
        st_true = make_state(oracle, R, p)
        rng = np.random.default_rng(5)
        scale = np.sqrt(np.r_[np.full(6, 1e-8), np.full(6, 1e-4), np.full(3, 1.0), np.full(3, 1e-3), np.full(3, 1e-2), np.full(3, 1e-5)])
        A = rng.normal(0, 1, (24, 24))
        Cm = A @ A.T / 24 + np.eye(24)
        Cm = Cm / np.sqrt(np.outer(np.diag(Cm), np.diag(Cm)))
        P = Cm * np.outer(scale, scale)
        for imu_en in (True, False):
            prop = lii.State(oracle.state_boxplus(st_true, np.r_[2e-4, -1e-4, 2e-4, 2e-3, -1e-3, 1e-3, np.zeros(18)]))
            prop.cov[:] = P
            cur = lii.State(oracle.state_boxplus(prop.pod, np.r_[rng.normal(0, 1e-4, 6), rng.normal(0, 1e-3, 6), rng.normal(0, 1e-2, 12)]))
            out[f"lio_regime_{'lio' if imu_en else 'lo'}"] = _update(reg, scan, cur, prop, 5, imu_en)
        # the first pivot 1 + (P11 G)_00 vanishes (test_elimination_with_row_exchanges_when_the_pivot_vanishes)
        scan, R, p = _scan(small_world, "vlp16", seed=11)
        st_true = make_state(oracle, R, p)
        st0 = oracle.state_boxplus(st_true, np.r_[0.002, -0.001, 0.002, 0.01, -0.01, 0.005, np.zeros(18)])
        reg.scan_upload(scan)
        reg.downsample_skip()
        ne = reg.iekf_iterate(lii.State(st0), True, True)
        G = np.zeros((12, 12))
        G[np.triu_indices(12)] = ne[:78]
        G = G + np.triu(G, 1).T
        u = G[:, 0]
        j = 1 + int(np.argmax(np.abs(u[1:])))
        v = np.zeros(12)
        v[0], v[j] = 1.0, -2.0 * u[0] / u[j]
        eps, delta = 1e-10, 1e-7
        s_ = (1.0 - delta + eps * u[0]) / u[0]
        prop = lii.State(st0)
        prop.cov[:] = 0
        prop.cov[:12, :12] = eps * np.eye(12) + s_ * np.outer(v, v)
        prop.cov[12:, 12:] = 1e-4 * np.eye(12)
        out["vanishing_pivot"] = _update(reg, scan, prop, prop, 4, True)
        # a rotation block of the prior so small that both rotation updates stay below Exp's 1e-5 branch: R (+) dtheta = R I
        scan, R, p = _scan(small_world, "tiny", seed=3)
        prop = lii.State(oracle.state_boxplus(make_state(oracle, R, p), np.r_[1e-6, -2e-6, 1e-6, 0.02, -0.01, 0.01, np.zeros(18)]))
        prop.cov[:] = 0
        prop.cov[np.arange(24), np.arange(24)] = np.r_[np.full(3, 1e-16), np.full(3, 1.0), np.full(3, 1e-16), np.full(15, 1e-5)]
        out["small_rotation"] = _update(reg, scan, prop, prop, 4, True)
        out["small_rotation"]["start_rot"] = prop.pod[:21].copy()
        # lii_scan_register, the launch plan on (the default): the second and third call run with the plan the first one taught
        scan, R, p = _scan(small_world, "tiny", seed=5)
        st0 = lii.State(oracle.state_boxplus(make_state(oracle, R, p), np.r_[0.004, -0.003, 0.005, 0.03, -0.02, 0.01, np.zeros(18)]))
        for k in range(3):
            reg.scan_upload(scan)
            s = st0.copy()
            rep = reg.scan_register(s, st0, leaf=0.1, max_iterations=5, imu_en=False)
            out[f"scan_register_{k}"] = _record(reg, s, rep)
    finally:
        reg.close()
    return out


@pytest.fixture(scope="module")
def got(oracle, small_world):
    return run_cases(oracle, small_world)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_every_recorded_case_is_run(got, golden):
    assert sorted({k.rsplit("/", 1)[0] for k in golden}) == sorted(got)
    assert len(got) == 8 + 2 + 1 + 1 + 3


def test_same_bits_as_the_recorded_library(got, golden):
    for name, case in sorted(got.items()):
        for f in FIELDS:
            want = golden[f"{name}/{f}"]
            print(name, f, "equal" if np.array_equal(case[f], want) else f"max |diff| {np.max(np.abs(np.asarray(case[f], np.float64) - want)):.3e}")
    for name, case in sorted(got.items()):
        for f in FIELDS:
            assert np.array_equal(case[f], golden[f"{name}/{f}"]), (name, f)


def test_the_cases_take_the_paths_they_are_named_for(got):
    assert got["vanishing_pivot"]["last_solve_info"] >= 1           # the routine with row exchanges ran and was reported
    assert got["lio_it5"]["last_solve_info"] == 0 and got["lo_it4"]["last_solve_info"] == 0
    for k in (1, 2):                                                  # stopped by the iteration bound ...
        assert got[f"lio_it{k}"]["iterations"] == k and got[f"lo_it{k}"]["iterations"] == k
    assert got["lio_it5"]["searches"] >= 2                            # ... and with a re-match behind the first search
    sr = got["small_rotation"]                                        # Exp returned the identity: both rotations kept their bits
    assert np.array_equal(sr["state"][0:9], sr["start_rot"][0:9]) and np.array_equal(sr["state"][12:21], sr["start_rot"][12:21])
    assert not np.array_equal(sr["state"][9:12], sr["start_rot"][9:12])

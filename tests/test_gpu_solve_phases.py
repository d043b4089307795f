"""The phases of the 24-state solve AROUND its elimination (k_reduce_solve / iekf_solve_body, lii_iekf.hip: the hand-off of the 91
sums, A = I + P11 G, the state update, the covariance tail) must give THE SAME BITS as the library that recorded
tests/golden/solve_phases/cases.npz (tools/record_solve_phases.py; recorded with the commit before the state phase was re-arranged:
the rotations alone on the first wavefront, the schedule, the vector blocks, the solution and the control words on the three others,
the schedule's verdict through LDS and a barrier at the end of every pass, the search log fetched with the control block).
Nothing is tolerated: np.array_equal on the final lii_state (all 612 doubles: state and covariance), normal_eq, iterations, searches,
effect_num, converged and last_solve_info of every case.
Cases, where the touched phases can go wrong:
  * clouds of 1, 63, 64, 65, 257 and 1 025 down-sampled points (one partial column of partial sums; fewer, exactly and more than 64
    columns; several chunks), each in LIO mode and in LO mode (imu_en false: columns 6 - 11 of the Jacobian are zero), full schedule
    with a re-match;
  * a registration that stops at pass 0 (max_iterations = 1: the covariance on the first pass), LIO and LO;
  * the vanishing first pivot (the elimination with row exchanges runs and lii_last_solve_info reports it);
  * a rotation update below Exp's identity threshold (|dtheta| < 1e-5) - the other cases are above it;
  * every case again through the three-launch form (k_reduce91 / all-reduce over one rank / k_iekf_solve): the fused launch's bits;
    and k_reduce91 alone (lii_iekf_iterate) gives the sums the fused launch reports for pass 0;
  * a sum that never arrives still ends in LII_ERR_COMM within its time bound."""
import os
import time

import numpy as np
import pytest

from conftest import make_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_phases", "cases.npz")
FIELDS = ("state", "normal_eq", "iterations", "searches", "effect_num", "converged", "last_solve_info")
SIZES = (1, 63, 64, 65, 257, 1025)


def _record(reg, s, rep):
    return dict(state=s.pod.copy(), normal_eq=np.array(rep["normal_eq"], np.float64), iterations=np.int64(rep["iterations"]),
                searches=np.int64(rep["searches"]), effect_num=np.int64(rep["effect_num"]), converged=np.int64(rep["converged"]),
                last_solve_info=np.int64(reg.last_solve_info()))


def _inputs(oracle, small_world):
    """[(name, cloud, state, propagated state, max_iterations, imu_en)] - built once, the same for every form of the update."""
    import lidar_imu_init_amd as lii
    from harness import synth
    hall, _ = small_world
    R = synth.rot_zyx(0.03, -0.02, 0.4)
    p = np.array([0.8, -0.6, 0.1])

    def scan_of(sensor, seed):
        return synth.make_scan(hall, sensor, R, p, noise=0.02, seed=seed)

    cases = []
    full = scan_of("vlp16", 11)
    full = full[np.random.default_rng(17).permutation(len(full))]  # any prefix is spread over the whole field of view
    assert len(full) >= max(SIZES)
    for imu_en in (True, False):
        R_LI = synth.rot_zyx(0.01, 0.02, -0.015) if imu_en else np.eye(3)
        T_LI = np.array([0.03, -0.02, 0.05]) if imu_en else np.zeros(3)
        Rw = R @ R_LI.T
        st_true = make_state(oracle, Rw, p - Rw @ T_LI, R_LI, T_LI)
        st0 = lii.State(oracle.state_boxplus(st_true, np.r_[0.006, -0.004, 0.008, 0.04, -0.03, 0.02, np.zeros(18)]))
        mode = "lio" if imu_en else "lo"
        for n in SIZES:
            cases.append((f"{mode}_n{n}", full[:n], st0, st0, 5, imu_en))
        cases.append((f"{mode}_pass0", full[:1025], st0, st0, 1, imu_en))
    return cases, scan_of, R, p


def _special_inputs(oracle, reg, scan_of, R, p):
    """The vanishing pivot (its prior is built from the sums of a pass: needs a registrar) and the rotation below Exp's threshold."""
    import lidar_imu_init_amd as lii
    cases = []
    scan = scan_of("vlp16", 11)
    st0 = oracle.state_boxplus(make_state(oracle, R, p), np.r_[0.002, -0.001, 0.002, 0.01, -0.01, 0.005, np.zeros(18)])
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
    prop.cov[:12, :12] = eps * np.eye(12) + s_ * np.outer(v, v)  # the first pivot 1 + (P11 G)_00 vanishes
    prop.cov[12:, 12:] = 1e-4 * np.eye(12)
    cases.append(("vanishing_pivot", scan, prop, prop, 4, True))
    prop = lii.State(oracle.state_boxplus(make_state(oracle, R, p), np.r_[1e-6, -2e-6, 1e-6, 0.02, -0.01, 0.01, np.zeros(18)]))
    prop.cov[:] = 0
    prop.cov[np.arange(24), np.arange(24)] = np.r_[np.full(3, 1e-16), np.full(3, 1.0), np.full(3, 1e-16), np.full(15, 1e-5)]
    cases.append(("small_rotation", scan_of("tiny", 3), prop, prop, 4, True))
    return cases


def _update(reg, scan, cur, prop, max_it, imu_en):
    reg.scan_upload(scan)
    reg.downsample_skip()
    s = cur.copy()
    rep = reg.iekf_update(s, prop, max_iterations=max_it, imu_en=imu_en)
    out = _record(reg, s, rep)
    out["start"] = cur.pod.copy()
    return out


def run_cases(oracle, small_world):
    """Every case's result with the library that is loaded, {form: {name: {field: array}}} (the recorder and the test share it):
    "fused" - k_reduce_solve; "three" - k_reduce91, the all-reduce of a one-rank communicator, k_iekf_solve; "sums91" - k_reduce91
    alone at the start state of the pass-0 cases."""
    import lidar_imu_init_amd as lii
    _, map_pts = small_world
    out = {"fused": {}, "three": {}, "sums91": {}}
    cases, scan_of, R, p = _inputs(oracle, small_world)
    for form in ("fused", "three"):
        reg = lii.Registrar(max_scan_points=150_000, max_map_points=400_000, filter_size_map=0.15)
        try:
            reg.map_build(map_pts)
            if form == "fused":
                cases = cases + _special_inputs(oracle, reg, scan_of, R, p)
                for name, scan, cur, prop, max_it, imu_en in cases:
                    if name.endswith("_pass0"):
                        reg.scan_upload(scan)
                        reg.downsample_skip()
                        out["sums91"][name] = np.asarray(reg.iekf_iterate(cur.copy(), True, imu_en)).copy()
            else:
                reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
                reg.comm_set_partition("caller")
                assert reg.comm_transport() == "rccl"
            for name, scan, cur, prop, max_it, imu_en in cases:
                out[form][name] = _update(reg, scan, cur, prop, max_it, imu_en)
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


NAMES = [f"{m}_{c}" for m in ("lio", "lo") for c in [f"n{n}" for n in SIZES] + ["pass0"]] + ["vanishing_pivot", "small_rotation"]


def test_every_recorded_case_is_run(got, golden):
    assert sorted({k.rsplit("/", 1)[0] for k in golden}) == sorted(NAMES)
    assert sorted(got["fused"]) == sorted(NAMES) and sorted(got["three"]) == sorted(NAMES)
    assert len(NAMES) == 2 * (len(SIZES) + 1) + 2


@pytest.mark.parametrize("form", ["fused", "three"])
@pytest.mark.parametrize("name", NAMES)
def test_same_bits_as_the_recorded_library(got, golden, form, name):
    case = got[form][name]
    for f in FIELDS:
        want = golden[f"{name}/{f}"]
        print(form, name, f, "equal" if np.array_equal(case[f], want) else f"max |diff| {np.max(np.abs(np.asarray(case[f], np.float64) - want)):.3e}")
    for f in FIELDS:
        assert np.array_equal(case[f], golden[f"{name}/{f}"]), (form, name, f)


@pytest.mark.parametrize("mode", ["lio", "lo"])
def test_the_sums_of_the_host_driven_pass_are_the_fused_launch_s(got, mode):
    # (max_iterations = 1: the report carries the sums of pass 0, formed at the start state by the summing workgroups of k_reduce_solve)
    assert np.array_equal(got["sums91"][f"{mode}_pass0"], got["fused"][f"{mode}_pass0"]["normal_eq"])


def test_the_cases_take_the_paths_they_are_named_for(got):
    g = got["fused"]
    for mode in ("lio", "lo"):
        assert g[f"{mode}_pass0"]["iterations"] == 1 and g[f"{mode}_pass0"]["searches"] == 1  # the covariance on the first pass
        assert not np.array_equal(g[f"{mode}_pass0"]["state"][36:], g[f"{mode}_pass0"]["start"][36:])
        assert g[f"{mode}_n1025"]["iterations"] >= 3 and g[f"{mode}_n1025"]["searches"] >= 2         # the full schedule, with a re-match
        assert g[f"{mode}_n1025"]["last_solve_info"] == 0
        for n in SIZES:
            assert (0 if n == 1 else 1) <= g[f"{mode}_n{n}"]["effect_num"] <= n  # (a lone point may fail the plane gate)
        # a rotation update above Exp's identity threshold: the rotation moved
        assert not np.array_equal(g[f"{mode}_n1025"]["state"][0:9], g[f"{mode}_n1025"]["start"][0:9])
    # LO mode: columns 6 - 11 of the Jacobian are zero, their sums with them
    ne = g["lo_pass0"]["normal_eq"]
    Gm = np.zeros((12, 12))
    Gm[np.triu_indices(12)] = ne[:78]
    assert not Gm[:, 6:].any() and not ne[84:90].any() and Gm[:6, :6].any()
    assert g["vanishing_pivot"]["last_solve_info"] >= 1               # the routine with row exchanges ran and was reported
    assert got["three"]["vanishing_pivot"]["last_solve_info"] >= 1
    sr = g["small_rotation"]                                          # Exp returned the identity: both rotations kept their bits
    assert np.array_equal(sr["state"][0:9], sr["start"][0:9]) and np.array_equal(sr["state"][12:21], sr["start"][12:21])
    assert not np.array_equal(sr["state"][9:12], sr["start"][9:12])


def test_a_dropped_sum_ends_in_an_error_within_its_bound(oracle, small_world):
    """LII_TEST=sum_lost: summing workgroup 5 keeps its sum to itself and the bound is 0.2 s - whichever wavefronts poll the tagged
    words, the solver gives up by the clock and the update ends with LII_ERR_COMM, not in a hang."""
    import lidar_imu_init_amd as lii
    _, map_pts = small_world
    cases, _, _, _ = _inputs(oracle, small_world)
    _, scan, cur, prop, max_it, imu_en = [c for c in cases if c[0] == "lio_n257"][0]
    old = os.environ.get("LII_TEST")
    os.environ["LII_TEST"] = "sum_lost"
    try:
        reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    finally:
        os.environ.pop("LII_TEST", None)
        if old is not None:
            os.environ["LII_TEST"] = old
    try:
        reg.map_build(map_pts)
        reg.scan_upload(scan)
        reg.downsample_skip()
        s = cur.copy()
        t0 = time.perf_counter()
        with pytest.raises(lii.LIIError) as e:
            reg.iekf_update(s, prop, max_iterations=max_it, imu_en=imu_en)
        dt = time.perf_counter() - t0
        print(f"LII_ERR_COMM after {dt:.3f} s")
        assert e.value.code == -6  # LII_ERR_COMM (include/liinit_hip.h)
        assert 0.15 < dt < 5.0, dt  # the bound, not a hang and not an instant failure
    finally:
        reg.close()

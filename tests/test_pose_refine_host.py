"""refine6_np (tests/pose_refine_cases.py) - the six-state restatement the device tests are held to - against the oracle's 24-state
Tree.iekf_update from the default state, on the 24 parity poses and both schedules (no GPU).

From the default covariance (the pose block uncorrelated with the rest) the six-state update IS the 24-state update in LO mode: the
iteration counts of every update and the last pass's effect_num are equal, the other 18 states do not move, and the pose differs by the
rounding between a 24 x 24 and a 6 x 6 inversion alone - measured 6.2e-10 m / 1.2e-10 rad at most, held to 1e-8 / 1e-8 (16 x headroom).
A pose far outside the map selects nothing: two iterations per update, pose and covariance unchanged.
"""
import numpy as np
import pytest

import pose_refine_cases as prc
import pose_score_cases as psc


@pytest.fixture(scope="module")
def world(oracle, small_world):
    _, map_pts = small_world
    tree = oracle.Tree("oracle")
    tree.build(map_pts)
    return dict(tree=tree, scan=psc.tiny_scan(small_world))


def _chain24(O, tree, scan, st0, max_it, updates):
    st, its, eff = st0.copy(), [], 0
    for _ in range(updates):
        r = tree.iekf_update(scan, st, st, max_iterations=max_it, imu_en=False, threads=4)
        st = r["state"]
        its.append(int(r["iters"]))
        eff = int(r["selected"].astype(bool).sum())
    return st, its, eff


@pytest.mark.parametrize("max_it,updates", prc.SCHEDULES)
def test_six_states_are_the_24_state_update(world, oracle, small_world, max_it, updates):
    O, tree, scan = oracle, world["tree"], world["scan"]
    worst_p = worst_r = worst_c = 0.0
    for k, (r_li, t_li, R, p) in enumerate(prc.all_poses(small_world)):
        st0 = psc.state_at(O, R, p, r_li, t_li)
        st6, its6, eff6 = prc.refine6_np(O, tree, scan, st0, max_it, updates)
        st24, its24, eff24 = _chain24(O, tree, scan, st0, max_it, updates)
        dp, dth = prc.pose_errors(O, st24, st6[:12])
        dc = float(np.abs(O.StateView(st6).cov[:6, :6] - O.StateView(st24).cov[:6, :6]).max())
        print(f"pose {k} ({max_it}, {updates}): iterations {its6} effect {eff6}  |dp| {dp:.2e} |dtheta| {dth:.2e} |dcov| {dc:.2e}")
        assert its6 == its24 and eff6 == eff24
        assert dp < 1e-8 and dth < 1e-8
        assert np.array_equal(st24[12:36], st0[12:36]), "the 24-state update in LO mode leaves the other 18 states alone"
        worst_p, worst_r, worst_c = max(worst_p, dp), max(worst_r, dth), max(worst_c, dc)
    print(f"worst: {worst_p:.2e} m, {worst_r:.2e} rad, cov {worst_c:.2e}")
    assert worst_c < 1e-12


def test_a_pose_outside_the_map_stays_where_it_is(world, oracle):
    O, tree, scan = oracle, world["tree"], world["scan"]
    st0 = psc.state_at(O, np.eye(3), np.array([500.0, 0.0, 0.0]))
    for max_it, updates in prc.SCHEDULES:
        info = {}
        st, its, eff = prc.refine6_np(O, tree, scan, st0, max_it, updates, info=info)
        assert its == [2] * updates and eff == 0 and info["searches"] == 2 * updates and info["converged"]
        assert np.array_equal(st, st0)

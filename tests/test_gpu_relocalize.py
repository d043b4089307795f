"""Re-localisation in a saved map: the update alone cannot leave a far-off guess, a scored grid of poses around the guess can.

The case: the hall map, the `tiny` scan (true pose rot_zyx(0.03, -0.02, 0.4), (0.8, -0.6, 0.1)), a guess 3.3 m / -2.2 m / 0.73 rad off
with roll / pitch 0.  The CPU oracle from the guess ends 3.9 m from the truth after eight updates; from the best node of the grid
(1 828 selected points against the guess's 571) one update ends 2 mm / 2.6e-4 rad from it.
"""
import numpy as np
import pytest

import pose_score_cases as psc

pytestmark = pytest.mark.gpu


def test_relocalize_from_a_far_off_guess(oracle, small_world):
    import lidar_imu_init_amd as lii
    hall, map_pts = small_world
    scan = psc.tiny_scan(small_world)
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    reg.scan_upload(scan)
    assert reg.downsample_skip() == len(scan)
    guess = lii.State(psc.state_at(oracle, psc.GUESS_R, psc.GUESS_P))

    def errors(st):
        return float(np.linalg.norm(st.pos_end - psc.TRUE_P)), float(np.linalg.norm(oracle.log_so3(psc.TRUE_R.T @ st.rot_end)))

    # the need: eight updates from the guess stay far from the truth
    st = guess.copy()
    for _ in range(8):
        reg.iekf_update(st, st.copy(), max_iterations=4, imu_en=False)
    dp, dth = errors(st)
    print(f"eight updates from the guess: {dp:.3f} m, {dth:.4f} rad from the truth")
    assert dp > 1.0

    # the grid: +-4 m at 0.5 m, every yaw at 10 degrees, roll / pitch / z of the guess; nodes within 0.3 m of the walls dropped
    R, p = lii.pose_grid(psc.GUESS_R, psc.GUESS_P, 4.0, 0.5, 0.0, 2 * np.pi, np.deg2rad(10.0))
    inside = np.all((p[:, :2] > hall.lo[:2] + 0.3) & (p[:, :2] < hall.hi[:2] - 0.3), axis=1)
    R, p = R[inside], p[inside]
    assert 5000 < len(R) <= 17 * 17 * 36
    best, info = reg.relocalize(guess, (R, p), top=3, max_iterations=4, updates=2)
    dp, dth = errors(best)
    order = info["order"]
    g_eff = reg.pose_score(guess, (psc.GUESS_R[None], psc.GUESS_P[None]))[1][0]
    print(f"{len(R)} nodes; best three effect_num {info['effect_num'][order[:3]]}, the guess {g_eff}; tried {info['tried']}; "
          f"relocalize ends {dp * 1e3:.2f} mm, {dth:.2e} rad from the truth")
    assert dp < 0.01 and dth < 0.002
    assert info["effect_num"][order[0]] >= 2 * g_eff
    assert np.all(np.diff(info["effect_num"][order]) <= 0)  # the ranking is by effect_num first
    reg.close()

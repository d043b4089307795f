"""The per-point noise model on the CPU (tests/point_noise_np.py): the basis-free closed form the library computes against calcBodyVar as
the reference writes it (src/laserMapping.cpp:158-181, :1039-1042) wherever that is finite - and the reason the closed form exists: at
z = 0 in the IMU frame the literal form is not finite, the closed form is.

The bound on the relative difference of sigma^2, 2^-22: the one float of the literal path that matters is `range` (:160) - a double rounded
to float, one or two roundings of 2^-24 - and it enters squared (A = range direction_hat N, var takes A A^T); everything else is double on
both sides.  Run with -s for the worst figure (profiles/point_noise.md records it)."""
import numpy as np

import plane_rows_np as pr
import point_noise_np as pn

BOUND = 2.0 ** -22


def _random_rotation(rng):
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_closed_form_against_the_literal_form():
    rng = np.random.default_rng(4201)
    worst, n = 0.0, 0
    while n < 20_000:
        d = pr._unit(rng.normal(0, 1, 3))
        if abs(d[2]) < 0.05:
            continue
        p = d * np.exp(rng.uniform(np.log(0.5), np.log(100.0)))
        R = _random_rotation(rng)
        normal = pr._unit(rng.normal(0, 1, 3)).astype(np.float32)
        lit, closed = pn.sigma2_literal(p, R, normal), pn.sigma2_closed(p, R, normal)
        assert np.isfinite(lit) and np.isfinite(closed) and closed >= 1.0 / pr.RINV
        worst = max(worst, abs(lit - closed) / closed)
        n += 1
    print(f"\nclosed form against calcBodyVar as written, {n} cases: worst relative difference of sigma^2 {worst:.3e} (bound 2^-22 = {BOUND:.3e})")
    assert worst <= BOUND


def test_z_zero_is_why_the_closed_form_exists():
    R = pr.POSES["lo"].R
    normal = pr._unit([0.3, -0.5, 0.8]).astype(np.float32)
    for p in ([3.0, 4.0, 0.0], [1.0, -1.0, 0.0], [0.5, 0.0, 0.0], [-60.0, 7.0, 0.0]):
        var = pn.calc_body_var_literal(p)
        assert not np.all(np.isfinite(var)), p
        assert not np.isfinite(pn.sigma2_literal(p, R, normal)), p
        closed = pn.sigma2_closed(p, R, normal)
        assert np.isfinite(closed) and closed > 1.0 / pr.RINV, p
        # ... while just off the ring, on either side, the two agree
        for dz in (0.06, -0.06):
            q = [p[0], p[1], dz * float(np.hypot(p[0], p[1]))]
            near, closed_q = pn.sigma2_literal(q, R, normal), pn.sigma2_closed(q, R, normal)
            assert abs(near - closed_q) / closed_q <= BOUND, (p, dz)


def test_the_point_at_the_origin_has_the_constant():
    for normal in ([0.0, 0.0, 1.0], [0.6, 0.0, 0.8]):
        assert pn.sigma2_closed(np.zeros(3), np.eye(3), np.array(normal, np.float32)) == 1.0 / pr.RINV
    # zero increments: the constant for every point
    assert pn.sigma2_closed([3.0, 4.0, 5.0], np.eye(3), np.array([0, 0, 1], np.float32), range_inc=0.0, degree_inc=0.0) == 1.0 / pr.RINV


def test_the_issue_s_illustrations():
    """0.02 m and 0.05 deg: about 714 head-on at 10 m, 929 grazing at 10 m, 115 grazing at 100 m."""
    n = np.array([1.0, 0.0, 0.0], np.float32)
    w = lambda p: 1.0 / pn.sigma2_closed(p, np.eye(3), n)
    assert abs(w([10.0, 0.0, 0.0]) - 714.3) < 0.5
    assert abs(w([0.0, 10.0, 0.0]) - 929.2) < 0.5
    assert abs(w([0.0, 100.0, 0.0]) - 116.1) < 1.5


def test_family_k_queries_lie_on_the_ring():
    """The added clusters: their queries have z_I = 0 - exactly where offset_R_L_I is the identity - the literal form is not finite there,
    and the numpy reference selects them (a row to compare)."""
    cs = pn.noise_cases()
    assert len(cs.nh) == len(pr.cases().nh) + 9 and np.array_equal(cs.map[:len(pr.cases().map)], pr.cases().map)
    for name, pose in pr.POSES.items():
        ks = [q for q in cs.queries if cs.nh[q["nh"]]["family"] == "K" and q["pose"] == name]
        assert len(ks) == 6
        for q in ks:
            p_i = pn.p_imu_of(pose, q["body"])
            if name == "lio":
                assert abs(p_i[2]) < 1e-5
                continue
            assert p_i[2] == 0.0
            r = pr.point_row(pose, False, q["body"], cluster=cs.nh[q["nh"]]["pts"])
            assert r["selected"], (name, q["kind"])
            normal = r["plane"]["pabcd"][:3].astype(np.float32)
            assert not np.isfinite(pn.sigma2_literal(p_i, pose.R, normal))
            assert 0.0 < pn.weight_of(pose, r) < pr.RINV

"""lii_sym3_eigen - the symmetric 3 x 3 eigen-solver the surface kernel runs on the device, here through its host form (no GPU) -
against np.linalg.eigh: eigenvalues within SOLVER_C u eig[2] (map_surface_cases.py; the constant is 4 x the worst figure this file
measures, and the file asserts the measured figure stays below it), the basis orthonormal to 1e-14, ||M v - lambda v|| within the same
bound, ascending order always."""
import numpy as np
import pytest

import lidar_imu_init_amd as lii
from map_surface_cases import SOLVER_C, U


def _m6(M):
    return [M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]]


def _rot(rng):
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return Q


def _with_spectrum(rng, lam):
    Q = _rot(rng)
    M = (Q * np.asarray(lam, np.float64)) @ Q.T
    return 0.5 * (M + M.T)


def _shapes():
    rng = np.random.default_rng(5)
    a = np.array([0.3, -0.5, 0.8])
    b = np.array([0.7, 0.1, -0.2])
    base = {
        "zero": np.zeros((3, 3)),
        "diagonal": np.diag([3.0, 1.0, 2.0]),
        "diagonal, descending": np.diag([5.0, 4.0, 0.5]),
        "double eigenvalue": _with_spectrum(rng, [1.0, 1.0, 4.0]),
        "double eigenvalue, upper": _with_spectrum(rng, [0.25, 2.0, 2.0]),
        "triple eigenvalue": np.eye(3) * 0.7,
        "triple eigenvalue, rotated": _with_spectrum(rng, [0.7, 0.7, 0.7]),
        "rank 1": np.outer(a, a),
        "rank 2": np.outer(a, a) + np.outer(b, b),
        "near-planar 1e-10": _with_spectrum(rng, [1e-10, 0.6, 1.0]),
        "near-planar 1e-10, axis-aligned": np.diag([1.0, 1e-10, 0.6]),
    }
    out = []
    for name, M in base.items():
        for s in (1.0, 1e-12, 1e6):
            out.append((f"{name} x {s:g}", M * s))
    return out


def _check(M, who):
    """Returns |eig - eigh| / (u eig[2]) (0 for the zero matrix) after asserting everything else."""
    eig, vec = lii.sym3_eigen(_m6(M))
    w = np.linalg.eigh(M)[0]
    top = max(abs(w[0]), abs(w[2]))
    bound = SOLVER_C * U * top
    assert np.all(np.diff(eig) >= 0), f"{who}: not ascending: {eig}"
    assert np.abs(vec @ vec.T - np.eye(3)).max() <= 1e-14, f"{who}: the basis is not orthonormal"
    err = np.abs(eig - w).max()
    res = max(np.linalg.norm(M @ vec[k] - eig[k] * vec[k]) for k in range(3))
    assert err <= bound, f"{who}: eigenvalues off by {err:.3g}, bound {bound:.3g}"
    assert res <= bound, f"{who}: residual {res:.3g}, bound {bound:.3g}"
    return (max(err, res) / (U * top)) if top > 0 else 0.0


@pytest.mark.parametrize("name,M", _shapes(), ids=[n for n, _ in _shapes()])
def test_shapes(name, M):
    c = _check(M, name)
    print(f"{name}: {c:.3g} u eig[2]")
    if not M.any():
        eig, vec = lii.sym3_eigen(_m6(M))
        assert not eig.any() and np.array_equal(vec, np.eye(3))
    if name.startswith("diagonal x") or "axis-aligned" in name:
        eig, _ = lii.sym3_eigen(_m6(M))
        assert np.array_equal(eig, np.sort(np.diag(M)))  # no rotation is made: the diagonal itself, bit for bit


def test_ten_thousand_random_covariances():
    """Covariances of 3 - 400 points drawn from anisotropic Gaussians in a random frame, by the formula of the surface kernel."""
    rng = np.random.default_rng(17)
    worst = 0.0
    for _ in range(10_000):
        n = int(rng.integers(3, 401))
        P = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 0, 3)) @ _rot(rng)
        mr = P.sum(axis=0) / n
        M = (P.T @ P) / n - np.outer(mr, mr)
        M = 0.5 * (M + M.T)
        worst = max(worst, _check(M, f"covariance of {n} points"))
    print(f"worst over 10 000 covariances: {worst:.3g} u eig[2]; SOLVER_C = {SOLVER_C}")
    assert 4.0 * worst <= SOLVER_C, "SOLVER_C no longer carries its margin of 4 over the measured worst case"


def test_the_small_eigenvalue_of_a_near_planar_matrix_survives():
    """What the closed form loses: eig0 / eig2 = 1e-10 comes back with a relative error far below 1."""
    rng = np.random.default_rng(23)
    for _ in range(200):
        M = _with_spectrum(rng, [1e-10, rng.uniform(0.2, 0.9), 1.0])
        eig, vec = lii.sym3_eigen(_m6(M))
        w = np.linalg.eigh(M)[0]
        assert abs(eig[0] - w[0]) <= SOLVER_C * U * w[2]
        assert abs(eig[0] - 1e-10) <= 1e-4 * 1e-10  # (SOLVER_C u / 1e-10 = 6e-5)

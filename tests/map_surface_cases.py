"""What the surface-statistics tests share (test_map_surface_ref.py and test_sym3_eigen.py on the CPU, test_gpu_map_surface.py on the
device): the numpy reference of lii_map_surface / lii_map_crispness, the selection hash, and the tolerances.

THE REFERENCE.  From map_radius_cases.Balls - the float32 brute-force ball, calc_dist's evaluation order, `float d2 <= double max_dist`
inclusive - the relative moments in float64, the covariance by the formula of include/liinit_hip.h

    d = (double)m - (double)q,  s1 = sum d,  s2_ab = sum d_a d_b,  mean_rel = s1 / n,  C_ab = s2_ab / n - mean_rel_a * mean_rel_b

(numpy has no FMA: every operation rounds once, as the library's does) and np.linalg.eigh.  Never the library.

THE TOLERANCES are derived here, not chosen.  u = 2^-53.
  count        exact.
  entries of C each moment sum has n terms of magnitude <= max_dist (1 + 4e-7) (a point is in the ball by its float32 d2, which carries a
               relative error < 4e-7).  Two summation orders of such a sum differ by at most n^2 u max_dist; after the division by n that is
               n u max_dist in s2 / n, twice n u max_dist in the product of the means (each mean moves by n u sqrt(max_dist), and is at
               most sqrt(max_dist)), and the three roundings of the formula itself stay below one more: |dC_ab| <= 4 n u max_dist.
  eigenvalues  Weyl: |d lambda| <= ||dC||_2 <= 3 max|dC_ab| for a 3 x 3 matrix, plus what the two solvers themselves add:
               SOLVER_C u eig[2].  SOLVER_C is MEASURED by tests/test_sym3_eigen.py (the largest |lii_sym3_eigen - eigh| / (u eig[2]) over
               its cases was 14 when the constant was set - 10 000 random covariances of 3 - 400 points and the degenerate
               shapes) and stands here with a margin of 4: 56.  That test asserts the measured figure stays below it.
  normal       Davis-Kahan: sin(angle) <= 2 ||dC|| / (eig[1] - eig[0]) with ||dC|| <= 3 (4 n u max_dist) + SOLVER_C u eig[2] (the solvers'
               backward error taken at its forward bound), plus 1e-14 for the orthonormality both solvers are held to.  Compared up to sign,
               and only where (eig[1] - eig[0]) / eig[2] >= GAP_MIN = 1e-3: below it the eigenvector of eig[0] is not a property of the
               ball any more.  tests/test_map_surface_ref.py asserts that these are at most 1 % of the valid queries.
  mean         the centroid q + s1 / n: n u sqrt(max_dist) from the order of s1's terms, and one rounding of the final sum at the size
               of the coordinate: 2 u (|q| + sqrt(max_dist)).
  curvature    c = e0 / S, S = e0 + e1 + e2:  |dc| <= (|de0| + c |dS|) / S + 4 u with |dS| <= 3 eig_bound; compared where S > 0.
  crispness    per used point |dh| <= 0.5 sum_k |d lambda_k| / lambda_k (first order, and the reference test asserts that no used point is
               within 1e6 of the degeneracy threshold, so lambda_0 >= 1e-6 eig[2] >> its bound), plus the ulp of log: three logarithms
               within 2 ulp of their size each (the device's log is documented to 1 ulp; numpy's likewise), 2 u sum_k |ln lambda_k|.  The
               mean of n_used such terms in another order moves by n_used u mean|h|: added once.  mpv likewise from the bound of eig[0];
               mean_count is an exact integer sum divided once: 2 u mean_count.
PROBE (tests/test_map_surface_ref.py repeats it): on the small_world hall, the same float64 sums taken in reverse order move C by at
most 2 % of the bound above at max_dist 0.04, 0.25 and 1.0 - the bound is safe, and still eleven orders below any real defect (a
dropped point moves C by max_dist / n)."""
import numpy as np

from map_nearest_cases import query_set
from map_radius_cases import Balls

U = 2.0 ** -53
SOLVER_C = 56.0  # 4 x the worst |lii_sym3_eigen - eigh| / (u eig[2]) measured by tests/test_sym3_eigen.py (14)
GAP_MIN = 1e-3
MAX_DISTS = (0.04, 0.25, 1.0)
DEGENERATE = 1e-12  # lii_map_crispness: eig[0] <= DEGENERATE * eig[2]
LN_2PIE_3 = 3.0 * np.log(2.0 * np.pi * np.e)


def mix(pts):
    """The selection hash of lii_map_crispness over the points' float bits, in uint32 arithmetic."""
    b = np.ascontiguousarray(pts, np.float32).view(np.uint32).reshape(-1, 3)
    with np.errstate(over="ignore"):
        h = (b[:, 0] * np.uint32(0x9E3779B1)) ^ (b[:, 1] * np.uint32(0x85EBCA77)) ^ (b[:, 2] * np.uint32(0xC2B2AE3D))
    return h ^ (h >> np.uint32(15))


def selected(pts, every):
    return mix(pts) % np.uint32(every) == 0


class Surface:
    """The reference records of the queries q over the map pts at max_dist, from the balls `case` = (offsets, idx, d2) of a Balls."""

    def __init__(self, q, pts, case, max_dist, reverse=False):
        off, idx, _ = case
        q = np.asarray(q, np.float32)
        n_q = len(off) - 1
        seg = np.repeat(np.arange(n_q), np.diff(off))
        d = np.asarray(pts, np.float32)[idx].astype(np.float64) - q[seg].astype(np.float64)
        if reverse:  # (the probe: the same terms in the opposite order)
            seg, d = seg[::-1], d[::-1]
        with np.errstate(invalid="ignore"):
            d = np.where(np.isfinite(d), d, 0.0)  # (a NaN query has no points: nothing of it is summed)
        n = np.diff(off).astype(np.float64)
        s1 = np.stack([np.bincount(seg, weights=d[:, a], minlength=n_q) for a in range(3)], axis=1)
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        s2 = np.stack([np.bincount(seg, weights=d[:, a] * d[:, b], minlength=n_q) for a, b in pairs], axis=1)
        self.max_dist = float(max_dist)
        self.count = np.diff(off).astype(np.int64)
        self.valid = self.count >= 3
        nn = np.where(n > 0, n, 1.0)
        mr = s1 / nn[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            self.mean = np.where((self.count > 0)[:, None], q.astype(np.float64) + mr, 0.0)
        c6 = np.stack([s2[:, k] / nn - mr[:, a] * mr[:, b] for k, (a, b) in enumerate(pairs)], axis=1)
        c6[~self.valid] = 0.0
        self.c6 = c6
        C = np.zeros((n_q, 3, 3))
        for k, (a, b) in enumerate(pairs):
            C[:, a, b] = c6[:, k]
            C[:, b, a] = c6[:, k]
        w, v = np.linalg.eigh(C)
        self.eig_raw = w
        self.eig = np.where(self.valid[:, None], np.maximum(w, 0.0), 0.0)
        self.normal = np.where(self.valid[:, None], v[:, :, 0], 0.0)
        s = self.eig.sum(axis=1)
        self.curvature = np.where(s > 0, self.eig[:, 0] / np.where(s > 0, s, 1.0), 0.0)
        self.q = q

    # ---- the bounds of the module docstring, per query
    def c_bound(self):
        return 4.0 * self.count * U * self.max_dist

    def eig_bound(self):
        return 3.0 * self.c_bound() + SOLVER_C * U * self.eig[:, 2]

    def gap(self):
        """(eig[1] - eig[0]) / eig[2]; 0 where the query is not valid or eig[2] is 0"""
        e = self.eig
        return np.where(self.valid & (e[:, 2] > 0), (e[:, 1] - e[:, 0]) / np.where(e[:, 2] > 0, e[:, 2], 1.0), 0.0)

    def normal_checked(self):
        return self.valid & (self.gap() >= GAP_MIN)

    def sin_bound(self):
        e = self.eig
        g = np.where(e[:, 1] - e[:, 0] > 0, e[:, 1] - e[:, 0], 1.0)
        return 2.0 * self.eig_bound() / g + 1e-14

    def mean_bound(self):
        r = np.sqrt(self.max_dist)
        with np.errstate(invalid="ignore"):
            size = np.nan_to_num(np.abs(self.q.astype(np.float64)).max(axis=1), nan=0.0, posinf=0.0) + r
        return self.count * U * r + 2.0 * U * size

    def curvature_bound(self):
        s = self.eig.sum(axis=1)
        s = np.where(s > 0, s, 1.0)
        return (self.eig_bound() + self.curvature * 3.0 * self.eig_bound()) / s + 4.0 * U


def check_records(rec, ref, who, normals=True):
    """Holds the device's records (SURFACE_DTYPE) to the reference: counts and valid equal, the rest within the derived bounds.  Prints
    each figure (as a share of its bound) before it asserts.  Returns the number of valid queries whose normal was not compared."""
    assert rec.dtype.itemsize == 88 and len(rec) == len(ref.count)
    n_cnt = int(np.count_nonzero(rec["count"] != ref.count))
    print(f"{who}: {len(rec)} queries, populations 0 - {int(ref.count.max(initial=0))}, counts differ {n_cnt}, valid {int(ref.valid.sum())}")
    assert n_cnt == 0, f"{who}: counts differ from the brute force"
    assert np.array_equal(rec["valid"], ref.valid.astype(np.int32)), f"{who}: valid != (count >= 3)"
    inv = ~ref.valid
    assert not rec["eig"][inv].any() and not rec["normal"][inv].any() and not rec["curvature"][inv].any(), f"{who}: an invalid record is not zeros"
    assert not rec["mean"][ref.count == 0].any()
    has = ref.count > 0
    dm = np.abs(rec["mean"][has] - ref.mean[has]).max(axis=1) / ref.mean_bound()[has] if has.any() else np.zeros(0)
    v = ref.valid
    de = np.abs(rec["eig"][v] - ref.eig[v]).max(axis=1) / np.maximum(ref.eig_bound()[v], 1e-300) if v.any() else np.zeros(0)
    dc = np.abs(rec["curvature"][v] - ref.curvature[v]) / ref.curvature_bound()[v] if v.any() else np.zeros(0)
    print(f"{who}: mean {dm.max(initial=0):.3g}, eig {de.max(initial=0):.3g}, curvature {dc.max(initial=0):.3g} of their bounds")
    assert np.all(dm <= 1.0), f"{who}: a centroid is off by {dm.max():.3g} x its bound"
    assert np.all(de <= 1.0), f"{who}: an eigenvalue is off by {de.max():.3g} x its bound"
    assert np.all(dc <= 1.0), f"{who}: a curvature is off by {dc.max():.3g} x its bound"
    assert np.all(np.diff(rec["eig"], axis=1) >= 0) and np.all(rec["eig"] >= 0), f"{who}: eig not ascending or negative"
    nrm = np.linalg.norm(rec["normal"][v], axis=1)
    assert np.all(np.abs(nrm - 1.0) <= 1e-14), f"{who}: a normal is not a unit vector"
    left_out = int(np.count_nonzero(v & ~ref.normal_checked()))
    if normals:
        ck = ref.normal_checked()
        sin = np.linalg.norm(np.cross(rec["normal"][ck], ref.normal[ck]), axis=1) / np.maximum(ref.sin_bound()[ck], 1e-300)
        print(f"{who}: normals compared {int(ck.sum())}, left out {left_out}, sin(angle) {sin.max(initial=0):.3g} of its bound")
        assert np.all(sin <= 1.0), f"{who}: a normal is off by {sin.max():.3g} x its bound"
        assert left_out <= 0.01 * max(int(v.sum()), 1), f"{who}: more than 1 % of the normals were left out"
    return left_out


def crispness_reference(pts, max_dist, min_count, every, chunk=64):
    """lii_map_crispness over the map `pts` by the reference: (figures dict, bounds dict, the Surface of the selected points)."""
    pts = np.ascontiguousarray(pts, np.float32)
    sel = selected(pts, every)
    q = pts[sel]
    ref = Surface(q, pts, Balls(q, pts, max_dist, chunk=chunk).case(max_dist), max_dist)
    sparse = ref.count < min_count
    degenerate = ~sparse & (ref.eig[:, 0] <= DEGENERATE * ref.eig[:, 2])
    used = ~sparse & ~degenerate
    out = dict(n_selected=int(sel.sum()), n_used=int(used.sum()), n_sparse=int(sparse.sum()), n_degenerate=int(degenerate.sum()), mme=0.0, mpv=0.0, mean_count=0.0)
    bounds = dict(mme=0.0, mpv=0.0, mean_count=0.0)
    if used.any():
        e, eb = ref.eig[used], ref.eig_bound()[used]
        h = 0.5 * (LN_2PIE_3 + np.log(e[:, 0]) + np.log(e[:, 1]) + np.log(e[:, 2]))
        nu = float(used.sum())
        out.update(mme=float(h.mean()), mpv=float(e[:, 0].mean()), mean_count=float(ref.count[used].mean()))
        dh = 0.5 * (eb[:, None] / e).sum(axis=1) + 2.0 * U * np.abs(np.log(e)).sum(axis=1)
        bounds.update(mme=float(dh.mean() + nu * U * np.abs(h).mean()), mpv=float(eb.mean() + nu * U * e[:, 0].mean()),
                      mean_count=2.0 * U * out["mean_count"])
    ref.used, ref.sparse, ref.degenerate = used, sparse, degenerate
    return out, bounds, ref


def check_crispness(got, expected, bounds, who):
    for k in ("n_selected", "n_used", "n_sparse", "n_degenerate"):
        print(f"{who}: {k} {got[k]} (reference {expected[k]})")
    for k in ("mme", "mpv", "mean_count"):
        print(f"{who}: {k} {got[k]!r} (reference {expected[k]!r}), off by {abs(got[k] - expected[k]):.3g}, bound {bounds[k]:.3g}")
    for k in ("n_selected", "n_used", "n_sparse", "n_degenerate"):
        assert got[k] == expected[k], f"{who}: {k}"
    assert got["n_selected"] == got["n_used"] + got["n_sparse"] + got["n_degenerate"]
    for k in ("mme", "mpv", "mean_count"):
        assert abs(got[k] - expected[k]) <= bounds[k], f"{who}: {k} off by {abs(got[k] - expected[k]):.3g}, bound {bounds[k]:.3g}"


_cache = {}


def small_world_surface(small_world):
    """The 2 000-query set over the suite's hall map, its balls up to d2 = 1 and the reference records at MAX_DISTS, once per session."""
    if "sw" not in _cache:
        hall, map_pts = small_world
        map_pts = np.ascontiguousarray(map_pts, np.float32)
        q = query_set(hall, map_pts)
        balls = Balls(q, map_pts, max(MAX_DISTS))
        _cache["sw"] = (q, balls, {md: Surface(q, map_pts, balls.case(md), md) for md in MAX_DISTS})
    return _cache["sw"]


CRISP_WORLD = dict(max_dist=0.25, min_count=5, every=16)


def small_world_crispness(small_world):
    """lii_map_crispness over the suite's hall map at CRISP_WORLD by the reference, once per session."""
    if "crisp" not in _cache:
        _cache["crisp"] = crispness_reference(np.ascontiguousarray(small_world[1], np.float32), **CRISP_WORLD)
    return _cache["crisp"]


def sheet_map(noise=0.0, n=5000, seed=61):
    """The hand-made map of the crispness tests: two perpendicular sheets of n points in all, 1 cm rough, plus `noise` metres of uniform
    noise on them; beside them, untouched by the noise, 40 lone points 2 m apart (sparse balls at max_dist <= 1) and 9 points of an
    axis-parallel dyadic line (a ball of 9 whose covariance has two eigenvalues that are exactly zero: degenerate)."""
    rng = np.random.default_rng(seed)
    a = np.c_[rng.uniform(-3, 3, (n // 2, 2)), rng.normal(0, 0.01, n // 2)]
    b = np.c_[rng.uniform(-3, 3, n - n // 2), rng.normal(3.0, 0.01, n - n // 2), rng.uniform(0, 3, n - n // 2)]
    pts = np.concatenate([a, b])
    if noise:
        pts = pts + np.random.default_rng(seed + 1).uniform(-noise, noise, pts.shape)
    lone = np.array([[20.0 + 2.0 * i, -20.0 + 2.0 * j, 5.0] for i in range(8) for j in range(5)])
    line = np.array([[-20.0 + k / 32.0, 12.5, -4.0] for k in range(9)])
    return np.ascontiguousarray(np.concatenate([pts, lone, line]), np.float32)

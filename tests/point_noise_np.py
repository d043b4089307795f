"""One scan point's measurement noise from its range and bearing - the 3 x 3 covariance the reference program forms for every selected point
and then discards - restated in numpy float64 with float32 casts where the reference has them, and what tests/test_point_noise_host.py
(CPU) and tests/test_gpu_point_noise.py (device) need around it.  No GPU is touched here.

Written from the reference program: src/laserMapping.cpp:158-181 (calcBodyVar) and :1039-1051 (its call site, the rotation into the world
frame, R_inv(i) = 1000 and the intensity sqrt(R_inv(i))) - not from the kernels.  World point, plane, gates and Jacobian row are
tests/plane_rows_np.py's.

  calc_body_var_literal   calcBodyVar as written: `range` and `range_var` floats, the tangent basis (1, 1, -(dx + dy) / dz) - not finite for a
                          point with z = 0 in the IMU frame
  sigma2_literal          LASER_POINT_COV + n^T (R_end var R_end^T) n with that var
  sigma2_closed           the basis-free form the library computes: N is an orthonormal basis of the ray's tangent plane, so
                          A diag(s^2) A^T = s^2 r^2 (I - d d^T) and, with t = R_end^T n, A = p_I x t, u = t . p_I, r^2 = |p_I|^2,
                              sigma^2 = 1 / rinv + sr2 u^2 / r^2 + s2 |A|^2          (the radial term 0 when r^2 == 0)
"""
import math

import numpy as np

import plane_rows_np as pr

F32, F64 = np.float32, np.float64
RANGE_INC, DEGREE_INC = 0.02, 0.05   # the arguments at src/laserMapping.cpp:1041
DEG2RAD = 0.017453293                # PCL's DEG2RAD macro as the reference compiles it (restated from knowledge of PCL, not pinned by a build)
W_EPS = 8 * 2.0 ** -52               # the weight's own double operations: two reciprocals, the square root, its square, two products


def noise_constants(range_inc=RANGE_INC, degree_inc=DEGREE_INC):
    """(sr2, s2): range_var - range_inc is a float, and so is the product (:158, :161) - and sin(DEG2RAD(degree_inc))^2 (:163)."""
    ri = F32(range_inc)
    sr2 = F64(F32(ri * ri))
    s2 = math.sin(float(F64(F32(degree_inc))) * DEG2RAD) ** 2
    return float(sr2), float(s2)


def _normalized(v):
    return v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])   # Eigen's normalize(): v /= sqrt(squaredNorm)


def calc_body_var_literal(pb, range_inc=RANGE_INC, degree_inc=DEGREE_INC):
    """calcBodyVar(pb, range_inc, degree_inc, var) (:158-181), line for line."""
    pb = np.asarray(pb, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rng = F64(F32(np.sqrt(pb[0] * pb[0] + pb[1] * pb[1] + pb[2] * pb[2])))                 # float range (:160)
        sr2, s2 = noise_constants(range_inc, degree_inc)                                    # float range_var (:161), direction_var (:162-164)
        direction_var = np.diag([s2, s2])
        d = _normalized(pb)                                                                 # :165-166
        d_hat = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])      # :167-169
        b1 = _normalized(np.array([1.0, 1.0, -(d[0] + d[1]) / d[2]]))                       # :170-172
        b2 = _normalized(np.cross(b1, d))                                                   # :173-174
        N = np.c_[b1, b2]                                                                   # :175-177
        A = (rng * d_hat) @ N                                                               # :178
        return np.outer(d * sr2, d) + (A @ direction_var) @ A.T                             # :179-180


def sigma2_literal(p_imu, R_end, normal_f32, rinv=pr.RINV, range_inc=RANGE_INC, degree_inc=DEGREE_INC):
    """LASER_POINT_COV + n^T (rot_end var rot_end^T) n (:1041-1042 and the weight the update would take from it)."""
    n = np.asarray(normal_f32, F32).astype(F64)
    R = np.asarray(R_end, F64)
    with np.errstate(invalid="ignore"):
        var = (R @ calc_body_var_literal(p_imu, range_inc, degree_inc)) @ R.T
        return 1.0 / rinv + float(n @ var @ n)


def sigma2_closed(p_imu, R_end, normal_f32, rinv=pr.RINV, range_inc=RANGE_INC, degree_inc=DEGREE_INC):
    p = np.asarray(p_imu, F64)
    n = np.asarray(normal_f32, F32).astype(F64)
    t = np.asarray(R_end, F64).T @ n
    A = np.cross(p, t)
    u = float(t @ p)
    r2 = float(p @ p)
    sr2, s2 = noise_constants(range_inc, degree_inc)
    radial = sr2 * (u * u) / r2 if r2 > 0.0 else 0.0
    return 1.0 / rinv + radial + s2 * float(A @ A)


# --------------------------------------------------------------------------------------------------------------------------------- one point's row
def p_imu_of(pose, body_f32):
    """point_this = offset_R_L_I * point_this_L + offset_T_L_I (:1039), one rounding per operation."""
    pb = np.asarray(body_f32, F32).astype(F64)
    return (pose.RLI[:, 0] * pb[0] + pose.RLI[:, 1] * pb[1]) + pose.RLI[:, 2] * pb[2] + pose.TLI


def weight_of(pose, r, range_inc=RANGE_INC, degree_inc=DEGREE_INC, rinv=pr.RINV):
    """R_inv_i of a selected point (r: a plane_rows_np.point_row dict of a pass at `pose`); 0.0 for a point that is not selected."""
    if not r["selected"]:
        return 0.0
    normal = r["plane"]["pabcd"][:3].astype(F32)
    return 1.0 / sigma2_closed(p_imu_of(pose, r["body"]), pose.R, normal, rinv, range_inc, degree_inc)


def weighted_out(r, w):
    """The 91 sums of one point under its own weight: w h h^T (upper triangle), w h z, 1."""
    if not r["selected"]:
        return np.zeros(91)
    G = w * np.outer(r["h"], r["h"])
    return np.r_[G[pr._IU], w * r["h"] * r["z"], 1.0]


def group_ratios(out, r, w, tol_hh, tol_hz, family, ref_out=None):
    """plane_rows_np.group_ratios with the point's own weight where that one has RINV: (worst |out - ref| over w |h|^2 on [0:78]) / tol_hh
    and (worst over w |h| |z| on [78:90]) / tol_hz, a flagged pd2's one float ulp taken off first."""
    h, z = r["h"], abs(r["z"])
    hn = math.sqrt(float(h @ h))
    d = np.abs(np.asarray(out) - (weighted_out(r, w) if ref_out is None else ref_out))
    a = 0.0 if hn == 0 else float(d[:78].max()) / (w * hn * hn)
    rest = d[78:90]
    if pr.pd2_flagged(r, family):
        rest = np.maximum(rest - pr._ulp32(r["pd2"]) * w * np.abs(h), 0.0)
    if z == 0 or hn == 0:
        b = 0.0 if rest.max() == 0 else np.inf
    else:
        b = float(rest.max()) / (w * hn * z)
    return a / tol_hh, b / tol_hz


def ulp32_apart(a, b):
    """Distance of two positive finite floats in units in the last place."""
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


# --------------------------------------------------------------------------------------------------------------------------------- the cases
class NoiseCases(pr.Cases):
    """plane_rows_np.Cases (every family, the same sites and queries) plus family K: per pose, clusters 12, 25 and 60 m out whose queries have
    z = 0 in the IMU frame - exactly, where offset_R_L_I is the identity ("identity", "lo"); to rounding under "lio" - the points
    calcBodyVar's tangent basis is not finite for.  Each cluster has a query 1 cm off its plane and one 1.3 m along it, both with z_I = 0.
    Ranges under 1 m are family J's (|p_body| = 0.5 m), ranges of 60 m families A, J and K's."""

    def __init__(self):
        super().__init__()
        self._family_k()
        self.map = np.ascontiguousarray(np.concatenate([self.filler_pts] + [c["pts"] for c in self.nh]), F32)
        self._check_isolation()

    def _family_k(self):
        rng = np.random.default_rng(1301)
        for name, pose in pr.POSES.items():
            for norm in (12.0, 25.0, 60.0):
                for _ in range(4000):
                    ang = rng.uniform(0, 2 * np.pi)
                    e = np.array([-np.sin(ang), np.cos(ang), 0.0])           # along the ring, z_I = 0
                    pis = [np.array([np.cos(ang), np.sin(ang), 0.0]) * norm + k * 1.3 * e for k in (0, 1)]
                    bodies = [(pose.RLI.T @ (p - pose.TLI)).astype(F32) for p in pis]
                    c0, c1 = (pose.forward(b).astype(F64) for b in bodies)
                    # (a query must stay REACH + 0.2 away from every other cluster's points, and the other clusters' queries - up to 1.3 m
                    # from their centres - from this cluster's: 4.4 m between centres, 3.2 m from the far query; _check_isolation has the last word)
                    if all(np.linalg.norm(n_["centre"] - c0) > 4.4 and np.linalg.norm(n_["centre"] - c1) > 3.2 for n_ in self.nh) and \
                            min(np.linalg.norm(self.filler_pts[0] - c0), np.linalg.norm(self.filler_pts[0] - c1)) > 8:
                        break
                else:
                    raise AssertionError("no free place")
                e_w = pr._unit(c1 - c0)
                while True:
                    v = rng.normal(0, 1, 3)
                    normal = pr._unit(v - (v @ e_w) * e_w)                    # the plane holds the direction to the far query
                    pts = self._patch(rng, c0 - 0.01 * normal, normal, 0.3, np.zeros(5))
                    if self._decided(pts):
                        break
                nh = self._add("K", pts, f"{name} |p| {norm}")
                self._query(nh, c0, "near", pose=name, body=bodies[0], tag="z_I = 0")
                self._query(nh, c1, "far", pose=name, body=bodies[1], tag="z_I = 0")


_noise_cases = None


def noise_cases():
    global _noise_cases
    if _noise_cases is None:
        _noise_cases = NoiseCases()
    return _noise_cases


def moved_pose(name, oracle_state_boxplus, state_init):
    """The pose of the cached-plane pass: state [+] plane_rows_np.MOVE."""
    pod2 = oracle_state_boxplus(pr.POSES[name].pod(state_init), pr.MOVE)
    return pr.Pose.from_pod(name + " moved", pod2), pod2

"""One scan point's share of a registration pass - world point, plane of its five neighbours, the two gates, its Jacobian row and the 91
sums it contributes - restated in numpy float64 with float32 casts where the reference program has them, and the neighbourhoods that
tests/test_plane_rows_host.py (CPU) and tests/test_gpu_plane_rows.py (device) run it on.  No GPU is touched here.

Written from the reference program: include/common_lib.h:236-269 (esti_plane) and src/laserMapping.cpp:209-220 (pointBodyToWorld),
:957-1012 (search, plane, gates), :1035-1071 (Jacobian row, R^-1, measurement) - not from the kernels and not from oracle/orc_*.hpp.
The column-pivoted QR is the one of tests/test_oracle_plane_degenerate.py.

Why one point can be checked through the public calls: lii_iekf_iterate returns the 91 sums of the scan; with ONE point in the scan, or
with one live point among points whose rows are exactly zero, the sums ARE that point's row - out[0:78] = rinv h h^T (upper triangle),
out[78:90] = rinv h z, out[90] = 0 or 1 - and no summation order is involved.  The map is a set of isolated clusters (nothing else within
sqrt(5) m of a query), so every query's five neighbours are known by construction.

Measured figures (the constants below) and what the device showed: profiles/plane_rows.md.
"""
import math

import numpy as np

from test_oracle_plane_degenerate import colpiv_qr_solve_numpy

F32, F64 = np.float32, np.float64
RINV = 1000.0            # lii_config::laser_point_cov_inv as the Registrar sets it (R_inv(i) = 1000, src/laserMapping.cpp:1050)
PLANE_THR = 0.1          # esti_plane's threshold at its call site (:997)
MAX_D2 = F32(5.0)
LATTICE = 8.0
SITE_MAX = 64.0
REACH = math.sqrt(5.0)

# ---------------------------------------------------------------------------------------------------------------------------------
# CPU discrepancy between the two references (oracle C++ against this file) on the cases below, every pose: the worst entry-wise
# difference per group as tests/test_plane_rows_host.py measures it (profiles/plane_rows.md has the run).  The device is held to
# DEVICE_FACTOR x these against each reference; a case is left out of a comparison only where one of its rounding / threshold distances
# is below EXCLUDE_FACTOR x the figure of that quantity.
# The plane's figures are kept per family: the millimetre patches of family G are worse conditioned than everything else by two orders of
# magnitude, and one figure for all would leave out a share of every family that exceeds the cap.
_FAMILIES = tuple("ABCDEFGHIJ") + ("A0",)   # (Z, the all-zero matrix, has no finite plane to measure)
DISC = dict(
    hh=2.2e-15,      # out[0:78], over rinv |h|^2
    hz=1.9e-15,      # out[78:90], over rinv |h| |z| (after pd2's allowance where flagged)
    # the plane's unit normal, absolute (components <= 1)
    normal=dict(zip(_FAMILIES, (2.9e-13, 8.4e-14, 3.6e-14, 0.0, 3.9e-14, 5.9e-14, 1.4e-11, 1.7e-13, 4.9e-15, 5.3e-15, 6.7e-15))),
    # the plane's d, over max(1, |d|)
    d=dict(zip(_FAMILIES, (3.2e-13, 1.4e-14, 5.4e-14, 0.0, 2.6e-14, 3.4e-13, 2.7e-11, 1.3e-13, 1.2e-14, 7.0e-14, 4.5e-15))),
    # pd2 before its cast to float (and the plane's residuals at the five points), over max(1, |d|)
    pd2=dict(zip(_FAMILIES, (1.4e-14, 1.1e-15, 1.3e-15, 0.0, 1.5e-15, 1.6e-14, 2.2e-13, 4.9e-15, 2.4e-16, 1.6e-15, 3.3e-15))),
)
# The device (MI355X, tests/test_gpu_plane_rows.py -s; the table is in the profile): worst difference from either reference 0.164 of the
# tolerance on out[0:78] and 0.144 on out[78:90] in the search pass, 0.117 and 0.142 on cached planes; nothing left out.
DISC_S = 2.0 ** -52 # s before its cast to float: the same float pd2 goes in, what differs is the last place of a double in [0, 1]
DEVICE_FACTOR = 8.0
EXCLUDE_FACTOR = 64.0
EXCLUDE_CAP = 0.02


# --------------------------------------------------------------------------------------------------------------------------------- poses
def _rot_zyx(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


class Pose:
    """rot_end, pos_end, offset_R_L_I, offset_T_L_I (include/common_lib.h:68-169)."""

    def __init__(self, name, R, p, RLI=None, TLI=None):
        self.name = name
        self.R, self.p = np.array(R, F64), np.array(p, F64)
        self.RLI = np.eye(3) if RLI is None else np.array(RLI, F64)
        self.TLI = np.zeros(3) if TLI is None else np.array(TLI, F64)

    @classmethod
    def from_pod(cls, name, pod):
        return cls(name, pod[0:9].reshape(3, 3), pod[9:12], pod[12:21].reshape(3, 3), pod[21:24])

    def pod(self, state_init):
        """The 612-double state with this pose (state_init: a fresh StatesGroup POD)."""
        s = np.array(state_init, F64)
        s[0:9], s[9:12], s[12:21], s[21:24] = self.R.reshape(-1), self.p, self.RLI.reshape(-1), self.TLI
        return s

    def forward(self, body_f32):
        """pointBodyToWorld (:209-220): double arithmetic on the float body point, stored as float."""
        pb = np.asarray(body_f32, F32).astype(F64)
        # (written out, one rounding per operation: the float the world point rounds to must not depend on whether a BLAS fuses a
        # multiply-add - the lists are exact, and a query whose world coordinate is a cancellation shows the last bit)
        pi = (self.RLI[:, 0] * pb[0] + self.RLI[:, 1] * pb[1]) + self.RLI[:, 2] * pb[2] + self.TLI
        g = (self.R[:, 0] * pi[0] + self.R[:, 1] * pi[1]) + self.R[:, 2] * pi[2] + self.p
        return g.astype(F32)

    def inverse(self, world):
        """A float body point whose world point is close to `world` (the tests recompute the world point forwards)."""
        w = np.asarray(world, F64)
        return (self.RLI.T @ (self.R.T @ (w - self.p) - self.TLI)).astype(F32)


POSES = {
    "identity": Pose("identity", np.eye(3), np.zeros(3)),
    "lo": Pose("lo", _rot_zyx(0.21, -0.13, 0.57), [3.7, -4.3, 3.6]),
    "lio": Pose("lio", _rot_zyx(-0.11, 0.17, -0.83), [-4.1, 3.4, -4.5], _rot_zyx(0.10, -0.20, 0.30), [0.30, -0.20, 0.50]),
}
# (pose, imu_en): the LIO pose runs with the extrinsic columns on and off
CONFIGS = (("identity", False), ("lo", False), ("lio", True), ("lio", False))
# the cached-plane pass runs at state [+] these (tests/test_gpu_register.py's second pass)
MOVE = np.r_[0.001, -0.002, 0.0015, 0.01, -0.005, 0.004, np.zeros(18)]


# --------------------------------------------------------------------------------------------------------------------------------- one point
def dist2_f32(q, p):
    """KD_TREE::calc_dist in float32, every operation rounded on its own: (dx dx + dy dy) + dz dz."""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    dx, dy, dz = q[..., 0] - p[..., 0], q[..., 1] - p[..., 1], q[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def nearest5(world_f32, pts_f32):
    """The list Nearest_Search(point_world, 5, ..., max_dist 5) returns from `pts` (a cluster: brute force): the points with d^2 <= 5,
    ascending, equal distances by x (PointType_CMP, include/ikd-Tree/ikd_Tree.h:50-61).  Returns (points (5, 3), d2 (5,), count)."""
    pts = np.asarray(pts_f32, F32).reshape(-1, 3)
    d = dist2_f32(np.asarray(world_f32, F32)[None, :], pts)
    keep = np.flatnonzero(d <= MAX_D2)
    order = keep[np.lexsort((pts[keep, 0], d[keep]))][:5]
    out, od = np.zeros((5, 3), F32), np.full(5, np.inf, F32)
    out[:len(order)], od[:len(order)] = pts[order], d[order]
    return out, od, len(order)


def _to_rounding_boundary(v):
    """Distance of the double v to the nearest point where its float32 rounding changes."""
    if not np.isfinite(v) or v == 0.0:   # (an exact zero - the component a rank-deficient solve drops - is a zero in any implementation)
        return np.inf
    f = F32(v)
    lo, hi = np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))
    return min(abs(v - (F64(f) + F64(lo)) / 2), abs(v - (F64(f) + F64(hi)) / 2))


# float s > 0.9 (a double constant): true from the first float above 0.9 on; the double s rounds there from this midpoint
_S_LO = F32(0.9)
_S_EDGE = (F64(_S_LO) + F64(np.nextafter(_S_LO, F32(1)))) / 2 if F64(_S_LO) < 0.9 else (F64(_S_LO) + F64(np.nextafter(_S_LO, F32(0)))) / 2


def esti_plane(nb):
    """esti_plane<double> (include/common_lib.h:236-269) on five float points.  Returns dict(ok, pabcd, res (the five residuals, signed),
    diag (nonzero_pivots, perm, tau0, renorm))."""
    A = np.asarray(nb, F32).astype(F64).reshape(5, 3)
    diag = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        n, _ = colpiv_qr_solve_numpy(A, -np.ones(5), diag)
        nn = np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
        pabcd = np.r_[n / nn, 1.0 / nn]
        res = pabcd[0] * A[:, 0] + pabcd[1] * A[:, 1] + pabcd[2] * A[:, 2] + pabcd[3]
        ok = not bool(np.any(np.abs(res) > PLANE_THR))   # (a NaN residual is not > threshold: the reference returns true)
    return dict(ok=ok, pabcd=pabcd, res=res, diag=diag)


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def jacobian_row(pose, imu_en, body_f32, normal_f32):
    """Hsub.row(i) (:1035-1066): products left to right, the normal read back from its floats."""
    pL = np.asarray(body_f32, F32).astype(F64)
    p_this = pose.RLI @ pL + pose.TLI
    nv = np.asarray(normal_f32, F32).astype(F64)
    Rt = pose.R.T
    h = np.zeros(12)
    h[0:3] = (_skew(p_this) @ Rt) @ nv
    h[3:6] = nv
    if imu_en:
        h[6:9] = ((_skew(pL) @ pose.RLI.T) @ Rt) @ nv
        h[9:12] = Rt @ nv
    return h


_IU = np.triu_indices(12)


def sums_of_row(h, z):
    """The 91 sums of one selected point: H^T R^-1 H (upper triangle, row-major), H^T R^-1 z, 1."""
    G = RINV * np.outer(h, h)
    return np.r_[G[_IU], RINV * h * z, 1.0]


def point_row(pose, imu_en, body_f32, cluster=None, cached=None):
    """One point of one pass.  cluster: the points the search can reach (a search pass); cached: the dict a search pass returned for the
    same point (a pass on cached planes: list, plane and selection of that pass, the pose is the new one).
    Returns dict(world, nb, d2, count, plane (dict or None), candidate, pd2, s, selected, h, z, out (91,), margin (dict), flag_pd2)."""
    body = np.asarray(body_f32, F32)
    world = pose.forward(body)
    r = dict(body=body, world=world, margin={}, selected=False, h=np.zeros(12), z=0.0, out=np.zeros(91), pd2=F32(0), s=F32(0), plane=None)
    if cached is None:
        r["nb"], r["d2"], r["count"] = nearest5(world, cluster)
        candidate = r["count"] == 5 and not (r["d2"][4] > MAX_D2)
        r["margin"]["d5"] = abs(float(r["d2"][4]) - 5.0) if r["count"] == 5 else np.inf
        plane = None
        if candidate:
            plane = esti_plane(r["nb"])
            r["margin"]["res"] = float(np.min(np.abs(np.abs(plane["res"]) - PLANE_THR))) if np.all(np.isfinite(plane["res"])) else np.inf
            candidate = plane["ok"]
        r["plane"] = plane
    else:
        r["nb"], r["d2"], r["count"], r["plane"] = cached["nb"], cached["d2"], cached["count"], cached["plane"]
        candidate = bool(cached["selected"])   # point_selected_surf[i] stays as the last pass left it (:989)
        plane = cached["plane"]
    r["candidate"] = candidate
    if not candidate:
        return r
    pabcd = plane["pabcd"]
    w = world.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pd2_d = pabcd[0] * w[0] + pabcd[1] * w[1] + pabcd[2] * w[2] + pabcd[3]
        pd2 = F32(pd2_d)
        pb = body.astype(F64)
        s_d = 1 - 0.9 * abs(F64(pd2)) / np.sqrt(np.sqrt(pb[0] * pb[0] + pb[1] * pb[1] + pb[2] * pb[2]))
        s = F32(s_d)
    r["pd2"], r["s"], r["pd2_double"] = pd2, s, pd2_d
    r["margin"]["pd2"] = _to_rounding_boundary(pd2_d)
    r["margin"]["s"] = abs(s_d - _S_EDGE) if np.isfinite(s_d) else np.inf
    r["margin"]["n"] = min(_to_rounding_boundary(v) for v in pabcd[:3])
    if F64(s) > 0.9:
        r["selected"] = True
        normal = pabcd[:3].astype(F32)
        r["h"] = jacobian_row(pose, imu_en, body, normal)
        r["z"] = -F64(pd2)
        r["out"] = sums_of_row(r["h"], r["z"])
    return r


def excluded(r, family, disc=None):
    """Whether a point's comparison is left out: a float rounding of its normal or a gate decision sits within EXCLUDE_FACTOR x the CPU
    discrepancy of that quantity (pd2's rounding is not a reason: see pd2_allowance)."""
    disc = DISC if disc is None else disc
    pl = r["plane"]
    if pl is None or not np.all(np.isfinite(pl["pabcd"])):
        return False
    scale = max(1.0, abs(pl["pabcd"][3]))
    m = r["margin"]
    if m.get("res", np.inf) < EXCLUDE_FACTOR * disc["pd2"].get(family, 0.0) * scale:
        return True
    if not r["candidate"]:
        return False
    return m["n"] < EXCLUDE_FACTOR * disc["normal"].get(family, 0.0) or m["s"] < EXCLUDE_FACTOR * DISC_S


def _ulp32(v):
    v = F32(abs(v))
    return float(np.nextafter(v, F32(np.inf)) - v)


def pd2_flagged(r, family, disc=None):
    """pd2's float rounding may legitimately differ between two correct implementations: its double value sits within EXCLUDE_FACTOR x
    the CPU discrepancy of a rounding boundary."""
    disc = DISC if disc is None else disc
    if not r["candidate"] or not r["selected"]:
        return False
    return r["margin"]["pd2"] < EXCLUDE_FACTOR * disc["pd2"].get(family, 0.0) * max(1.0, abs(r["plane"]["pabcd"][3]))


def group_ratios(out, ref_r, tol_hh, tol_hz, family, disc=None, ref_out=None):
    """(worst |out - ref| over rinv |h|^2 on [0:78]) / tol_hh and (worst over rinv |h| |z| on [78:90]) / tol_hz.  A flagged pd2 may move
    out[78:90] by one float32 ulp of pd2 times rinv |h_i|: that much is taken off first.  ref_out: the other reference's sums for the
    same point (the norms that scale the differences are this file's either way)."""
    h, z = ref_r["h"], abs(ref_r["z"])
    hn = math.sqrt(float(h @ h))
    d = np.abs(np.asarray(out) - (ref_r["out"] if ref_out is None else ref_out))
    a = 0.0 if hn == 0 else float(d[:78].max()) / (RINV * hn * hn)
    rest = d[78:90]
    if pd2_flagged(ref_r, family, disc):
        rest = np.maximum(rest - _ulp32(ref_r["pd2"]) * RINV * np.abs(h), 0.0)
    if z == 0 or hn == 0:
        b = 0.0 if rest.max() == 0 else np.inf
    else:
        b = float(rest.max()) / (RINV * hn * z)
    return a / tol_hh, b / tol_hz


# --------------------------------------------------------------------------------------------------------------------------------- the cases
def _unit(v):
    v = np.asarray(v, F64)
    return v / np.linalg.norm(v)


def _frame(n):
    n = _unit(n)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.8 else np.array([0.0, 1.0, 0.0])
    u = _unit(np.cross(n, a))
    return u, np.cross(n, u), n


class Cases:
    """nh: list of dict(family, tag, pts (k, 3) float32, centre); queries: list of dict(nh, world (float32 target), kind 'near' / 'far' /
    'other', pose (None: every pose; a name: that pose only), body (a fixed float32 body point, or None: the pose's inverse of `world`),
    tag).  filler_pts / filler_world: the cluster whose plane is rejected decisively and the query beside it."""

    def __init__(self):
        self.nh, self.queries, self._sites = [], [], set()
        self._build_filler()
        self._family_d()   # (the families that need sites on an axis or a coordinate plane choose first)
        self._family_c()
        self._family_i()
        self._family_g()
        self._family_a()
        self._family_b()
        self._family_e()
        self._family_f()
        self._family_h()
        self._family_j()
        self.map = np.ascontiguousarray(np.concatenate([self.filler_pts] + [c["pts"] for c in self.nh]), F32)
        self._check_isolation()

    # ------------------------------------------------------------------ plumbing
    def _site(self, target, fixed=None):
        """The free lattice site nearest to `target`; fixed: {axis: value} coordinates the site must have."""
        t = np.asarray(target, F64)
        base = np.clip(np.round(t / LATTICE), -SITE_MAX / LATTICE, SITE_MAX / LATTICE).astype(int)
        best = None
        for dx in range(-3, 4):
            for dy in range(-3, 4):
                for dz in range(-3, 4):
                    s = base + np.array([dx, dy, dz])
                    if fixed:
                        for a, v in fixed.items():
                            s[a] = v
                    if np.any(np.abs(s) > SITE_MAX / LATTICE) or tuple(s) in self._sites or tuple(s) == (0, 0, 0):
                        continue
                    d = float(np.sum((s * LATTICE - t) ** 2))
                    if best is None or d < best[0]:
                        best = (d, tuple(int(v) for v in s))
        assert best is not None, target
        self._sites.add(best[1])
        return np.array(best[1], F64) * LATTICE

    def _add(self, family, pts, tag=""):
        pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
        self.nh.append(dict(family=family, tag=tag, pts=pts, centre=pts.astype(F64).mean(axis=0)))
        return len(self.nh) - 1

    def _query(self, nh, world, kind, pose=None, body=None, tag=""):
        self.queries.append(dict(nh=nh, world=np.asarray(world, F32), kind=kind, pose=pose,
                                 body=None if body is None else np.asarray(body, F32), tag=tag))

    def _decided(self, pts, by=3e-11):
        """Whether the float roundings of the patch's normal are decided by more than `by` - some hundred times what two correct
        double-precision solves differ by on a well-conditioned patch.  The generators draw a patch again otherwise, so that few cases
        have to be left out of a comparison later (the cap is 2 % per family)."""
        pl = esti_plane(np.asarray(pts, F32))
        return bool(np.all(np.isfinite(pl["pabcd"]))) and min(_to_rounding_boundary(v) for v in pl["pabcd"][:3]) > by

    def _patch(self, rng, centre, normal, extent, offsets):
        """Five points: in a disc of diameter `extent` around centre in the plane of `normal`, offsets[i] along the normal."""
        u, v, n = _frame(normal)
        r = 0.5 * extent * np.sqrt(rng.uniform(0.15, 1.0, 5))
        ang = rng.uniform(0, 2 * np.pi) + 2 * np.pi * (np.arange(5) + rng.uniform(-0.3, 0.3, 5)) / 5
        return centre + np.outer(r * np.cos(ang), u) + np.outer(r * np.sin(ang), v) + np.outer(offsets, n)

    def _near_far(self, nh, rng, centre, normal, lift=None, far=True, far_along=None):
        u, v, n = _frame(normal)
        lift = rng.uniform(-0.03, 0.03) if lift is None else lift
        self._query(nh, centre + 0.02 * rng.uniform(-1, 1) * u + 0.02 * rng.uniform(-1, 1) * v + lift * n, "near")
        if far:
            d = u if far_along is None else np.asarray(far_along, F64)
            self._query(nh, centre + 1.3 * d + rng.uniform(-0.03, 0.03) * n, "far")

    def _build_filler(self):
        """Five points within 0.375 m of a site - every query beside the site is finished by the search pass (d5 < 0.16 m^2) - found by a
        hill climb on the smallest of the five residuals of esti_plane's plane: all five exceed 0.27, the plane is rejected whatever the
        last bits of the fit are, and the point's row is exactly zero."""
        site = np.array([-40.0, 48.0, -24.0])
        self._sites.add((-5, 6, -3))
        off = np.array([[0.12109375, -0.3408203125, 0.072265625], [-0.1953125, 0.2060546875, -0.240234375],
                        [-0.2880859375, 0.2353515625, -0.0439453125], [0.263671875, -0.2294921875, -0.0068359375],
                        [0.1201171875, -0.2421875, 0.251953125]])
        self.filler_pts = np.ascontiguousarray(site + off, F32)
        self.filler_world = [(site + np.array([k * 2.0 ** -9, 0.0, 0.0])).astype(F32) for k in range(-3, 4)]

    def filler_queries(self, n):
        return np.ascontiguousarray([self.filler_world[k % len(self.filler_world)] for k in range(n)], F32)

    def _check_isolation(self):
        """No query within sqrt(5) m (and a margin) of a point of another cluster."""
        owner = np.concatenate([np.full(len(self.filler_pts), -1)] + [np.full(len(c["pts"]), k) for k, c in enumerate(self.nh)])
        m64 = self.map.astype(F64)
        for q in self.queries:
            d = np.sqrt(((m64 - q["world"].astype(F64)) ** 2).sum(axis=1))
            assert not np.any((d < REACH + 0.2) & (owner != q["nh"])), (q["tag"], self.nh[q["nh"]]["family"])
        for w in self.filler_world:
            d = np.sqrt(((m64 - w.astype(F64)) ** 2).sum(axis=1))
            assert not np.any((d < REACH + 0.2) & (owner != -1))

    # ------------------------------------------------------------------ families
    def _family_a(self):
        """8 ... 60 m out, on the lattice.  0.5 ... 4 m: MiniMaps' family A0 (no two clusters that close to the origin are out of each
        other's reach)."""
        rng = np.random.default_rng(1101)
        for extent in (0.08, 0.3, 0.6):
            for noise in (0.0, 0.01, 0.05, 0.09, 0.2):
                for dist in (8, 13, 18, 24, 30, 36, 43, 50, 56, 60):
                    site = self._site(_unit(rng.normal(0, 1, 3)) * dist)
                    centre = site + rng.uniform(-0.5, 0.5, 3)
                    while True:
                        normal = rng.normal(0, 1, 3)
                        off = noise * rng.permutation([1.0, -1.0, 1.0, -1.0, 1.0]) * rng.uniform(0.7, 1.0, 5)
                        pts = self._patch(rng, centre, normal, extent, off)
                        if self._decided(pts, by=1e-9):   # (the 8 cm patches 60 m out: conditioned like family G's)
                            break
                    nh = self._add("A", pts, f"e{extent} n{noise}")
                    self._near_far(nh, rng, centre, normal)

    def _family_b(self):
        """One residual of the fitted plane at 0.1 (1 -/+ 0.01): the out-of-plane pattern is scaled until the largest residual is there."""
        rng = np.random.default_rng(1102)
        for side in (-1, 1):
            for k in range(10):
                site = self._site(_unit(rng.normal(0, 1, 3)) * rng.uniform(8, 60))
                centre = site + rng.uniform(-0.5, 0.5, 3)
                while True:
                    normal = rng.normal(0, 1, 3)
                    base = self._patch(rng, centre, normal, 0.2, np.zeros(5))
                    pattern = np.outer(np.roll([1.0, -0.8, 0.9, -0.7, 0.1], k), _unit(normal))   # (alternating around the ring: a plane cannot follow it)
                    target = PLANE_THR * (1 + 0.01 * side)
                    lo, hi = 0.0, 0.3
                    for _ in range(60):
                        mid = 0.5 * (lo + hi)
                        worst = np.max(np.abs(esti_plane((base + mid * pattern).astype(F32))["res"]))
                        lo, hi = (mid, hi) if worst < target else (lo, mid)
                    at = np.max(np.abs(esti_plane((base + lo * pattern).astype(F32))["res"]))
                    if abs(at - target) < 1e-5 and self._decided(base + lo * pattern):
                        break
                nh = self._add("B", base + lo * pattern, "inside" if side < 0 else "outside")
                self._near_far(nh, rng, centre, normal)

    def _family_c(self):
        """All five points have one coordinate exactly 0: a zero column, rank 2.  Half are close to a line (the plane through that line
        and the axis passes the gate), half are spread (rejected)."""
        rng = np.random.default_rng(1103)
        for axis in range(3):
            a, b = [c for c in range(3) if c != axis]
            for k in range(10):
                t = rng.uniform(-60, 60, 3)
                site = self._site(t, fixed={axis: 0})
                while True:
                    pts = np.zeros((5, 3))
                    pts[:, a] = site[a] + rng.uniform(-0.25, 0.25, 5)
                    pts[:, b] = site[b] + rng.uniform(-1, 1, 5) * (0.04 if k % 2 == 0 else 0.25)
                    if self._decided(pts):
                        break
                nh = self._add("C", pts, f"axis{axis} {'line' if k % 2 == 0 else 'spread'}")
                centre = site.copy()
                e_a, e_ax = np.eye(3)[a], np.eye(3)[axis]
                self._query(nh, centre + 0.02 * e_a + rng.uniform(-0.05, 0.05) * e_ax + 0.01 * np.eye(3)[b], "near")
                self._query(nh, centre + 1.3 * e_a + rng.uniform(-0.05, 0.05) * e_ax, "far")

    def _family_d(self):
        """Rank 1: five points on a coordinate axis - distinct, close together and spread out - and five EQUAL points on an axis
        (lii_map_build keeps exact duplicates).  Not here: five equal points off the axes.  Their rank is 1 only up to rounding - the
        second pivot decision rides on remainders of a few eps that any two correct implementations round differently
        (tests/test_oracle_plane_degenerate.py accepts 75 % agreement there) - so no row can be expected of them.  The all-zero matrix
        is MiniMaps' family Z."""
        rng = np.random.default_rng(1104)
        for axis in range(3):
            e = np.eye(3)[axis]
            others = {c: 0 for c in range(3) if c != axis}
            for spread, tag in ((0.05, "close"), (0.3, "spread"), (0.0, "equal")):
                for sign in (-1, 1):
                    site = self._site(e * sign * rng.uniform(8, 60), fixed=others)
                    pts = site + np.outer(rng.uniform(-spread, spread, 5) if spread else np.full(5, 0.125), e)
                    nh = self._add("D", pts, f"axis{axis} {tag}")
                    side = np.eye(3)[(axis + 1) % 3]
                    self._query(nh, site + 0.03 * e + 0.05 * side, "near")
                    self._query(nh, site + 0.04 * e + 1.3 * side, "far")

    def _family_e(self):
        rng = np.random.default_rng(1105)
        for lift in (0.05, 0.3, -0.2):
            for k in range(6):
                site = self._site(_unit(rng.normal(0, 1, 3)) * rng.uniform(8, 60))
                centre = site + rng.uniform(-0.5, 0.5, 3)
                while True:
                    normal = rng.normal(0, 1, 3)
                    pts = self._patch(rng, centre, normal, 0.4, np.r_[0, 0, 0, 0, lift])
                    if self._decided(pts):
                        break
                nh = self._add("E", pts, f"lift {lift}")
                self._near_far(nh, rng, centre, normal)

    def _family_f(self):
        """Far out along the axes and the diagonals, every orientation of the patch: all six pivot orders."""
        rng = np.random.default_rng(1106)
        dirs = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1), (-1, 1, 0), (1, -1, -1)]
        for d in dirs:
            for k in range(6):
                site = self._site(_unit(d) * rng.uniform(30, 64) + rng.uniform(-3, 3, 3))
                centre = site + rng.uniform(-0.5, 0.5, 3)
                while True:
                    normal = rng.normal(0, 1, 3)
                    pts = self._patch(rng, centre, normal, 0.3, rng.uniform(-0.01, 0.01, 5))
                    if self._decided(pts):
                        break
                nh = self._add("F", pts, f"dir {d}")
                self._near_far(nh, rng, centre, normal)

    def _family_g(self):
        """Nearly parallel columns: a patch of a few millimetres far out on a space diagonal - the down-dated column norms lose their
        digits and are computed afresh."""
        rng = np.random.default_rng(1107)
        for k in range(16):
            sg = np.array([1 if (k >> b) & 1 else -1 for b in range(3)])
            site = self._site(sg * 64.0 - sg * LATTICE * (k >> 3) * np.array([1, 0, 0]))
            centre = site + rng.uniform(-0.2, 0.2, 3)
            while True:  # (a patch this small this far out is worse conditioned by two orders of magnitude: a wider margin)
                normal = rng.normal(0, 1, 3)
                pts = self._patch(rng, centre, normal, 0.006, rng.uniform(-0.0002, 0.0002, 5))
                if self._decided(pts, by=2e-9):
                    break
            nh = self._add("G", pts, "tiny patch")
            self._near_far(nh, rng, centre, normal, lift=rng.uniform(-0.02, 0.02))

    def _family_h(self):
        """Two, three and four neighbours at the same float32 distance: offsets are multiples of 2^-4 around an integer site, the query
        sits on the site (and 2^-4 above it).  The tied points stand in the map in DESCENDING x: the list must come back ascending."""
        rng = np.random.default_rng(1108)
        s = 1.0 / 16
        kinds = {
            2: [(4, 2, 0), (-4, 2, 0), (1, -3, 0), (5, -1, 1), (-2, -5, 0)],
            3: [(4, 2, 1), (2, 1, 4), (1, 4, 2), (-3, -3, 0), (5, -2, 1)],
            4: [(4, 2, 1), (2, 1, 4), (1, 4, 2), (-4, 2, 1), (3, -5, 0)],
        }
        for ties, offs in kinds.items():
            for k in range(6):
                scale = (1, 1, 0.5)[k % 3]
                o = np.array(offs, F64) * s * scale * (0.5 if ties != 2 else 1.0)
                tied = o[:ties][np.argsort(-o[:ties, 0])]
                while True:
                    site = self._site(rng.uniform(-56, 56, 3))
                    pts = site + np.r_[tied, o[ties:]] if k % 2 == 0 else site + np.r_[o[ties:], tied]
                    if self._decided(pts):
                        break
                nh = self._add("H", pts, f"ties {ties}")
                self._query(nh, site, "near", tag="tie")
                self._query(nh, site + np.array([0, 0, s]), "near", tag="tie")
                self._query(nh, site + np.array([0, 1.25, 0]), "far", tag="tie")

    def _family_i(self):
        """The match bound: the fifth neighbour at d^2 = 5 exactly, one float above 5, and clusters of four."""
        rng = np.random.default_rng(1109)
        near4 = np.array([(0.25, 0.125, 0), (-0.1875, 0.25, 0), (0.0625, -0.3125, 0), (-0.25, -0.125, 0)])
        # (the four lie in z = 0.06 x - 0.03 y - 0.02: a tilted plane that holds (1, 2, -0.02), with the query 2 cm above it - a query IN
        # the plane has a pd2 that is rounding noise, and its float is anybody's)
        near4[:, 2] = 0.06 * near4[:, 0] - 0.03 * near4[:, 1] - 0.02
        for k in range(4):
            site = self._site(rng.uniform(-56, 56, 3))
            nh = self._add("I", site + np.r_[near4, [(1.0, 2.0, 0.0)]], "d5 = 5")
            self._query(nh, site, "far", tag="bound")
        for k in range(3):
            site = self._site(rng.uniform(-56, 56, 3), fixed={0: 0})
            x5 = F32(1.0)
            q = site.astype(F32)
            while dist2_f32(q, np.array([x5, site[1] + 2.0, site[2]], F32)) <= MAX_D2:
                x5 = np.nextafter(x5, F32(2))
            pts = site + np.r_[near4, [(0.0, 2.0, 0.0)]]
            pts[4, 0] = x5
            assert dist2_f32(q, pts[4].astype(F32)) == np.nextafter(MAX_D2, F32(6))
            nh = self._add("I", pts, "d5 = 5 + 1 ulp")
            self._query(nh, site, "far", tag="bound")
        for k in range(4):
            site = self._site(rng.uniform(-56, 56, 3))
            nh = self._add("I", site + near4, "four points")
            self._query(nh, site + np.array([0.02, 0.01, 0.03]), "other", tag="bound")
            self._query(nh, site + np.array([1.3, 0.0, 0.02]), "far", tag="bound")

    def _family_j(self):
        """The residual gate s > 0.9, i.e. |pd2| < sqrt(|p_body|) / 9: queries at that distance (1 -/+ 0.01) from an exact plane, on both
        sides of it, with |p_body| = 0.5, 5 and 60 m - built per pose, since |p_body| is the pose's.  And the body point (0, 0, 0)."""
        rng = np.random.default_rng(1110)
        for name, pose in POSES.items():
            for norm in (0.5, 5.0, 60.0):
                for _ in range(2000):
                    b0 = _unit(rng.normal(0, 1, 3)) * norm
                    c0 = pose.forward(b0.astype(F32)).astype(F64)
                    if all(np.linalg.norm(c["centre"] - c0) > (4.2 if c["family"] == "J" else 5.8) for c in self.nh) and np.linalg.norm(self.filler_pts[0] - c0) > 8:
                        break
                else:
                    raise AssertionError("no free place")
                while True:
                    normal = _unit(rng.normal(0, 1, 3))
                    pts = self._patch(rng, c0, normal, 0.3, np.zeros(5))
                    if self._decided(pts):
                        break
                nh = self._add("J", pts, f"{name} |p| {norm}")
                for side in (-1, 1):
                    for f in (0.99, 1.01):
                        t = 0.0
                        for _ in range(8):
                            body = pose.inverse(c0 + side * t * normal)
                            t = f * math.sqrt(float(np.linalg.norm(body.astype(F64)))) / 9.0
                        self._query(nh, c0 + side * t * normal, "near" if norm < 10 else "other", pose=name, body=body, tag=f"gate {f}")
                self._query(nh, c0 + 0.01 * normal, "near", tag="plain")
                if norm == 0.5:
                    self._query(nh, pose.forward(np.zeros(3, F32)), "other", pose=name, body=np.zeros(3, F32), tag="body origin")

    # ------------------------------------------------------------------ what a test runs
    def bodies(self, pose_name):
        """(ids into self.queries, body points (m, 3) float32) of the queries that exist under this pose."""
        pose = POSES[pose_name]
        ids = [k for k, q in enumerate(self.queries) if q["pose"] in (None, pose_name)]
        body = [self.queries[k]["body"] if self.queries[k]["body"] is not None else pose.inverse(self.queries[k]["world"]) for k in ids]
        return np.array(ids), np.ascontiguousarray(body, F32)

    def filler_bodies(self, pose_name, n):
        pose = POSES[pose_name]
        distinct = np.ascontiguousarray([pose.inverse(w) for w in self.filler_world], F32)
        return np.ascontiguousarray(distinct[np.arange(n) % len(distinct)])

    def reference(self, pose_name, imu_en, pose=None, cached=None):
        """point_row of every query of the pose (a search pass; or, with `pose` and `cached`, the pass on cached planes at `pose`)."""
        ids, body = self.bodies(pose_name)
        p = POSES[pose_name] if pose is None else pose
        if cached is None:
            return [point_row(p, imu_en, b, cluster=self.nh[self.queries[k]["nh"]]["pts"]) for k, b in zip(ids, body)]
        return [point_row(p, imu_en, b, cached=c) for b, c in zip(body, cached)]


class MiniMaps(Cases):
    """Neighbourhoods that cannot stand in the one map of Cases, each a map of its own (lii_map_build replaces the map):
      A0  generic patches 0.5, 1, 2 and 4 m from the origin (every extent and out-of-plane offset of family A) - the small-|d| regime, where
          the solved vector is the unit normal over d and 1 / nn is small.  They are within reach of one another, and of family J's
          clusters beside the origin, so they cannot share a map.  A normal within 0.3 of perpendicular to the line of sight is drawn
          again: the plane would pass the origin, A n = -1 has no solution there and no two solvers agree on one.
      Z   five points AT the origin: the all-zero matrix - every norm 0, every reflector with tau = 0, 0 / 0 in the back substitution, a NaN
          plane that passes esti_plane's test (fabs(NaN) > threshold is false) and a NaN s that fails the residual gate: count 5, left out."""

    def __init__(self):
        self.nh, self.queries, self._sites = [], [], set()
        self.filler_pts = np.zeros((0, 3), F32)
        rng = np.random.default_rng(1201)
        for dist in (0.5, 1.0, 2.0, 4.0):
            for extent in (0.08, 0.3, 0.6):
                for noise in (0.0, 0.01, 0.05, 0.09, 0.2):
                    while True:
                        centre = _unit(rng.normal(0, 1, 3)) * dist
                        normal = _unit(rng.normal(0, 1, 3))
                        if abs(float(normal @ _unit(centre))) < 0.3:
                            continue
                        off = noise * rng.permutation([1.0, -1.0, 1.0, -1.0, 1.0]) * rng.uniform(0.7, 1.0, 5)
                        pts = self._patch(rng, centre, normal, extent, off)
                        if self._decided(pts, by=3e-10):
                            break
                    nh = self._add("A0", pts, f"r{dist} e{extent} n{noise}")
                    self._near_far(nh, rng, centre, normal)
        nh = self._add("Z", np.zeros((5, 3)), "all zero")
        self._query(nh, [0.1, 0.2, 0.1], "near")
        self._query(nh, [1.3, 0.2, 0.1], "far")


_cases = None
_minis = None


def cases():
    global _cases
    if _cases is None:
        _cases = Cases()
    return _cases


def minimaps():
    global _minis
    if _minis is None:
        _minis = MiniMaps()
    return _minis


def scan_of(bodies):
    b = np.ascontiguousarray(bodies, F32).reshape(-1, 3)
    return np.ascontiguousarray(np.c_[b, np.zeros(len(b), F32)], F32)


def fsum_rows(rows):
    """math.fsum per entry of single-point rows (m, 91) and the bound (m - 1) 2^-53 sum|addend| a recursive sum of them stays within."""
    rows = np.asarray(rows, F64).reshape(-1, 91)
    total = np.array([math.fsum(rows[:, t]) for t in range(91)])
    bound = max(len(rows) - 1, 0) * 2.0 ** -53 * np.abs(rows).sum(axis=0)
    return total, bound


# --------------------------------------------------------------------------------------------------------------------------------- the two references, side by side
_measured = None


def _measure_set(oracle, cs, tree_of, disc):
    """Both references on every query of `cs` (Cases: one map, one tree; MiniMaps: tree_of(nh) is the tree of that neighbourhood's map)."""
    st0 = oracle.state_init()
    cfgs = {}
    for pname, imu_en in CONFIGS:
        pose = POSES[pname]
        ids, body = cs.bodies(pname)
        pod = pose.pod(st0)
        pod2 = oracle.state_boxplus(pod, MOVE)
        ref = cs.reference(pname, imu_en)
        ref2 = cs.reference(pname, imu_en, pose=Pose.from_pod(pname + " moved", pod2), cached=ref)
        orc, orc2 = [], []
        F, U = np.zeros(len(ids), bool), np.zeros(len(ids), bool)
        for at, (k, b, r) in enumerate(zip(ids, body, ref)):
            tree = tree_of(cs.queries[k]["nh"])
            o = tree.iterate_once(scan_of(b), pod, search=True, imu_en=imu_en)
            orc.append(dict(count=int(o["nearest_n"][0]), nb=o["nearest"][0].copy(), selected=bool(o["selected"][0]), out=o["out91"].copy(),
                            pabcd=o["pabcd"][0].copy()))
            o2 = tree.iterate_once(scan_of(b), pod2, search=False, imu_en=imu_en, selected=o["selected"])
            orc2.append(dict(selected=bool(o2["selected"][0]), out=o2["out91"].copy()))
            _, d6, c6 = tree.knn(r["world"][None, :], k=6)
            c5, d5, d6 = min(int(c6[0]), 5), d6[0, 4], (d6[0, 5] if c6[0] == 6 else np.inf)
            F[at] = c5 == 5 and d5 < F32(0.16) and d5 < d6
            U[at] = c5 < 5 or d5 > F32(0.81)
        fam = np.array([cs.nh[cs.queries[k]["nh"]]["family"] for k in ids])
        cfgs[(pname, imu_en)] = dict(ids=ids, body=body, pod=pod, pod2=pod2, ref=ref, ref2=ref2, orc=orc, orc2=orc2, F=F, U=U, fam=fam)
        for r, o, f in zip(ref, orc, fam):
            if r["plane"] is None:
                continue
            pn, po = r["plane"]["pabcd"], o["pabcd"]
            if not (np.all(np.isfinite(pn)) and np.all(np.isfinite(po))):
                continue
            scale = max(1.0, abs(pn[3]))
            w = r["world"].astype(F64)
            pd = abs((po[0] * w[0] + po[1] * w[1] + po[2] * w[2] + po[3]) - (pn[0] * w[0] + pn[1] * w[1] + pn[2] * w[2] + pn[3]))
            disc["normal"][f] = max(disc["normal"].get(f, 0.0), float(np.abs(po[:3] - pn[:3]).max()))
            disc["d"][f] = max(disc["d"].get(f, 0.0), abs(po[3] - pn[3]) / scale)
            disc["pd2"][f] = max(disc["pd2"].get(f, 0.0), pd / scale)
    return cfgs


def measure(oracle):
    """Both CPU references on the one-point scans of every query, every CONFIGS entry, search pass and cached-plane pass at the moved
    pose; the F / U classes on the CPU tree; the worst discrepancies.  Computed once per process.  Returns dict(
      cfg[(pose, imu_en)] = dict(ids, body, pod, pod2, ref, ref2 (point_row dicts), orc, orc2 (dicts: count, nb, selected, out, pabcd),
                                 F, U (bool arrays), fam (family of each query)) for cases(), mini[...] the same for minimaps(),
      disc = dict(hh, hz, normal{family}, d{family}, pd2{family}), excluded{family: (left out, of)}, tree)."""
    global _measured
    if _measured is not None:
        return _measured
    cs, mm = cases(), minimaps()
    tree = oracle.Tree("oracle")
    tree.build(cs.map)
    mini_trees = {}

    def mini_tree(nh):
        if nh not in mini_trees:
            mini_trees[nh] = oracle.Tree("oracle")
            mini_trees[nh].build(mm.nh[nh]["pts"])
        return mini_trees[nh]

    disc = dict(hh=0.0, hz=0.0, normal={}, d={}, pd2={})
    cfgs = _measure_set(oracle, cs, lambda nh: tree, disc)
    mini = _measure_set(oracle, mm, mini_tree, disc)
    # rows: where both references selected the point and no exclusion applies (with the figures just measured)
    excl = {}
    for c in list(cfgs.values()) + list(mini.values()):
        for passes in ((c["ref"], c["orc"]), (c["ref2"], c["orc2"])):
            for r, o, f in zip(*passes, c["fam"]):
                ex = excluded(r, f, disc)
                n_ex, n_all = excl.get(f, (0, 0))
                excl[f] = (n_ex + int(ex), n_all + 1)
                if ex or not (r["selected"] and o["selected"]):
                    continue
                a, b = group_ratios(o["out"], r, 1.0, 1.0, f, disc)
                disc["hh"], disc["hz"] = max(disc["hh"], a), max(disc["hz"], b)
    _measured = dict(cfg=cfgs, mini=mini, disc=disc, excluded=excl, tree=tree)
    return _measured

"""What the local-map tests share (test_gpu_local_map.py): the 40 m / 10 m cube, a platform that travels at constant velocity through a
hall (so that lasermap_fov_segment has something to do within a dozen scans), its scans and IMU samples, and the comparison helpers.
Scans are ~4 000 points: 32 rings x 128 columns of harness/synth.py's spinning sensor."""
import numpy as np

from harness import synth

CUBE_LEN, DET_RANGE = 40.0, 10.0
RINGS, COLS = 32, 128


def as_set(a):
    return np.unique(np.ascontiguousarray(a, np.float32).reshape(-1, 3), axis=0)


def _sweep(sweep_s):
    return synth.spinning_lidar(RINGS, COLS, -25.0, 25.0, sweep_ms=1000.0 * sweep_s)


def static_scan(hall, R_wb, p_wb, seed, max_range=100.0, noise=0.02):
    """synth.make_scan with this file's sensor: one undistorted sweep from (R_wb, p_wb), ascending time order."""
    rng = np.random.default_rng(seed)
    dirs_b, t_ms = _sweep(0.1)
    r = hall.raycast(p_wb, dirs_b @ np.asarray(R_wb).T) + rng.normal(0, noise, len(dirs_b))
    ok = np.isfinite(r) & (r > 0.5) & (r < max_range)
    s = np.concatenate([dirs_b[ok] * r[ok, None], t_ms[ok, None]], 1).astype(np.float32)
    return np.ascontiguousarray(s[np.argsort(s[:, 3], kind="stable")])


class Traveller(synth.Trajectory):
    """Constant velocity `v` from the origin at t = T0, a slow yaw: enough motion to cross the cube's thresholds, none that a
    constant-velocity or an IMU propagation over one scan period would miss by more than centimetres."""
    T0 = 10.0

    def __init__(self, v=(1.3, 0.65, 0.0), yaw_rate=0.01):
        super().__init__()
        self.v, self.yaw_rate = np.asarray(v, float), yaw_rate

    def euler(self, t):
        t = np.asarray(t, float)
        return [np.zeros_like(t), np.zeros_like(t), self.yaw_rate * (t - self.T0)]

    def p(self, t):
        t = np.asarray(t, float)
        return (t - self.T0)[..., None] * self.v


class Stream:
    """Scan k begins at T0 + k * PERIOD and sweeps SWEEP seconds; the state handed to the first call is the pose one period before the
    end of scan 0.  With v = (1.3, 0.65, 0) and the cube initialised at the end of scan 0 the cube moves along x at scans 4 and 12 and along
    x AND y at scan 8 (the tests assert that from lii_local_map_get, not from here)."""
    PERIOD, SWEEP, IMU_HZ = 1.0, 0.1, 50.0

    def __init__(self, n_scans=14):
        import lidar_imu_init_amd as lii
        self.hall = synth.Hall(size=(70.0, 40.0, 8.0), n_boxes=10, seed=7)
        self.map_pts = self.hall.surface_points(0.25, noise=0.01, seed=7)
        self.traj = Traveller()
        self.n_scans = n_scans
        T0 = self.traj.T0
        self.scans = [self._scan(k) for k in range(n_scans)]
        t_first = T0 + self.SWEEP - self.PERIOD
        self.imu = synth.simulate_imu(self.traj, t_first - 0.1, T0 + n_scans * self.PERIOD, self.IMU_HZ, np.eye(3), np.zeros(3), np.zeros(3), np.zeros(3), 0.0,
                                      noise_g=1e-4, noise_a=1e-3)
        st = lii.State()
        st.rot_end[:] = self.traj.R(np.array([t_first]))[0]
        st.pos_end[:] = self.traj.p(np.array([t_first]))[0]
        st.vel_end[:] = self.traj.v
        st.gravity[:] = [0.0, 0.0, -9.81]
        st.cov[:] = np.diag(np.r_[np.full(6, 1e-4), np.full(6, 1e-6), np.full(3, 1e-2), np.full(9, 1e-5)])
        self.state0 = st
        t, g, a = self.imu
        k0 = int(np.searchsorted(t, t_first, side="right"))
        self.k_imu0 = k0
        self.carry0 = dict(last_imu=np.r_[t[k0 - 1], g[k0 - 1], a[k0 - 1]], acc_s_last=np.array([0.0, 0.0, 9.81]), angvel_last=np.zeros(3), last_lidar_end_time=t_first)

    def _scan(self, k):
        """synth.make_distorted_scan with this file's sensor: ray j is cast from the pose the platform has at its own instant"""
        rng = np.random.default_rng(900 + k)
        dirs_b, t_ms = _sweep(self.SWEEP)
        tj = self.traj.T0 + k * self.PERIOD + t_ms.astype(np.float64) / 1000.0
        dirs_w = np.einsum("nij,nj->ni", self.traj.R(tj), dirs_b)
        r = self.hall.raycast(self.traj.p(tj), dirs_w) + rng.normal(0, 0.01, len(dirs_b))
        ok = np.isfinite(r) & (r > 0.5) & (r < 100.0)
        s = np.concatenate([dirs_b[ok] * r[ok, None], t_ms[ok, None]], 1).astype(np.float32)
        return np.ascontiguousarray(s[np.argsort(s[:, 3], kind="stable")])

    def t_beg(self, k):
        return self.traj.T0 + k * self.PERIOD

    def t_end(self, k):
        return self.t_beg(k) + float(self.scans[k][-1, 3]) / 1000.0

    def imu_rows(self, k):
        """the samples of scan k: stamps in (end of scan k - 1, end of scan k]"""
        t, g, a = self.imu
        lo = self.k_imu0 if k == 0 else int(np.searchsorted(t, self.t_end(k - 1), side="right"))
        hi = int(np.searchsorted(t, self.t_end(k), side="right"))
        return np.c_[t[lo:hi], g[lo:hi], a[lo:hi]]

    def lo_rates(self, st):
        """what the LO loop does between two scans (src/laserMapping.cpp:1137-1143): the rates of the motion, here the trajectory's own"""
        st.vel_end[:] = self.traj.v
        st.bias_g[:] = [0.0, 0.0, self.traj.yaw_rate]

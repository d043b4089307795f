"""The scan, the poses and the numpy restatement that tests/test_gpu_pose_score.py (device), tests/test_gpu_relocalize.py (device) and
tests/test_pose_grid_host.py (CPU) share.  No GPU is touched here.

The world is the suite's hall map (conftest.small_world) and the `tiny` scan of tests/test_gpu_register.py: true pose
rot_zyx(0.03, -0.02, 0.4), (0.8, -0.6, 0.1).
"""
import numpy as np

from conftest import make_state
from harness import synth
from lidar_imu_init_amd import pose_grid

TRUE_R = synth.rot_zyx(0.03, -0.02, 0.4)
TRUE_P = np.array([0.8, -0.6, 0.1])
# the far-off initial guess of the re-localisation case: truth + (3.3, -2.2, 0) m, yaw + 0.73 rad, roll / pitch 0
GUESS_R = synth.rot_zyx(0.0, 0.0, 0.4 + 0.73)
GUESS_P = TRUE_P + np.array([3.3, -2.2, 0.0])
# the non-trivial extrinsic of test_iterate_matches_oracle
R_LI = synth.rot_zyx(0.01, 0.02, -0.015)
T_LI = np.array([0.03, -0.02, 0.05])


def tiny_scan(small_world):
    hall, _ = small_world
    return synth.make_scan(hall, "tiny", TRUE_R, TRUE_P, noise=0.02, seed=3)


def perturbed(with_extrinsic):
    """The perturbed start pose of test_iterate_matches_oracle: the LiDAR pose is (R, p) + a small error either way."""
    rli, tli = (R_LI, T_LI) if with_extrinsic else (np.eye(3), np.zeros(3))
    Rw = TRUE_R @ synth.rot_zyx(0.004, -0.003, 0.005) @ rli.T
    pw = TRUE_P + np.array([0.03, -0.02, 0.01]) - Rw @ tli
    return Rw, pw


def parity_poses(small_world):
    """The 24 poses of the oracle parity test as two batches, one per base state: [(R_LI, T_LI, R (K, 3, 3), p (K, 3)), ...].
    Batch 0 (identity extrinsic, 23 poses): the true pose; the perturbed pose; the far-off guess; a pose 0.4 m off the +x wall that
    looks out of the hall (many lists short, many queries past the map's edge); 19 nodes of the 0.5 m / 10 degree grid around the
    perturbed pose (the 27 nodes less the centre, the first 19 in grid order).  Batch 1: the perturbed pose with its extrinsic in base."""
    hall, _ = small_world
    Rp, pp = perturbed(False)
    gR, gp = pose_grid(Rp, pp, 0.5, 0.5, -np.deg2rad(10.0), np.deg2rad(15.0), np.deg2rad(10.0))
    assert len(gR) == 27
    keep = [i for i in range(27) if i != 13][:19]  # (node 13: offset (0, 0), yaw 0 - the centre itself)
    wall_p = np.array([hall.hi[0] - 0.4, 0.5, 0.1])
    R0 = np.concatenate([np.stack([TRUE_R, Rp, GUESS_R, np.eye(3)]), gR[keep]])
    p0 = np.concatenate([np.stack([TRUE_P, pp, GUESS_P, wall_p]), gp[keep]])
    Rl, pl = perturbed(True)
    return [(np.eye(3), np.zeros(3), R0, p0), (R_LI, T_LI, Rl[None], pl[None])]


def state_at(oracle, R, p, r_li=None, t_li=None):
    return make_state(oracle, R, p, r_li, t_li)


def total_residual_np(ref):
    """total_residual of a search pass restated from the oracle's per-point outputs: the float |pd2| of every selected point (normvec's
    fourth component, src/laserMapping.cpp:1007-1008), added in double in index order."""
    sel = ref["selected"].astype(bool)
    r = np.abs(ref["normvec"][sel, 3]).astype(np.float64)
    tot = 0.0
    for v in r:
        tot += float(v)
    return int(sel.sum()), tot


def res_row_np(ref):
    """res_last of that pass: |pd2| (float) where selected, -1000 elsewhere (:987)."""
    sel = ref["selected"].astype(bool)
    return np.where(sel, np.abs(ref["normvec"][:, 3]), np.float32(-1000.0)).astype(np.float32)

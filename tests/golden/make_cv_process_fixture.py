"""Records what the UNMODIFIED reference header computes for one LO-mode scan - ImuProcess::Process with imu_en == false,
src/IMU_Processing.hpp:212-266: constant-velocity propagation + de-skew, compiled as oracle/_ref/libref_imu.so by `make -C oracle ref` -
into tests/golden/imu/reference_cv_process.npz: the inputs of the cases of tests/test_gpu_scan_register_cv.py and
tests/test_gpu_map_build_from_scan.py and the recorded outputs of oracle.ref_imu_process_cv (propagated state, de-skewed cloud).

  A  4 097 points (16 x 256 + 1: the last scan workgroup of the de-skew launch holds one point, the propagating workgroup is block 17),
     bias_g and vel_end non-zero, dt = 0.05 (as the header forms it: a difference of absolute stamps)
  B  the first 4 096 points of A (full blocks only), bias_g = 0, vel_end = 0, first frame: dt = 0.1, Exp's small-angle branch
  C  A's points in a fixed random permutation (the time-extent form); the header sorts by stamp, so its output is A's

The scan is synth.make_distorted_scan(Hall(size=(24, 18, 6), n_boxes=8, seed=7), "mid16k", Trajectory(), ...) reduced to distinct
ascending stamps (make_scan below says how: the sensor model stamps a whole column alike) and thinned to exactly 4 097 points; before the file is written the CPU chain - oracle.voxel_grid(header cloud, 0.1),
Tree("oracle").iekf_update against hall.surface_points(0.15, noise=0.01, seed=7) - must converge with effect_num > 100 for A and B
(it does at 4 097: no need to thin less).  The input points are STORED: the tests never regenerate them.

Run once where the reference library is built.  DATA only: numbers the reference program reads and writes, no program text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "imu", "reference_cv_process.npz")
N_A = 16 * 256 + 1
T_BEG, SWEEP = 2.5, 0.05
COV_GYR_SCALE, COV_ACC_SCALE = np.array([50.0, 40.0, 60.0]), np.array([2.0, 3.0, 1.5])  # distinct per axis: a swapped index shows
LEAF, MAX_IT = 0.1, 5


def hall():
    from harness import synth
    return synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)


def lo_state(t, moving):
    """The LO-phase state at time t on the synthetic trajectory: LiDAR pose, identity extrinsic; moving: vel_end = the velocity, bias_g =
    the body angular velocity (what the LO filter estimates in those slots), else both zero."""
    import lidar_imu_init_amd as lii
    from harness import synth
    from oracle import oracle as O
    traj = synth.Trajectory()
    R = lambda s: traj.R(np.array([s]))[0]
    p = lambda s: traj.p(np.array([s]))[0]
    st = lii.State()
    st.rot_end[:] = R(t)
    st.pos_end[:] = p(t)
    if moving:
        h = 1e-3
        st.vel_end[:] = (p(t + h) - p(t - h)) / (2 * h)
        st.bias_g[:] = O.log_so3(R(t - h).T @ R(t + h)) / (2 * h)
    st.cov[:] = np.diag(np.r_[np.full(6, 1e-4), np.full(6, 1e-6), np.full(3, 1e-2), np.full(3, 1e-3), np.full(6, 1e-5)])
    return st


def make_scan(k=0):
    """Sub-frame k of the stream (k = 0: the scan of the cases; tests/test_gpu_scan_register_cv.py takes the next ones for its run of
    consecutive scans)."""
    from harness import synth
    s = synth.make_distorted_scan(hall(), "mid16k", synth.Trajectory(), T_BEG + k * SWEEP, SWEEP, noise=0.01, seed=5000 + k)
    # "mid16k" fires its 32 rings together: 512 distinct stamps, fewer than the case needs.  The points of a column are kept and their
    # stamps staggered inside the column's slot (ring j: + j / 32 of the column period, as a sensor that fires its rings in turn stamps
    # them; 3 us apart, a platform at 1 m/s moves 3 um): ascending, distinct stamps, so that the header's std::sort leaves the order alone.
    s = s[np.argsort(s[:, 3], kind="stable")]
    t, start, count = np.unique(s[:, 3], return_index=True, return_counts=True)
    slot = float(np.diff(t.astype(np.float64)).min())
    rank = np.arange(len(s)) - np.repeat(start, count)
    assert rank.max() < 32
    s[:, 3] = (s[:, 3].astype(np.float64) + rank * slot / 32.0).astype(np.float32)
    assert np.all(np.diff(s[:, 3]) > 0)
    keep = np.unique(np.round(np.linspace(0, len(s) - 1, N_A)).astype(np.int64))
    assert len(keep) == N_A, (len(s), len(keep))
    return np.ascontiguousarray(s[keep])


def run_header(c):
    """(propagated state, de-skewed cloud in the header's time-sorted order) of one case dict."""
    from oracle import oracle as O
    first = bool(c["first_frame"])
    return O.ref_imu_process_cv(100.0 + float(c["dt"]), 100.0, first, c["cov_gyr_scale"], c["cov_acc_scale"], c["state"], c["pts"])


def cpu_chain(state, cloud):
    from oracle import oracle as O
    tree = O.Tree("oracle")
    tree.build(hall().surface_points(0.15, noise=0.01, seed=7))
    body, _ = O.voxel_grid(cloud, LEAF)
    r = tree.iekf_update(body, state, state, max_iterations=MAX_IT, imu_en=False)
    tree.close()
    return r


def cases():
    pts = make_scan()
    perm = np.random.default_rng(11).permutation(N_A)
    base = dict(cov_gyr_scale=COV_GYR_SCALE, cov_acc_scale=COV_ACC_SCALE)
    return {
        "A": dict(base, pts=pts, state=lo_state(T_BEG, True).pod.copy(), dt=0.05, first_frame=0),
        "B": dict(base, pts=np.ascontiguousarray(pts[:N_A - 1]), state=lo_state(T_BEG + SWEEP, False).pod.copy(), dt=0.1, first_frame=1),
        "C": dict(base, pts=np.ascontiguousarray(pts[perm]), state=lo_state(T_BEG, True).pod.copy(), dt=0.05, first_frame=0),
    }


def main():
    from oracle import oracle as O
    assert O.ref_imu_lib() is not None, "build oracle/_ref/libref_imu.so first (make -C oracle ref)"
    out = {}
    cs = cases()
    for name, c in cs.items():
        st, cloud = run_header(c)
        if name in ("A", "B"):
            r = cpu_chain(st, cloud)
            effect = int(r["selected"].sum())  # effect_feat_num of the last pass
            moved = float(np.linalg.norm(r["state"][9:12] - st[9:12]))
            print(f"case {name}: {len(c['pts'])} points, CPU chain: iterations {r['iters']} of at most {MAX_IT}, effect_num {effect}, moved {moved:.4f} m")
            assert effect > 100 and r["iters"] < MAX_IT, (effect, r["iters"])  # (stops before the last pass: converged and re-matched)
        for k, v in c.items():
            if name == "C" and k == "pts":
                continue  # (A's points through `perm`)
            out[f"{name}/in/{k}"] = np.asarray(v)
        out[f"{name}/out/state"] = st
        if name == "C":
            assert np.array_equal(cloud, out["A/out/points"])  # the header sorts by stamp: the same cloud as A's
        else:
            out[f"{name}/out/points"] = cloud
    out["C/in/perm"] = np.random.default_rng(11).permutation(N_A).astype(np.int32)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def load(name):
    """The case as the tests use it: inputs + the header's outputs, from the file."""
    F = np.load(OUT)
    src = name
    c = {k: F[f"{src}/in/{k}"] for k in ("state", "dt", "first_frame", "cov_gyr_scale", "cov_acc_scale")}
    if name == "C":
        c["perm"] = F["C/in/perm"]
        c["pts"] = np.ascontiguousarray(F["A/in/pts"][c["perm"]])
        c["out_points"] = F["A/out/points"]
    else:
        c["pts"] = F[f"{name}/in/pts"]
        c["out_points"] = F[f"{name}/out/points"]
    c["out_state"] = F[f"{name}/out/state"]
    c["dt"] = float(c["dt"])
    return c


if __name__ == "__main__":
    main()

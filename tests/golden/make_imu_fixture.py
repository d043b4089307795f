"""Records what the UNMODIFIED reference header computes for the IMU forward propagation
(ImuProcess::Process, src/IMU_Processing.hpp:419-461, compiled as oracle/_ref/libref_imu.so by `make -C oracle ref`)
into tests/golden/imu/reference_propagation.npz: the inputs of every case of tests/test_gpu_imu_propagate.py and the
recorded outputs of ref_imu_process_lio / ref_imu_process_cv (states, IMUpose tables, carries).

Run once where the reference library is built; a GPU box without it still has the header's answers.  DATA only: numbers the
reference program reads and writes, no program text.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "imu", "reference_propagation.npz")
MEAN_ACC_NORM = 9.805


def random_state(rng, lio, pos_scale=2.0):
    """tests/test_replay_host.py:_random_state (same draws in the same order)."""
    import lidar_imu_init_amd as lii
    from harness import synth
    st = lii.State()
    st.rot_end[:] = synth.rot_zyx(*rng.normal(0, 0.5, 3))
    st.pos_end[:] = rng.normal(0, pos_scale, 3)
    st.vel_end[:] = rng.normal(0, 0.5, 3)
    st.bias_g[:] = rng.normal(0, 0.4 if not lio else 0.003, 3)
    if lio:
        st.bias_a[:] = rng.normal(0, 0.01, 3)
        st.offset_R_L_I[:] = synth.rot_zyx(*rng.normal(0, 0.3, 3))
        st.offset_T_L_I[:] = rng.normal(0, 0.1, 3)
        st.gravity[:] = [0.1, -0.2, -9.8]
    A = rng.normal(0, 1e-2, (24, 24))
    st.cov[:] = A @ A.T + np.eye(24) * 1e-4
    return st


def lio_cases():
    """name -> inputs.  The first three are the cases of tests/test_replay_host.py:80-89 (same generator, same seed)."""
    rng = np.random.default_rng(6)
    cases = {}
    specs = [("n20_end_after", 20, True, 0, 2.0), ("n11_end_before", 11, False, 0, 2.0), ("n2_end_after", 2, True, 0, 2.0),
             ("skip3", 14, True, 3, 2.0), ("n63", 63, False, 0, 2.0), ("far100", 20, True, 0, 100.0), ("noise_axes", 20, True, 0, 2.0)]
    for name, n_imu, end_after, skip, pos_scale in specs:
        st = random_state(rng, lio=True, pos_scale=pos_scale)
        t0 = 50.0
        last_imu = np.r_[t0 - 0.002, rng.normal(0, 0.3, 3), rng.normal(0, 0.5, 3) + [0, 0, 9.8]]
        t = t0 + 0.003 + 0.005 * np.arange(n_imu)
        imu = np.c_[t, rng.normal(0, 0.3, (n_imu, 3)), rng.normal(0, 0.5, (n_imu, 3)) + [0, 0, 9.8]]
        # the previous scan ended between two IMU samples; skip > 0: behind the first `skip` samples of THIS scan (the `continue`
        # of :307 for them, the first form of dt, :325-326, for the step that straddles the end)
        last_end = t0 + 0.0003 if skip == 0 else t[skip - 1] + 0.002
        beg = last_end
        end = t[-1] + (0.002 if end_after else -0.001)
        pts = np.c_[rng.uniform(-5, 5, (3, 3)), [0.0, 1e3 * (end - beg) / 2, 1e3 * (end - beg)]].astype(np.float32)
        cases[name] = dict(state=st.pod.copy(), imu=imu, last_imu=last_imu, last_end=last_end, acc_s_last=rng.normal(0, 0.2, 3),
                           angvel_last=rng.normal(0, 0.2, 3), beg=beg, pts=pts, cov_gyr=np.full(3, 0.1), cov_acc=np.full(3, 0.1))
    # the two noise vectors the reference wrapper takes, distinct from each other and from axis to axis (a swapped index, or R diag(cov_acc)
    # used transposed, would pass with equal values)
    cases["noise_axes"].update(cov_gyr=np.array([0.1, 0.2, 0.3]), cov_acc=np.array([0.4, 0.5, 0.6]))
    return cases


def cv_cases():
    """tests/test_replay_host.py:55-70."""
    rng = np.random.default_rng(5)
    cases = {}
    for dt in (0.05, 0.1, 0.013):
        st = random_state(rng, lio=False)
        pts = np.c_[rng.uniform(-5, 5, (4, 3)), [0.0, 10.0, 20.0, 30.0]].astype(np.float32)
        cases[f"dt{dt}"] = dict(state=st.pod.copy(), dt=dt, pts=pts, cov_gyr_scale=np.full(3, 50.0), cov_acc_scale=np.full(3, 2.0))
    return cases


def run_reference_lio(c):
    from oracle import oracle as O
    return O.ref_imu_process_lio(c["imu"], c["last_imu"], c["last_end"], c["acc_s_last"], c["angvel_last"], c["cov_gyr"], c["cov_acc"],
                                 MEAN_ACC_NORM, c["beg"], c["state"], c["pts"])


def run_reference_cv(c):
    from oracle import oracle as O
    return O.ref_imu_process_cv(100.0 + c["dt"], 100.0, False, c["cov_gyr_scale"], c["cov_acc_scale"], c["state"], c["pts"])[0]


def main():
    from oracle import oracle as O
    assert O.ref_imu_lib() is not None, "build oracle/_ref/libref_imu.so first (make -C oracle ref)"
    out = {}
    for name, c in lio_cases().items():
        ref = run_reference_lio(c)
        for k, v in c.items():
            out[f"lio/{name}/in/{k}"] = np.asarray(v)
        out[f"lio/{name}/out/state"] = ref["state"]
        out[f"lio/{name}/out/poses"] = ref["poses"]
        out[f"lio/{name}/out/carry"] = np.r_[ref["acc_s_last"], ref["angvel_last"], ref["last_lidar_end_time"]]
    for name, c in cv_cases().items():
        for k, v in c.items():
            out[f"cv/{name}/in/{k}"] = np.asarray(v)
        out[f"cv/{name}/out/state"] = run_reference_cv(c)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()

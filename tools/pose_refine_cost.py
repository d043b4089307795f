#!/usr/bin/env python3
"""What lii_pose_refine costs against the loop it replaces, on one MI355X.

  python tools/pose_refine_cost.py [--reps 5] [--out profiles/pose_refine.md]

One process, one GPU run, the suite's hall map (68 k points) and the `tiny` scan of the tests (2 048 points) at the schedule
(max_iterations, updates) = (4, 2).  The K poses are the K best-ranked nodes (lii_pose_score, rank_poses) of the 0.5 m / 10 degree grid
around the far-off guess of tests/test_gpu_relocalize.py - what Registrar.relocalize(top = K) refines.  For K in {1, 3, 4, 6, 8, 16, 64, 256}:
  * lii_pose_refine, host arrays in and out: wall clock, `reps` times after two warm-up calls (mean, min, max);
  * lii_pose_refine_dev, poses / records on the device: HIP events on the handle's stream around one enqueued call, `reps` times;
  * the serial inner loop of Registrar.relocalize for the same K poses on the same handle - K x updates lii_iekf_update calls, each the
    whole per-scan chain and a host wait: wall clock, `reps` times; and whether both select the same winner.
Launches and scratch are the call's own arithmetic (lii_refine.hip, lii_context.h), not measurements."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.map_nearest_cost import Events  # noqa: E402

KS = (1, 3, 4, 6, 8, 16, 64, 256)
MAX_IT, UPDATES, N = 4, 2, 2048


def scratch_bytes(K, n):
    """planes (32) + flag (1) per pair, 232 per workgroup of 64 pairs of one pose, 512 per pose (lii_context::PoseRefine)"""
    return 33 * K * n + 232 * K * ((n + 63) // 64) + 512 * K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_refine.md"))
    a = ap.parse_args()
    import numpy as np
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd.api import POSE_REFINED_DTYPE, poses_array
    from harness import synth

    hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)
    map_pts = hall.surface_points(0.15, noise=0.01, seed=7)
    R_true, p_true = synth.rot_zyx(0.03, -0.02, 0.4), np.array([0.8, -0.6, 0.1])
    cloud = np.ascontiguousarray(synth.make_scan(hall, "tiny", R_true, p_true, noise=0.02, seed=3), np.float32)
    gR, gp = lii.pose_grid(synth.rot_zyx(0.0, 0.0, 0.4 + 0.73), p_true + [3.3, -2.2, 0.0], 4.0, 0.5, 0.0, 2 * np.pi, np.deg2rad(10.0))
    inside = np.all((gp[:, :2] > hall.lo[:2] + 0.3) & (gp[:, :2] < hall.hi[:2] - 0.3), axis=1)
    grid = poses_array((gR[inside], gp[inside]))
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    reg.scan_upload(cloud)
    assert reg.downsample_skip() == N
    base = lii.State()
    _, effect, total = reg.pose_score(base, grid)
    P_all = np.ascontiguousarray(grid[lii.rank_poses(effect, total)[:max(KS)]])
    ev = Events(reg)
    d_P, d_out = reg.dev_alloc(P_all.nbytes), reg.dev_alloc(max(KS) * POSE_REFINED_DTYPE.itemsize)
    rows = []
    for K in KS:
        P = np.ascontiguousarray(P_all[:K])
        reg.dev_upload(d_P, P)
        for _ in range(2):
            rec = reg.pose_refine(base, P, MAX_IT, UPDATES)
            reg.pose_refine_dev(base, d_P, K, d_out, MAX_IT, UPDATES)
        reg.synchronize()
        host_ms, dev_ms, loop_ms = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rec = reg.pose_refine(base, P, MAX_IT, UPDATES)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        for _ in range(a.reps):
            ev.start()
            reg.pose_refine_dev(base, d_P, K, d_out, MAX_IT, UPDATES)
            dev_ms.append(ev.stop_ms())
        effs = None
        for rep in range(a.reps + 1):  # (the first one warms up)
            t0 = time.perf_counter()
            effs = []
            for k in range(K):  # (the inner loop of Registrar.relocalize)
                st = base.copy()
                st.rot_end[:] = P[k, :9].reshape(3, 3)
                st.pos_end[:] = P[k, 9:]
                eff = 0
                for _ in range(UPDATES):
                    eff = reg.iekf_update(st, st.copy(), max_iterations=MAX_IT, imu_en=False)["effect_num"]
                effs.append(eff)
            if rep:
                loop_ms.append((time.perf_counter() - t0) * 1e3)
        rows.append(dict(K=K, host=host_ms, dev=dev_ms, loop=loop_ms, iters=float(rec["iterations"].mean()), searches=float(rec["searches"].mean()),
                         same_winner=bool(int(np.argmax(effs)) == int(np.argmax(rec["effect_num"]))),
                         same_effect=bool(np.array_equal(np.asarray(effs), rec["effect_num"]))))
        print({k: (v if not isinstance(v, list) else [round(x, 3) for x in v]) for k, v in rows[-1].items()}, flush=True)
    reg.close()

    def mmm(v):
        return f"{np.mean(v):.3f} ({np.min(v):.3f} .. {np.max(v):.3f})"

    lines = ["# What lii_pose_refine costs (one MI355X)", "",
             f"`python tools/pose_refine_cost.py --reps {a.reps}`: the hall map of the tests ({len(map_pts)} points, cell 0.30 m), the `tiny` scan ({N} points), the "
             f"schedule (max_iterations, updates) = ({MAX_IT}, {UPDATES}), the K best-ranked nodes of the 0.5 m / 10 degree re-localisation grid.  One run; every "
             f"figure is the mean of {a.reps} repetitions with (min .. max) behind it.", "",
             "lii_pose_refine (host arrays) and the serial loop - the inner loop of Registrar.relocalize: K x updates lii_iekf_update calls on the same handle - by the "
             "wall clock; lii_pose_refine_dev by HIP events on the handle's stream around one enqueued call.", "",
             "| K | lii_pose_refine, host [ms] | lii_pose_refine_dev [ms] | serial loop [ms] | serial / host call | launches per call | scratch [bytes] | iterations, searches per pose (mean) | same winner | same effect_num |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['K']} | {mmm(r['host'])} | {mmm(r['dev'])} | {mmm(r['loop'])} | {np.mean(r['loop']) / np.mean(r['host']):.2f}x (worst case "
                     f"{np.min(r['loop']) / np.max(r['host']):.2f}x) | {2 * MAX_IT * UPDATES} (+ 2 copies in the host form) | {scratch_bytes(r['K'], N)} | "
                     f"{r['iters']:.2f}, {r['searches']:.2f} | {r['same_winner']} | {r['same_effect']} |")
    lines += ["", f"The serial loop is K x {UPDATES} registrations of about 12 launches and one host wait each; the call is {2 * MAX_IT * UPDATES} launches and one wait, "
              "whatever K is.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

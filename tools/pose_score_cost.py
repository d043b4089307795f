#!/usr/bin/env python3
"""What lii_pose_score costs against the loop it replaces, on one MI355X.

  python tools/pose_score_cost.py [--reps 5] [--out profiles/pose_score.md]

One process, one GPU run, the suite's hall map (68 k points).  For (n_down, K) in {2 048, 20 000} x {16, 256} - the cloud is the `tiny`
scan of the tests, for 20 000 points ten of them from the same pose with different noise - and K nodes of the 0.5 m / 10 degree grid
around the far-off guess of tests/test_gpu_relocalize.py:
  * lii_pose_score_dev, poses / scores / res on the device: HIP events on the handle's stream around one enqueued call, `reps` times
    after two warm-up calls (mean, min, max);
  * lii_pose_score, host arrays in and out, without res: wall clock, `reps` times;
  * the loop: K calls of lii_iekf_iterate(search = 1) on the same handle, wall clock around the K calls, `reps` times - and the k-NN
    launch of such a call alone (lii_last_timings [7]): the specialised search launch per query against the wavefront per query here.
Algorithmic bytes per (pose, point) pair: the body point (16), five neighbours (80), res (4)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.map_nearest_cost import Events  # noqa: E402

SIZES, KS = (2048, 20_000), (16, 256)
PAIR_BYTES = 16 + 80 + 4
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_score.md"))
    a = ap.parse_args()
    import numpy as np
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd.api import poses_array
    from harness import synth

    hall = synth.Hall(size=(24.0, 18.0, 6.0), n_boxes=8, seed=7)
    map_pts = hall.surface_points(0.15, noise=0.01, seed=7)
    R_true, p_true = synth.rot_zyx(0.03, -0.02, 0.4), np.array([0.8, -0.6, 0.1])
    clouds = {2048: synth.make_scan(hall, "tiny", R_true, p_true, noise=0.02, seed=3)}
    clouds[20_000] = np.concatenate([synth.make_scan(hall, "tiny", R_true, p_true, noise=0.02, seed=3 + j) for j in range(10)])[:20_000]
    gR, gp = lii.pose_grid(synth.rot_zyx(0.0, 0.0, 0.4 + 0.73), p_true + [3.3, -2.2, 0.0], 4.0, 0.5, 0.0, 2 * np.pi, np.deg2rad(10.0))
    pick = np.linspace(0, len(gR) - 1, max(KS)).astype(int)  # spread over the grid: near and far nodes alike
    P_all = poses_array((gR[pick], gp[pick]))
    reg = lii.Registrar(max_scan_points=32_768, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    ev = Events(reg)
    base = lii.State()
    d_P = reg.dev_alloc(P_all.nbytes)
    d_sc = reg.dev_alloc(max(KS) * 16)
    d_res = reg.dev_alloc(max(KS) * max(SIZES) * 4)
    rows = []
    for n in SIZES:
        cloud = np.ascontiguousarray(clouds[n], np.float32)
        reg.scan_upload(cloud)
        assert reg.downsample_skip() == n
        for K in KS:
            P = np.ascontiguousarray(P_all[:: max(KS) // K][:K])
            reg.dev_upload(d_P, P)
            for _ in range(2):
                reg.pose_score_dev(base, d_P, K, d_sc, d_res)
            reg.synchronize()
            dev_ms = []
            for _ in range(a.reps):
                ev.start()
                reg.pose_score_dev(base, d_P, K, d_sc, d_res)
                dev_ms.append(ev.stop_ms())
            reg.pose_score(base, P)
            host_ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                eff = reg.pose_score(base, P)[1]
                host_ms.append((time.perf_counter() - t0) * 1e3)
            states = []
            for k in range(K):
                st = lii.State()
                st.rot_end[:] = P[k, :9].reshape(3, 3)
                st.pos_end[:] = P[k, 9:]
                states.append(st)
            for st in states[:4]:
                reg.iekf_iterate(st, True, False)
            loop_ms, loop_eff = [], None
            for _ in range(a.reps):
                t0 = time.perf_counter()
                loop_eff = [int(reg.iekf_iterate(st, True, False)[90]) for st in states]
                loop_ms.append((time.perf_counter() - t0) * 1e3)
            reg.set_profiling(1)
            for st in states[:8]:
                reg.iekf_iterate(st, True, False)
            knn_ms = reg.timings()[7] / 8
            reg.set_profiling(0)
            rows.append(dict(n=n, K=K, dev=dev_ms, host=host_ms, loop=loop_ms, knn=knn_ms, same=bool(np.array_equal(eff, loop_eff))))
            print({k: (v if not isinstance(v, list) else [round(x, 3) for x in v]) for k, v in rows[-1].items()}, flush=True)
    reg.close()

    def mmm(v):
        return f"{np.mean(v):.3f} ({np.min(v):.3f} .. {np.max(v):.3f})"

    lines = ["# What lii_pose_score costs (one MI355X)", "",
             f"`python tools/pose_score_cost.py --reps {a.reps}`: the hall map of the tests ({len(map_pts)} points, cell 0.30 m), the `tiny` scan (ten of them for 20 000 "
             "points), K nodes spread over the 0.5 m / 10 degree re-localisation grid.  One run; every figure is the mean of "
             f"{a.reps} repetitions with (min .. max) behind it.", "",
             "lii_pose_score_dev with res: HIP events on the handle's stream around one enqueued call.  lii_pose_score (host arrays, no res) and the loop - K calls of "
             "lii_iekf_iterate(search = 1) on the same handle, each a host round trip with the Jacobian rows and the Gram sums - by the wall clock.", "",
             "| n_down | K | lii_pose_score_dev [ms] | ns per (pose, point) | of 8 TB/s at 100 B per pair | lii_pose_score, host [ms] | loop of K iterates [ms] | loop / host call | same effect_num |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        pairs = r["n"] * r["K"]
        d = float(np.mean(r["dev"]))
        lines.append(f"| {r['n']} | {r['K']} | {mmm(r['dev'])} | {1e6 * d / pairs:.2f} | {100 * pairs * PAIR_BYTES / (d * 1e-3) / HBM_BYTES_PER_S:.2f} % | {mmm(r['host'])} | "
                     f"{mmm(r['loop'])} | {np.mean(r['loop']) / np.mean(r['host']):.1f}x (worst case {np.min(r['loop']) / np.max(r['host']):.1f}x) | {r['same']} |")
    lines += ["", "The search alone: the specialised k-NN launch of one lii_iekf_iterate(search = 1) (lii_last_timings [7]) per query against the whole scoring kernel per pair "
              "(search by a wavefront per pair + fit + gate).", "",
              "| n_down | K | k-NN launch of an iterate [ms] | ns per query | lii_pose_score_dev ns per pair | ratio |", "|---|---|---|---|---|---|"]
    for r in rows:
        pairs = r["n"] * r["K"]
        per_pair = 1e6 * float(np.mean(r["dev"])) / pairs
        per_q = 1e6 * r["knn"] / r["n"]
        lines.append(f"| {r['n']} | {r['K']} | {r['knn']:.4f} | {per_q:.2f} | {per_pair:.2f} | {per_pair / per_q:.1f}x |")
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

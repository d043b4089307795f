#!/usr/bin/env python3
"""What lii_li_init_windows costs against the serial loop, on the reference's committed run (tests/golden/li_init/reference_run.npz:
1 369 aligned states, orig_odom_freq 10, cut_frame_num 5).

The windows are prefixes [0, n) of the run - what the reference's loop would have calibrated on had the initialisation fired at
frame n - with K ends spread evenly over [200, 1369] (K = 1: the whole run).  For K in 1, 4, 16, 64, 256, in one process:

  windows   one lii_li_init_windows call on the K windows: wall time around the ctypes call (upload and the one wait included)
  serial    K lii_li_init_resident calls on the same slices, one after the other, on a second handle
  scratch   the bytes of device scratch the windows call holds on a fresh handle (lii_li_init_windows_scratch)

  python tools/li_init_windows_cost.py [--reps 5] [--warmup 2] [--markdown]

Every time is the mean over --reps repetitions after --warmup, with (min .. max).  The records of the windows call are compared with
the serial calls' results byte for byte on the way ("same bits").  Prints one JSON line; --markdown adds the table of
profiles/li_init_windows.md."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = (1, 4, 16, 64, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import li_init_fixture as F
    import lidar_imu_init_amd as lii

    imu, lid = F.sequences()
    imu22, lid22 = np.ascontiguousarray(imu.to_records()), np.ascontiguousarray(lid.to_records())
    n = len(imu22)
    freq, cut = 10, 5
    serial_reg = lii.Registrar(max_scan_points=1000, max_map_points=1000)

    def timed(call):
        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(mean_ms=round(sum(ts) / len(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))

    rows = []
    for K in KS:
        counts = [n] if K == 1 else [int(c) for c in np.round(np.linspace(200, n, K))]
        wins = lii.li_init_window_array([(0, c) for c in counts])
        reg = lii.Registrar(max_scan_points=1000, max_map_points=1000)  # a fresh handle: its scratch is this K's
        got = []
        row = dict(K=K, windows=timed(lambda: got.append(reg.li_init_windows_records(imu22, lid22, wins, freq, cut))))
        row["scratch_bytes"], row["allocations"] = reg.li_init_windows_scratch()
        row["launches"], row["host_waits"] = got[-1][0].rep.launches, got[-1][0].rep.host_waits
        want = []

        def serial():
            want.clear()
            for c in counts:
                want.append(serial_reg.li_init_resident(imu22[:c], lid22[:c], freq, cut))

        row["serial"] = timed(serial)
        row["same_bits"] = all(q.status == 0 and bytes(q.res) == bytes(res) and bytes(q.rep.params) == bytes(rep.params)
                               and q.rep.time_lag_1 == rep.time_lag_1 for q, (res, rep) in zip(got[-1], want))
        row["serial_over_windows"] = round(row["serial"]["mean_ms"] / row["windows"]["mean_ms"], 3)
        rec = reg.li_init_windows(imu22, lid22, wins, freq, cut)
        s = lii.li_init_spread(rec)
        row["spread"] = dict(rot_deg_std=s["rot_deg_std"], dT_std=s["dT_std"], dlag_std=s["dlag_std"])
        reg.close()
        rows.append(row)
    serial_reg.close()
    print(json.dumps(dict(states=n, reps=a.reps, warmup=a.warmup, rows=rows)))
    if a.markdown:
        f = lambda t: "%.3f (%.3f .. %.3f)" % (t["mean_ms"], t["min_ms"], t["max_ms"])  # noqa: E731
        print("| K | lii_li_init_windows [ms] | K x lii_li_init_resident [ms] | serial / windows | per window [ms] | launches, waits | scratch [bytes] | same bits |")
        print("|---|---|---|---|---|---|---|---|")
        for r in rows:
            print("| %d | %s | %s | %.2fx | %.3f | %d, %d | %d | %s |" % (r["K"], f(r["windows"]), f(r["serial"]), r["serial_over_windows"],
                                                                        r["windows"]["mean_ms"] / r["K"], r["launches"], r["host_waits"],
                                                                        r["scratch_bytes"], r["same_bits"]))


if __name__ == "__main__":
    main()

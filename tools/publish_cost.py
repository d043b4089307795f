#!/usr/bin/env python3
"""What the registered clouds of a scan cost (lii_publish_set) on the stream100k shapes -> profiles/publish.md.

  python tools/publish_cost.py [--out profiles/publish.md] [--steps 200]

Measures, each GPU step in a child process of its own under `timeout -k 10`, the steps chained (a failure ends the script):
  1. kernel time of k_publish_world from ONE `rocprofv3 --kernel-trace --stats` run of a short child (no counters in that run);
  2. ms per scan of a registration loop with the order off, with DENSE to the device only, with DENSE + to_host fetched one scan late
     (from while_waiting of the next call);
  3. what a caller had to do before: lii_scan_download(h, 0) + pointBodyToWorld in numpy on the host, per scan.
`--child MODE` is the measured loop itself."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(mode, steps):
    import numpy as np
    import bench
    import lidar_imu_init_amd as lii
    wl = bench.build_workload("stream100k", 8)
    states0, tables = bench.start_states(wl)
    n_full = max(len(s) for s in wl["scans"])
    reg = lii.Registrar(max_scan_points=n_full + 1024, max_map_points=int(len(wl["map"]) * 1.5) + 1024, filter_size_map=wl["fs_map"])
    reg.map_build(wl["map"])
    reg.map_commit()
    dev = [reg.device_scan(s) for s in wl["scans"]]
    if mode == "dense":
        reg.publish_set(1, to_host=False)
    elif mode == "dense_host":
        reg.publish_set(1, to_host=True)
    got = [0]

    def late():
        got[0] += len(reg.publish_fetch(1, copy=False))

    def one(k, hook=None):
        j = k % len(dev)
        st = states0[j].copy()
        reg.scan_register(st, states0[j], imu_poses=tables[j], leaf=wl["fs_surf"], max_iterations=wl["max_it"], imu_en=True, scan_dev=dev[j],
                          scan_sorted=True, while_waiting=hook)
        return st

    for k in range(10):
        one(k)
    reg.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        st = one(k, late if mode == "dense_host" else None)
        if mode == "download":  # the parent commit's only way to the dense world cloud
            body = reg.scan_download(0)
            b = body[:, :3].astype(np.float64)
            w = ((b @ st.offset_R_L_I.T + st.offset_T_L_I) @ st.rot_end.T + st.pos_end).astype(np.float32)
            got[0] += len(w)
    reg.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    reg.close()
    print("RESULT " + json.dumps(dict(mode=mode, ms_per_scan=ms, points=got[0])))


def run(cmd, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"step failed ({r.returncode}): {' '.join(cmd)}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "publish.md"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps)
    me = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps)]
    res = {}
    for mode in ("off", "dense", "dense_host", "download"):
        out = run(me + ["--child", mode], 240)
        res[mode] = json.loads(out.split("RESULT ")[1].splitlines()[0])
    kern = "not measured (rocprofv3 is not on the PATH)"
    if shutil.which("rocprofv3"):
        with tempfile.TemporaryDirectory() as td:
            run(["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "pub", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                 "--steps", "40", "--child", "dense_host"], 300)
            for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
                for line in open(f):
                    if "k_publish_world" in line:
                        kern = line.strip()
    off = res["off"]["ms_per_scan"]
    lines = ["# What the registered clouds of a scan cost (stream100k shapes, one MI355X)", "",
             f"`python tools/publish_cost.py --steps {a.steps}`: a Python registration loop over 8 scans of 100 k points (leaf, IMU de-skew, "
             "time-sorted, scan on the device), each form in a process of its own.", "",
             "| form | ms per scan | added to the order-off loop |", "|---|---|---|"]
    names = dict(off="order off", dense="LII_PUB_DENSE, device only", dense_host="LII_PUB_DENSE + to_host, fetched one scan late (while_waiting)",
                 download="before: lii_scan_download(h, 0) + pointBodyToWorld in numpy")
    for mode in ("off", "dense", "dense_host", "download"):
        ms = res[mode]["ms_per_scan"]
        lines.append(f"| {names[mode]} | {ms:.4f} | {ms - off:+.4f} |")
    lines += ["", "k_publish_world in one `rocprofv3 --kernel-trace --stats` run of 50 scans (name, calls, total ns, average ns, ...):", "", "    " + kern, ""]
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

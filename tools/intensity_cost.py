#!/usr/bin/env python3
"""What the intensity channel costs (lii_scan_intensity_*, LII_PUB_INTENSITY) on the stream100k shapes.

  python tools/intensity_cost.py [--steps 200] [--out profiles/intensity_cost.md]

A Python registration loop over the 8 scans of the bench stream, each form in a child process of its own under `timeout -k 10`, the
steps chained (a failure ends the script):
  job       the bench's form: the job adopts scan_dev (such a job cannot carry intensity), nothing ordered
  setdev    lii_scan_set_device per scan, LII_PUB_DENSE | LII_PUB_DOWN ordered, no intensity: the form the next one is compared with
  intensity lii_scan_set_device + lii_scan_intensity_set_device per scan, LII_PUB_DENSE | LII_PUB_DOWN | LII_PUB_INTENSITY ordered
Per form: ms per scan of the loop, then a profiled pass (lii_set_profiling(h, 3)): launches and microseconds per scan and kind.
`--child MODE` is the measured loop itself."""
import argparse
import json
import os
import subprocess
import sys
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
    rng = np.random.default_rng(1)
    dint = [reg.device_intensity(rng.uniform(0, 255, len(s)).astype(np.float32)) for s in wl["scans"]]
    if mode == "setdev":
        reg.publish_set(1 | 2, to_host=False)
    elif mode == "intensity":
        reg.publish_set(1 | 2 | 16, to_host=False)

    def one(k):
        j = k % len(dev)
        st = states0[j].copy()
        kw = dict(imu_poses=tables[j], leaf=wl["fs_surf"], max_iterations=wl["max_it"], imu_en=True, scan_sorted=True)
        if mode == "job":
            reg.scan_register(st, states0[j], scan_dev=dev[j], **kw)
        else:
            reg.scan_set_device(dev[j])
            if mode == "intensity":
                reg.scan_intensity_set_device(dint[j])
            reg.scan_register(st, states0[j], **kw)

    for k in range(16):
        one(k)
    reg.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        one(k)
    reg.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    n_down = len(reg.scan_download(1))
    reg.set_profiling(1)
    reg.set_profiling(3)
    for k in range(40):
        one(k)
    prof, scans = reg.kernel_profile()
    reg.close()
    print("RESULT " + json.dumps(dict(mode=mode, ms_per_scan=ms, scans_per_s=1e3 / ms, n_scan=n_full, n_down=n_down, profiled_scans=scans,
                                      kinds={k: dict(us_per_scan=1e3 * v[0] / max(scans, 1), launches_per_scan=v[1] / max(scans, 1)) for k, v in prof.items()})))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensity_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps)
    me = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps)]
    modes = ("job", "setdev", "intensity")
    res = {m: json.loads(run(me + ["--child", m], 240).split("RESULT ")[1].splitlines()[0]) for m in modes}
    kinds = list(res["job"]["kinds"])
    n, nd = res["intensity"]["n_scan"], res["intensity"]["n_down"]
    lines = ["# What the intensity channel costs (stream100k shapes, one MI355X)", "",
             f"`python tools/intensity_cost.py --steps {a.steps}`: {n} points per scan, {nd} voxels.", "",
             "| form | ms per scan | scans/s |", "|---|---|---|"]
    lines += [f"| {m} | {res[m]['ms_per_scan']:.4f} | {res[m]['scans_per_s']:.0f} |" for m in modes]
    lines += ["", "Per kind and scan under lii_set_profiling(h, 3): microseconds (launches).", "", "| form | " + " | ".join(kinds) + " |", "|---|" + "---|" * len(kinds)]
    for m in modes:
        lines.append(f"| {m} | " + " | ".join(f"{res[m]['kinds'][k]['us_per_scan']:.2f} ({res[m]['kinds'][k]['launches_per_scan']:.2f})" for k in kinds) + " |")
    lines += ["", f"Extra traffic of the channel from the shapes: voxel emit 4 B x {n} read + 4 B x {nd} written = {4 * (n + nd) / 1e3:.0f} kB per scan; "
              f"publish (DENSE + DOWN) 8 B x {n} + 8 B x {nd} = {8 * (n + nd) / 1e3:.0f} kB; the attach copy 8 B x {n} = {8 * n / 1e3:.0f} kB.", ""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

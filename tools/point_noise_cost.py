#!/usr/bin/env python3
"""What lii_point_noise_set costs a scan on the stream100k shapes: the per-scan time of the bench's registration call with the model off
against another build of the library (the parent commit's), and with the model on against off.

  python tools/point_noise_cost.py [--steps 400] [--blocks 5] [--rounds 2] [--parent-lib PATH] [--out profiles/point_noise_cost.md]

Method (what a difference of a few hundred nanoseconds per fit launch needs): the two settings are compared INSIDE one process, on two
handles over the same map, in alternating blocks of `--steps` scans - off, on, off, on, ... - each block timed by the host clock around
registration calls that end in lii_synchronize, behind a warm-up of both handles; the figure of a setting is the median of its blocks, its
spread the range of them.  The two builds cannot share a process: each runs in a child of its own under `timeout -k 10`, the children
alternating - parent, this build, parent, this build - `--rounds` times; the steps are chained (a failure ends the script).  A block of
400 scans is some 80 ms of device time.  `--child` is the measured loop itself; the library a child loads is LII_LIB's (api.py)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(steps, blocks):
    import bench
    import lidar_imu_init_amd as lii
    wl = bench.build_workload("stream100k", 8)
    states0, tables = bench.start_states(wl)
    n_full = max(len(s) for s in wl["scans"])
    has_model = hasattr(lii.load_library(), "lii_point_noise_set")
    modes = ("off", "on") if has_model else ("off",)
    regs, devs = {}, {}
    for m in modes:
        reg = lii.Registrar(max_scan_points=n_full + 1024, max_map_points=int(len(wl["map"]) * 1.5) + 1024, filter_size_map=wl["fs_map"])
        reg.map_build(wl["map"])
        reg.map_commit()
        if m == "on":
            reg.set_point_noise()
        regs[m], devs[m] = reg, [reg.device_scan(s) for s in wl["scans"]]

    def one(m, k):
        j = k % len(wl["scans"])
        st = states0[j].copy()
        rep = regs[m].scan_register(st, states0[j], imu_poses=tables[j], leaf=wl["fs_surf"], max_iterations=wl["max_it"], imu_en=True,
                                    scan_sorted=True, scan_dev=devs[m][j])
        return rep["iterations"]

    passes = {}
    for m in modes:
        passes[m] = sum(one(m, k) for k in range(32)) / 32.0   # (warm-up; and the fit launches a scan runs)
        regs[m].synchronize()
    ms = {m: [] for m in modes}
    for _ in range(blocks):
        for m in modes:
            t0 = time.perf_counter()
            for k in range(steps):
                one(m, k)
            regs[m].synchronize()
            ms[m].append((time.perf_counter() - t0) / steps * 1e3)
    n_down = len(regs["off"].scan_download(1))
    for reg in regs.values():
        reg.close()
    print("RESULT " + json.dumps(dict(lib=os.environ.get("LII_LIB", "in-tree"), ms=ms, passes_per_scan=passes, n_scan=n_full, n_down=n_down)))


def run(cmd, limit, env):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"step failed ({r.returncode}): {' '.join(cmd)}")
    return json.loads(r.stdout.split("RESULT ")[1].splitlines()[0])


def summary(v):
    return f"{statistics.median(v) * 1e3:.2f} ({min(v) * 1e3:.2f} .. {max(v) * 1e3:.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_noise_cost.md"))
    a = ap.parse_args()
    if a.child:
        return child(a.steps, a.blocks)
    me = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--blocks", str(a.blocks)]
    builds = ([("parent", os.path.abspath(a.parent_lib))] if a.parent_lib else []) + [("this", "")]
    got = {name: dict(off=[], on=[]) for name, _ in builds}
    info = {}
    for _ in range(a.rounds):
        for name, lib in builds:
            env = dict(os.environ)
            env.pop("LII_LIB", None)
            if lib:
                env["LII_LIB"] = lib
            res = run(me, 400, env)
            info = res if name == "this" else info
            for m, v in res["ms"].items():
                got[name][m] += v
    lines = ["# What the per-point noise model costs a scan (stream100k shapes, one MI355X)", "",
             f"`python tools/point_noise_cost.py --steps {a.steps} --blocks {a.blocks} --rounds {a.rounds}" + (" --parent-lib <the parent commit's build>`" if a.parent_lib else "`")
             + f": {info['n_scan']} points per scan, {info['n_down']} voxels, {info['passes_per_scan']['off']:.2f} fit launches per scan.", "",
             "Microseconds per scan, host clock around blocks of registration calls ending in lii_synchronize: median over the blocks (range).", "",
             "| build | model | us per scan | blocks |", "|---|---|---|---|"]
    for name, _ in builds:
        for m in ("off", "on"):
            if got[name][m]:
                lines.append(f"| {name} | {m} | {summary(got[name][m])} | {len(got[name][m])} |")
    this = got["this"]
    if this["on"]:
        d = (statistics.median(this["on"]) - statistics.median(this["off"])) * 1e3
        lines += ["", f"Model on against off, this build: {d:+.2f} us per scan, {d / max(info['passes_per_scan']['on'], 1e-9):+.3f} us per fit launch "
                  f"({info['passes_per_scan']['on']:.2f} launches per scan with the model on)."]
    if a.parent_lib:
        d = (statistics.median(this["off"]) - statistics.median(got["parent"]["off"])) * 1e3
        lines += [f"Model off against the parent's build: {d:+.2f} us per scan."]
    lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the registered clouds of a scan cost (lii_publish_set) on the stream100k shapes -> profiles/publish.md.

  python tools/publish_cost.py [--out profiles/publish.md] [--steps 200]

Measures, each GPU step in a child process of its own under `timeout -k 10`, the steps chained (a failure ends the script):
  1. kernel time of k_publish_world from ONE `rocprofv3 --kernel-trace --stats` run of a short child (no counters in that run);
  2. ms per scan of a registration loop with the order off, with DENSE to the device only, with DENSE + to_host fetched one scan late
     (from while_waiting of the next call);
  3. what a caller had to do before: lii_scan_download(h, 0) + pointBodyToWorld in numpy on the host, per scan.
`--child MODE` is the measured loop itself.

  python tools/publish_cost.py --wire [--other-lib build_ab/NAME/libliinit_hip.so] [--steps 200] [--repeats 3]

The clouds as message bytes (lii_publish_wire_set) -> profiles/publish_wire.md: what the order adds to the same
loop against the path it replaces (lii_publish_fetch + lii_publish_fetch_intensity + a host pack into 48-byte records), and the publish
launch's duration with and without the order.  --other-lib: a second build of the library (tools/ab_build.sh) measured beside the in-tree
one, the two alternating - how the two store shapes of the records were compared (lii_publish.hip: wire_store_slab).
`--wire-child MODE` is that leg's measured loop."""
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


WIRE_CLOUDS = 1 | 4 | 8  # what the reference publishes every scan by default: the dense world cloud, the effect cloud, the body cloud
WIRE_MODES = dict(
    off="no order",
    pack="before: lii_publish_set (| LII_PUB_INTENSITY, to_host) + lii_publish_fetch + lii_publish_fetch_intensity + numpy pack into 48-byte records, one scan late",
    wire_dev="lii_publish_wire_set, device only (nothing fetched)",
    wire="lii_publish_wire_set + to_host, lii_publish_wire_fetch one scan late",
    both="both orders + to_host, lii_publish_wire_fetch one scan late")


def wire_child(mode, steps):
    """One form of the --wire leg: the registration loop of child(), the scans and their intensities resident on the device; what
    the host does with scan m's clouds happens inside call m + 1 (while_waiting), as INTEGRATION.md section 2 places it."""
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
    idev = [reg.device_intensity(rng.uniform(1.0, 255.0, len(s)).astype(np.float32)) for s in wl["scans"]]
    if mode in ("pack", "both"):
        reg.publish_set(WIRE_CLOUDS | 16, to_host=True)
    if mode in ("wire", "wire_dev", "both"):
        reg.publish_wire_set(WIRE_CLOUDS, to_host=mode != "wire_dev")
    got = [0]
    eff_int = np.float32(np.sqrt(1000.0))

    def pack():  # the per-point host loop every integrator had to write (numpy here: a C++ loop moves the same bytes)
        for cloud in (1, 4, 8):
            c4 = reg.publish_fetch(cloud, copy=False)
            rec = np.zeros((len(c4), 12), np.float32)
            rec[:, 0:3] = c4[:, 0:3]
            rec[:, 3] = 1.0
            rec[:, 8] = eff_int if cloud == 4 else reg.publish_fetch_intensity(cloud, copy=False)
            if cloud == 8:
                rec[:, 9] = c4[:, 3]
            got[0] += rec.nbytes

    def fetch():
        for cloud in (1, 4, 8):
            got[0] += reg.publish_wire_fetch(cloud, copy=False).nbytes

    hook = dict(pack=pack, wire=fetch, both=fetch).get(mode)

    def one(k, first=False):
        j = k % len(dev)
        st = states0[j].copy()
        reg.scan_set_device(dev[j])
        reg.scan_intensity_set_device(idev[j])
        reg.scan_register(st, states0[j], imu_poses=tables[j], leaf=wl["fs_surf"], max_iterations=wl["max_it"], imu_en=True, scan_sorted=True,
                          while_waiting=None if first else hook)

    for k in range(10):
        one(k, first=k == 0)
    reg.synchronize()
    got[0] = 0
    t0 = time.perf_counter()
    for k in range(steps):
        one(k)
    reg.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    reg.close()
    print("RESULT " + json.dumps(dict(mode=mode, ms_per_scan=ms, bytes_per_scan=got[0] / steps)))


def kernel_lines(me, mode, env):
    """k_publish_world's rows of one `rocprofv3 --kernel-trace --stats` run of a short child (no counters in that run)"""
    with tempfile.TemporaryDirectory() as td:
        run(["rocprofv3", "--kernel-trace", "--stats", "-d", td, "-o", "pub", "--output-format", "csv", "--"] + me + ["--steps", "40", "--wire-child", mode], 300, env)
        rows = []
        for f in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            rows += [line.strip() for line in open(f) if "k_publish_world" in line]
        return rows or ["(no k_publish_world launch in the trace)"]


def wire_leg(a):
    """--wire: what lii_publish_wire_set adds to a registration loop, against the path it replaces -> profiles/publish_wire.md.
    --other-lib: a second build of the library (tools/ab_build.sh), measured beside the in-tree one, the two alternating, --repeats times
    each."""
    me = [sys.executable, os.path.abspath(__file__)]
    libs = [("in-tree build", None)] + ([("--other-lib build", a.other_lib)] if a.other_lib else [])
    res = {}
    for rep in range(a.repeats):
        for lib_name, lib in libs:
            env = dict(os.environ, LII_LIB=os.path.abspath(lib)) if lib else None
            for mode in WIRE_MODES:
                if lib and mode in ("off", "pack"):
                    continue  # (the same code in both builds)
                out = run(me + ["--steps", str(a.steps), "--wire-child", mode], 240, env)
                res.setdefault((lib_name, mode), []).append(json.loads(out.split("RESULT ")[1].splitlines()[0]))
                print(f"repeat {rep} {lib_name} {mode}: {res[(lib_name, mode)][-1]['ms_per_scan']:.4f} ms per scan", file=sys.stderr, flush=True)
    kern = {}
    if shutil.which("rocprofv3"):
        for lib_name, lib in libs:
            env = dict(os.environ, LII_LIB=os.path.abspath(lib)) if lib else None
            for mode in ("pack", "wire_dev", "both") if not lib else ("wire_dev", "both"):
                kern[(lib_name, mode)] = kernel_lines(me, mode, env)
    off = min(r["ms_per_scan"] for r in res[("in-tree build", "off")])
    lines = ["# What the registered clouds as message bytes cost (stream100k shapes, one MI355X)", "",
             f"`python tools/publish_cost.py --wire --steps {a.steps} --repeats {a.repeats}" + (" --other-lib ...`" if a.other_lib else "`") +
             ": a Python registration loop over 8 scans of 100 k points (leaf, IMU de-skew, time-sorted; scans and intensities on the device), "
             "clouds DENSE | EFFECT | BODY, each form in a process of its own, the forms alternating; ms per scan: every repeat, then the least "
             "of them against the least of the loop without an order.", "",
             "| build | form | ms per scan (repeats) | least, added to the loop without an order | bytes the host handled per scan |", "|---|---|---|---|---|"]
    for (lib_name, mode), rs in res.items():
        ms = [r["ms_per_scan"] for r in rs]
        lines.append(f"| {lib_name} | {WIRE_MODES[mode]} | {' '.join(f'{m:.4f}' for m in ms)} | {min(ms) - off:+.4f} | {rs[0]['bytes_per_scan']:.0f} |")
    lines += ["", "The publish launch in one `rocprofv3 --kernel-trace --stats` run of 50 scans per form (name, calls, total ns, average ns, ...):", ""]
    for (lib_name, mode), rows in kern.items():
        lines += [f"- {lib_name}, {WIRE_MODES[mode]}:", ""] + ["      " + r for r in rows] + [""]
    if not kern:
        lines += ["not measured (rocprofv3 is not on the PATH)", ""]
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


def run(cmd, limit, env=None):
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"step failed ({r.returncode}): {' '.join(cmd)}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--wire", action="store_true", help="the lii_publish_wire_set leg -> profiles/publish_wire.md")
    ap.add_argument("--wire-child", choices=sorted(WIRE_MODES))
    ap.add_argument("--other-lib", help="--wire: a second build of the library (tools/ab_build.sh), measured beside the in-tree one")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "publish_wire.md" if a.wire else "publish.md")
    if a.child:
        return child(a.child, a.steps)
    if a.wire_child:
        return wire_child(a.wire_child, a.steps)
    if a.wire:
        return wire_leg(a)
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

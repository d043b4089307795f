#!/usr/bin/env python3
"""Wall time of LI_Initialization on the reference's committed run (tests/golden/li_init/reference_run.npz: 1 369 aligned states,
orig_odom_freq 10, cut_frame_num 5), three ways in one process on one handle:

  host_chain    lii_li_init_run with lii_li_init_set_device(h, 0): conditioning on the host, host LM around lii_calib_eval
  device_chain  lii_li_init_run with lii_li_init_set_device(h, 1): the two filters and the cross-correlation through the device
  resident      lii_li_init_resident, aligned form: one upload, a fixed sequence of launches, one wait

  python tools/li_init_time.py [--calls 20] [--warmup 3]

Each figure is the median over --calls calls after --warmup calls, timed on the host around the ctypes call (upload and final wait
included).  Prints one JSON line: the three medians in ms, their minima and maxima, the launches and waits the resident call reports.
Under `rocprofv3 --kernel-trace --stats -- python tools/li_init_time.py` the per-kernel times of profiles/li_init_resident.md."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import li_init_fixture as F
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd import api

    imu, lid = F.sequences()
    imu22, lid22 = np.ascontiguousarray(imu.to_records()), np.ascontiguousarray(lid.to_records())
    n = len(imu22)
    reg = lii.Registrar(max_scan_points=1000, max_map_points=1000)
    L, h = reg.L, reg.h
    res = api.lii_calib_result()
    l1, tot = C.c_double(0), C.c_double(0)
    job = api.lii_li_init_job(C.sizeof(api.lii_li_init_job), 0, imu22.ctypes.data, n, lid22.ctypes.data, n, 0.0, 10, 5)
    rep = api.lii_li_init_report(C.sizeof(api.lii_li_init_report))
    pi, pl = imu22.ctypes.data_as(C.c_void_p), lid22.ctypes.data_as(C.c_void_p)

    def run_chain():
        assert L.lii_li_init_run(h, pi, pl, n, 10, 5, C.byref(res), C.byref(l1), C.byref(tot)) == 0

    def run_resident():
        assert L.lii_li_init_resident(h, C.byref(job), C.byref(res), C.byref(rep)) == 0

    def measure(call):
        for _ in range(a.warmup):
            call()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))

    out = dict(states=n, calls=a.calls, warmup=a.warmup)
    reg.li_init_set_device(False)
    out["host_chain"] = measure(run_chain)
    out["host_chain"]["iterations"] = res.iterations[:]
    reg.li_init_set_device(True)
    out["device_chain"] = measure(run_chain)
    reg.li_init_set_device(False)
    out["resident"] = measure(run_resident)
    out["resident"].update(iterations=res.iterations[:], launches=rep.launches, host_waits=rep.host_waits)
    reg.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

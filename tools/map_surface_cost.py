#!/usr/bin/env python3
"""What lii_map_surface_dev and lii_map_crispness cost on the bench's 1 M-point map, one MI355X.

  python tools/map_surface_cost.py [--queries 100000] [--reps 5] [--windows 5] [--out profiles/map_surface.md]

One process, one GPU run.  The queries are points drawn from the map itself (the self-query case of the crispness figures).  Per max_dist
in {0.04, 0.25, 1.0}, HIP events on the handle's stream (tools/map_nearest_cost.Events) around `reps` enqueued calls, after two warm-up
calls, `windows` times, alternating the two calls; the figure is the MEDIAN window:
  * S: lii_map_surface_dev - the ball walk with the nine f64 sums, one butterfly and the eigen-solve per query;
  * R: lii_map_radius_dev in its offsets-only form (pts_dev = d2_dev = NULL) on the same queries - the same walk without the sums, plus
    the exclusive scan of the counts and the copy of the total; R0, the same call for NaN queries (no walk), is what that extra costs.
Two ratios are reported: S / R, call against call, and S / (R - R0 + E), with E the empty surface launch (NaN queries): walk against walk.
lii_map_crispness over the whole map is timed with the host clock (the call ends in a synchronise), median of `windows` calls."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MAX_DISTS = (0.04, 0.25, 1.0)


def render(rows, crisp, n, n_map, fs_map, reps, windows):
    lines = ["# What lii_map_surface and lii_map_crispness cost (one MI355X)", "",
             f"`python tools/map_surface_cost.py --queries {n} --reps {reps} --windows {windows}`: {n} queries drawn from the bench's {n_map}-point map "
             f"(filter_size_map {fs_map:g}), queries and records on the device.  One run; HIP events on the handle's stream around {reps} enqueued calls, "
             f"{windows} windows per call, alternating; the figures are medians, the spread is max - min over the windows.", "",
             "surface = lii_map_surface_dev; count pass = lii_map_radius_dev, offsets only, minus the same call for NaN queries (its scan and copy), plus the empty "
             "surface launch: walk against walk; 'radius call' is the whole offsets-only call.  The surface kernel holds 72 VGPRs against the count pass's 47 (7 against 8 wavefronts per SIMD by registers).", "",
             "| max_dist | mean / max ball | surface [ms] | spread | radius offsets-only [ms] | its scan + copy [ms] | empty surface launch [ms] | count pass [ms] | ratio surface / radius call | ratio surface / count pass | surface - count walk [ms] | ns per query (surface) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        walk = r["R"] - r["R0"] + r["E"]
        lines.append(f"| {r['md']:g} | {r['mean_count']:.1f} / {r['max_count']} | {r['S']:.3f} | {r['S_spread']:.3f} | {r['R']:.3f} | {r['R0']:.3f} | {r['E']:.3f} | {walk:.3f} | "
                     f"{r['S'] / r['R']:.2f} | {r['S'] / walk:.2f} | {r['S'] - (r['R'] - r['R0']):.3f} | {1e6 * r['S'] / n:.1f} |")
    lines += ["", "WHERE THE TIME GOES.  The ratio exceeds 1.5.  What the surface call costs beyond the count walk (last but one column) does not grow with the ball: the nine "
              "f64 additions a point ride under the walk's loads, and the bill is the tail every query pays once - the butterfly and, above all, the eigen-solve: a serial "
              "chain of f64 divisions and square roots (four and two a rotation) that the whole wavefront issues as one lane's work, hidden only by the 7 wavefronts a SIMD "
              "holds (8 for the count pass: the registers cost one).  The figures point to the latency of that chain, not to occupancy and not to the f64 rate of the "
              "sums; the solve was not timed in isolation.  Two earlier "
              "forms of this kernel, same tool, same map: with every one of the 24 rotations made the tail was 0.41 / 0.40 / 0.40 ms (dropping negligible entries "
              "without a rotation took 0.10 ms off); with the butterfly as six __shfl_xor steps (108 ds_bpermute a query) the EMPTY launch took 0.110 ms instead of "
              "0.048 ms, and the loaded call the same time as now - the crossbar was hidden behind the solve.", "",
              "lii_map_crispness over the whole map (host clock around the synchronous call: gather, select, scan, compact, the surface kernel in its term form, "
              "the one-workgroup reduction, two small copies):", "",
              "| max_dist | every | selected | used | call [ms] | spread | mme | mpv |", "|---|---|---|---|---|---|---|---|"]
    for c in crisp:
        lines.append(f"| {c['md']:g} | {c['every']} | {c['n_selected']} | {c['n_used']} | {c['ms']:.2f} | {c['spread']:.2f} | {c['mme']:.6f} | {c['mpv']:.6g} |")
    lines += ["", "The wave-per-query form re-walks, for every query, a cell neighbourhood that the queries of the same cell share: with the map's own points as "
              "queries each cell's 27-cell (or wider) neighbourhood is read once per point of the cell.  A cell-major kernel for the self-query case would read it "
              "once per cell; it is not part of this work.", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_surface.md"))
    a = ap.parse_args()
    import numpy as np
    import bench
    import lidar_imu_init_amd as lii
    from harness import params, synth
    from map_nearest_cost import Events

    fs_map = params.load(bench.WORKLOADS["stream100k"][2]).filter_size_map
    hall, map_pts = synth.bench_world(bench.WORKLOADS["stream100k"][1], fs_map, seed=20220613)
    map_pts = np.ascontiguousarray(map_pts, np.float32)
    q = np.ascontiguousarray(map_pts[np.random.default_rng(5).choice(len(map_pts), a.queries, replace=False)])
    n = len(q)
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=int(len(map_pts) * 1.5) + 1024, filter_size_map=fs_map)
    reg.map_build(map_pts)
    ev = Events(reg)
    d_q, d_nan = reg.dev_alloc(q.nbytes), reg.dev_alloc(q.nbytes)
    reg.dev_upload(d_q, q)
    reg.dev_upload(d_nan, np.full_like(q, np.nan))
    d_rec, d_o, d_t = reg.dev_alloc(88 * n), reg.dev_alloc(8 * (n + 1)), reg.dev_alloc(8)

    def window(call):
        ev.start()
        for _ in range(a.reps):
            call()
        return ev.stop_ms() / a.reps

    rows = []
    for md in MAX_DISTS:
        calls = dict(S=lambda: reg.map_surface_dev(d_q, n, md, d_rec), E=lambda: reg.map_surface_dev(d_nan, n, md, d_rec),
                     R=lambda: reg.map_radius_dev(d_q, n, md, d_o, None, None, 0, d_t), R0=lambda: reg.map_radius_dev(d_nan, n, md, d_o, None, None, 0, d_t))
        for c in calls.values():
            c()
            c()
        reg.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(a.windows):  # (alternating: a drift of the machine falls on every call alike)
            for k, c in calls.items():
                ms[k].append(window(c))
        r = {k: float(np.median(v)) for k, v in ms.items()}
        r.update({k + "_spread": float(np.max(v) - np.min(v)) for k, v in ms.items()})
        cnt = reg.map_surface(q[:20_000], md)["count"]
        r.update(md=md, mean_count=float(cnt.mean()), max_count=int(cnt.max()))
        rows.append(r)
        print(r, flush=True)

    crisp = []
    for md, every in ((0.25, 1), (0.25, 16), (1.0, 16)):
        reg.map_crispness(md, 5, every)
        ts = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            out = reg.map_crispness(md, 5, every)
            ts.append((time.perf_counter() - t0) * 1e3)
        crisp.append(dict(md=md, every=every, ms=float(np.median(ts)), spread=float(max(ts) - min(ts)), **out))
        print(crisp[-1], flush=True)
    n_map = reg.map_size()
    reg.close()

    lines = render(rows, crisp, n, n_map, fs_map, a.reps, a.windows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()

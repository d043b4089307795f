#!/usr/bin/env python3
"""bench.py — ICP+ESKF scans/sec on the north-star stream (100 k points/scan vs a 1 M-point local map).

A "step" is ONE lii_scan_register call (src/laserMapping.cpp:909-1134) on a scan that is already resident in HBM:
    scan adoption + time extent -> IMU back-propagation de-skew -> voxel-grid down-sampling (leaf 0.05) -> iterated
    Kalman update, everything on the GPU and device-driven (k-NN + plane fit + residual + Jacobian + H^T R^-1 H
    reduction + 24-state solve + the reference's convergence / re-match schedule), one host round trip per scan.
The scans arrive time-sorted, as Preprocess::process_cut_frame_* hands them over (src/preprocess.cpp:296-302).
The local map is static during the timed region unless --map-update (map_incremental every step); 8 distinct scans are
cycled and every step starts from that scan's propagated state (all of this is stated in `config.workload`).

Contract: python bench.py --gpus N --steps K --warmup W ; rank 0 prints ONE JSON line.
A plain run sets up, warms up, times the K steps, writes the last step's outputs (--dump-outputs DIR) and prints the line.  Everything
else the line can carry - value_long, roofline, the per-launch profile, parity, the CPU baseline, the calibration record, the complete
pipeline, the other transports and partitions of a sharded job - is measured only with --full (the --no-* switches apply there).
N > 1 (launched by torch.distributed.run): every rank holds the map and receives the whole scan; the de-skew and the
voxel filter run replicated (their output is bit-identical on every rank), the down-sampled cloud - voxel-key ordered -
is split into contiguous blocks inside the library, and each IEKF iteration sums the 91 normal-equation scalars over
the ranks ("strong" scaling: the per-scan work is fixed).  With --full the line also carries `parity`: the final state of every
distinct scan of the stream against the CPU oracle (computed in the cpu_baseline leg, outside the timed region).
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); measured copy ceiling 6290 GB/s

WORKLOADS = {
    # name: (sensor, map points, yaml the parameters come from, cut_frame_num or None = the yaml's own)
    # filter_size_surf / filter_size_map / max_iteration are READ from the reference-format yaml + launch files under
    # harness/config (harness/params.py); ouster.yaml's scan_line is 128 there, not the shipped 32.
    "stream100k": ("stream100k", 1_000_000, "ouster", 1),
    "vlp16": ("vlp16", 300_000, "velodyne", 1),
    "os1_128": ("os1_128", 1_000_000, "ouster", 1),
    "os1_128_cut3": ("os1_128", 1_000_000, "ouster", 3),   # BASELINE.json configs[3]: 30 Hz sub-frames of ~43.7 k points
    "dense500k": ("dense500k", 1_000_000, "hesai", 1),
}


# --edge: the map lacks a patch of the floor that every pose of the stream looks at - the part of the hall a live sensor has not mapped
# yet.  Every scan then has queries whose 2.2 m ball (max_match_dist2 = 5) reaches past what the map holds: the completion path of
# k_fit_reduce on EVERY scan, where the plain stream has it on one scan of eight (profiles/r06_edge.md).
EDGE_PATCH = ((9.0, 11.4), (-1.2, 1.2), (-10.0, -1.0))  # x, y, z ranges [m] of the floor patch taken out of the map (--edge-wide: six times the area)
EDGE_PATCH_WIDE = ((8.0, 14.0), (-3.0, 3.0), (-10.0, -1.0))


def build_workload(name, n_scans, seed=20220613, map_cache=None, edge=False):
    # (edge: False, True = EDGE_PATCH, "wide" = EDGE_PATCH_WIDE)
    """Synthetic stream: `n_scans` sweeps from poses on a small loop, time-sorted (and, for cut_frame_num > 1, cut into
    sub-frames the way process_cut_frame_pcl2 does: equal point counts, time re-based to the sub-frame start)."""
    from harness import params, synth
    sensor, n_map, yaml_name, cut = WORKLOADS[name]
    prm = params.load(yaml_name)
    fs_map, fs_surf, max_it = prm.filter_size_map, prm.filter_size_surf, prm.max_iteration
    if map_cache is not None and (n_map, fs_map) in map_cache:
        hall, map_pts = map_cache[(n_map, fs_map)]
    else:
        hall, map_pts = synth.bench_world(n_map, fs_map, seed=seed)
        if map_cache is not None:
            map_cache[(n_map, fs_map)] = (hall, map_pts)
    if edge:
        (x0, x1), (y0, y1), (z0, z1) = EDGE_PATCH_WIDE if edge == "wide" else EDGE_PATCH
        m = map_pts
        inside = (m[:, 0] > x0) & (m[:, 0] < x1) & (m[:, 1] > y0) & (m[:, 1] < y1) & (m[:, 2] > z0) & (m[:, 2] < z1)
        map_pts = np.ascontiguousarray(m[~inside])
    rng = np.random.default_rng(seed)
    scans, poses, sweeps = [], [], []
    k = 0
    while len(scans) < n_scans:
        yaw = 0.15 * k
        R = synth.rot_zyx(0.02 * np.sin(k), 0.015 * np.cos(k), yaw)
        p = np.array([3.0 * np.cos(0.2 * k), 2.0 * np.sin(0.2 * k), 0.2 + 0.05 * np.sin(k)])
        sweep = synth.make_scan(hall, sensor, R, p, noise=0.02, seed=seed + k)
        sweep = sweep[np.argsort(sweep[:, 3], kind="stable")]  # time order, as the ingest delivers it
        sweeps.append(sweep)  # (the whole driver message: complete_pipeline.from_wire packs it as PointCloud2 bytes)
        for c in range(cut):
            lo, hi = (len(sweep) * c) // cut, (len(sweep) * (c + 1)) // cut
            sub = sweep[lo:hi].copy()
            sub[:, 3] -= sub[0, 3]
            if len(scans) < n_scans:
                scans.append(sub)
                poses.append((R, p))
        k += 1
    return dict(name=name, map=map_pts, hall=hall, scans=scans, poses=poses, fs_map=fs_map, fs_surf=fs_surf, max_it=max_it, rng=rng,
                sweep_s=0.1 / cut, params=prm, edge=edge, sweeps=sweeps, cut=cut)


def start_states(wl):
    """The state IMU propagation hands to the update for every scan of the stream: the true pose with a perturbation."""
    import lidar_imu_init_amd as lii
    from harness.lo_harness import so3_exp  # numpy helper of the test harness (the oracle is only used by cpu_baseline)
    states0 = []
    for (R, p) in wl["poses"]:
        st = lii.State()
        st.rot_end[:] = R
        st.pos_end[:] = p
        pert = np.r_[0.004, -0.003, 0.005, 0.03, -0.02, 0.015, np.zeros(18)]
        st.rot_end[:] = st.rot_end @ so3_exp(pert[0:3])  # StatesGroup boxplus on the pose part (include/common_lib.h:126-136)
        st.pos_end[:] = st.pos_end + pert[3:6]
        states0.append(st)
    tables = [pose_table(s0.rot_end, s0.pos_end, sweep_s=wl["sweep_s"]) for s0 in states0]  # consistent with the propagated state
    return states0, tables


def oracle_scan_register(O, tree, scan, s0, table, leaf, max_it, threads):
    """The oracle's restatement of one lii_scan_register call: time sort + IMU back-propagation de-skew
    (src/IMU_Processing.hpp:390-414), voxel grid (src/laserMapping.cpp:917-919), iterated update (:957-1134)."""
    und = O.undistort_imu(scan, table, s0.rot_end, s0.pos_end, s0.offset_R_L_I, s0.offset_T_L_I)
    body = und if not leaf > 0 else O.voxel_grid(und, leaf)[0]
    r = tree.iekf_update(body, s0.pod, s0.pod, max_iterations=max_it, imu_en=True, threads=threads)
    r["n_down"] = len(body)
    return r


def exact_posterior(P_prior, normal_eq):
    """The posterior covariance of the update in exact arithmetic: (P^-1 + G (+) 0)^-1 - what the reference's (I - K H) P with
    K = (H^T R^-1 H (+) 0 + P^-1)^-1 H^T R^-1 (src/laserMapping.cpp:1081-1114) is algebraically - from the prior the update was
    given and the 12 x 12 G = H^T R^-1 H of its stopping iteration (lii_iekf_report::normal_eq[0:78]), in 60-digit arithmetic."""
    import mpmath as mp
    mp.mp.dps = 60
    G = np.zeros((12, 12))
    G[np.triu_indices(12)] = np.asarray(normal_eq)[:78]
    G = G + G.T - np.diag(np.diag(G))
    A = mp.matrix(np.asarray(P_prior, np.float64).tolist()) ** -1
    for i in range(12):
        for j in range(12):
            A[i, j] += mp.mpf(float(G[i, j]))
    S = A ** -1
    return np.array([[float(S[i, j]) for j in range(24)] for i in range(24)])


def cov_rel_err(P, P_ref):
    """max_ij |P - P_ref|_ij / sqrt(P_ref_ii P_ref_jj): element-wise, relative to the scale of the two states an entry couples."""
    d = np.sqrt(np.abs(np.diag(P_ref)))
    return float(np.max(np.abs(np.asarray(P) - P_ref) / np.outer(d, d)))


def parity_against_oracle(O, ref, state_pod, rep, prior_cov=None):
    """Differences between one GPU result (final lii_state + report) and the oracle's (dict of oracle_scan_register)."""
    v = O.StateView(ref["state"])
    w = O.StateView(np.asarray(state_pod))
    d24 = O.state_boxminus(np.asarray(state_pod), ref["state"])
    # the LiDAR pose R_end R_LI, R_end T_LI + p_end: what the measurements observe (in LIO mode the split of a correction between
    # the IMU pose and the extrinsic is held by the prior alone, and is only as determinate as cond(P^-1 + H^T R^-1 H) eps)
    Rl_v, Rl_w = v.rot_end @ v.offset_R_L_I, w.rot_end @ w.offset_R_L_I
    pl_v, pl_w = v.rot_end @ v.offset_T_L_I + v.pos_end, w.rot_end @ w.offset_T_L_I + w.pos_end
    extra = {}
    if prior_cov is not None:
        # both posteriors against the EXACT posterior of the same normal equations: the arithmetic noise of the reference's
        # algebra (restated by the oracle: two 24 x 24 inversions) and of the device's (one 12-step elimination, symmetrised)
        Ps = exact_posterior(prior_cov, rep["normal_eq"])
        extra = dict(dcov_gpu_exact=cov_rel_err(w.cov, Ps), dcov_oracle_exact=cov_rel_err(v.cov, Ps), dcov_gpu_oracle=cov_rel_err(w.cov, v.cov))
    return dict(**extra, dp=float(np.linalg.norm(v.pos_end - w.pos_end)),
                dtheta=float(np.linalg.norm(O.log_so3(v.rot_end.T @ w.rot_end))),
                dp_lidar=float(np.linalg.norm(pl_v - pl_w)), dtheta_lidar=float(np.linalg.norm(O.log_so3(Rl_v.T @ Rl_w))),
                dstate_pose_ext=float(np.max(np.abs(d24[:12]))), dstate_rest=float(np.max(np.abs(d24[12:]))),
                dcov_rel=float(np.max(np.abs(v.cov - w.cov)) / max(np.max(np.abs(v.cov)), 1e-300)),
                iters_equal=bool(rep["iterations"] == ref["iters"]),
                searches_equal=bool(rep["searches"] == int(ref["logs"][:, 0].sum())),
                effect_diff=int(abs(rep["effect_num"] - int(ref["logs"][-1, 1]))))


def pose_table(R_end=np.eye(3), p_end=np.zeros(3), n_poses=12, sweep_s=0.1):
    """A pose table of a body that barely moves during the sweep and ends at (R_end, p_end) (the scans are generated
    undistorted); every point still goes through the full back-propagation arithmetic (sin/cos, 3 rotations)."""
    from lidar_imu_init_amd import pose6d_array
    T = pose6d_array(n_poses)
    for k in range(n_poses):
        T[k, 0] = sweep_s * k / (n_poses - 1) if k else 0.0
        T[k, 4:7] = [1e-5, -2e-5, 1.5e-5]      # gyr
        T[k, 7:10] = [1e-5, 1e-5, 0.0]          # vel
        T[k, 10:13] = p_end
        T[k, 13:22] = np.asarray(R_end).reshape(-1)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--profile-every", type=int, default=8, help="HIP-event kernel timing on every Nth timed step (0: never)")
    ap.add_argument("--upload", action="store_true",
                    help="hand every scan over from HOST memory (lii_scan_upload, PCIe inside the timed region) instead of HBM")
    ap.add_argument("--separate-calls", action="store_true", help="undistort / downsample / update as three library calls")
    ap.add_argument("--python-loop", action="store_true", help="drive the per-scan loop from Python (ctypes) instead of the C++ host loop")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="stream100k", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true", help="skip the separately timed complete-pipeline figure (upload + register + map update)")
    ap.add_argument("--no-downsample", action="store_true",
                    help="skip the GPU voxel-grid filter (mapping/filter_size_surf) that the step includes by default")
    ap.add_argument("--map-update", action="store_true",
                    help="also run map_incremental (device-side ikd-Tree Add_Points semantics + index rebuild) every step")
    ap.add_argument("--map-update-separate", action="store_true",
                    help="--map-update / the complete pipeline: lii_map_incremental as a call of its own behind lii_scan_register (round 3's form) "
                         "instead of lii_scan_job::map_update (its launches enqueued behind the update's passes)")
    ap.add_argument("--long-steps", type=int, default=400, help="steps of the second timed region behind `value` (value_long; 0: none; skipped when --steps is larger)")
    ap.add_argument("--kernel-profile-steps", type=int, default=64, help="steps of the per-launch profile pass (roofline.kernels / roofline.scan; 0: none)")
    ap.add_argument("--no-live-traffic", action="store_true", help="roofline.traffic from the committed PMC profile instead of two rocprofv3 --pmc passes of this command made now (child processes, ~15 s each)")
    ap.add_argument("--no-calibration", action="store_true", help="leave the calibration record (GPU LI-Init vs oracle / reference result / ground truth) out of the line")
    ap.add_argument("--no-calibration-stream", action="store_true", help="calibration record: the reference's committed run only, not the synthetic LO -> LI-Init stream")
    ap.add_argument("--partition", default=os.environ.get("LII_BENCH_PARTITION", "voxel"), choices=["index", "voxel"],
                    help="--gpus N > 1: how the library splits the down-sampled cloud over the ranks (lii_comm_set_partition): contiguous blocks, or "
                         "by voxel inside the fused filter; `value` is measured with this one, the other is timed beside it (`partitions`)")
    ap.add_argument("--prime", type=int, default=150, help="untimed runtime-priming steps before the warm-up")
    ap.add_argument("--scans", type=int, default=8, help="distinct resident scans cycled through")
    ap.add_argument("--cell-size", type=float, default=0.0, help="k-NN grid cell edge [m]; 0 = 2 x filter_size_map")
    ap.add_argument("--edge", action="store_true", help="every scan looks past the edge of the map (a floor patch in view of every pose is missing from it)")
    ap.add_argument("--edge-wide", action="store_true", help="--edge with a patch of six times the area: more unfinished queries per search pass than the completion workgroups take (256)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline figure as well: value_long, roofline and the per-launch profile, parity, the CPU "
                         "baseline, the calibration record, the complete pipeline, the other transports / partitions of a sharded job")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the final state of the last timed step (what the caller of lii_scan_register receives) as DIR/<field>.npy, float64")
    ap.add_argument("--cpu-sweep-worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_sweep_worker:  # (cpu_baseline's thread sweep, in a process of its own: see there)
        return cpu_sweep_worker(args)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import torch  # device sync + torch.distributed rendezvous only (plumbing)
    import lidar_imu_init_amd as lii
    dist = None
    # LII_BENCH_ONE_DEVICE=1: rehearsal of the multi-rank path on a single-GPU box (every rank drives device 0, rendezvous
    # over gloo; RCCL refuses two ranks on one device, the library's node-local mailbox transport does not).  The ranks
    # then time-share one GPU: the line it prints proves the path, it is not a scaling number.
    one_device = world > 1 and os.environ.get("LII_BENCH_ONE_DEVICE") == "1"
    if one_device:
        local_rank = 0
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local_rank)
        if one_device:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    if args.edge_wide:
        args.edge = "wide"
    wl = build_workload(args.workload, args.scans, edge=args.edge)
    n_full = max(len(s) for s in wl["scans"])
    reg = lii.Registrar(max_scan_points=n_full + 1024, max_map_points=int(len(wl["map"]) * 1.5) + 1024,
                        filter_size_map=wl["fs_map"], map_cell_size=args.cell_size, device=local_rank)
    def attach(transport):
        """(Re-)creates the job's communicator with the named transport on every rank."""
        if os.environ.get("LII_BENCH_DEBUG"):
            print(f"[bench rank {rank}] attach {transport} / {partition_now[0]}", file=sys.stderr, flush=True)
        reg.comm_destroy()
        uid = [reg.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        reg.comm_init(world, rank, uid[0], transport)
        reg.comm_set_partition(partition_now[0])

    partition_now = [args.partition]
    # Which transport of the 91-scalar exchange `value` is measured on: ranks on distinct devices -> RCCL (north_star / SURVEY 8(e):
    # "one RCCL all-reduce", so the headline line says config.transport "rccl" and config.rccl_ranks == world); the library's own
    # node-local choice (the peer-mapped HBM mailbox) and the host mailbox are timed beside it under `transports`.  Ranks
    # rehearsing on ONE device cannot use RCCL (it refuses two ranks on a device): the library's choice there.
    default_transport = os.environ.get("LII_BENCH_TRANSPORT", "auto" if one_device else "rccl")
    attach_errors = {}
    if world > 1:
        try:
            attach(default_transport)
        except Exception as e:  # (the same on every rank: the set-up is collective) - the library's own choice carries the line instead
            attach_errors[default_transport] = {"error": str(e)[:200]}
            if default_transport == "auto":
                raise
            default_transport = "auto"
            attach(default_transport)
    reg.map_build(wl["map"])
    reg.map_commit()
    # Every rank receives the WHOLE scan (and holds the whole map) and the library splits the work (lii_comm_set_partition): by voxel
    # (--partition voxel, the default here: every rank de-skews the scan but inserts, filters, searches and fits only the voxels whose
    # key hashes to it) or by index (de-skew + voxel filter replicated, contiguous blocks of the down-sampled cloud) - sharded ==
    # unsharded up to the re-association of the 91 sums either way (tests/test_gpu_multirank.py).
    dev_scans = [reg.device_scan(s) for s in wl["scans"]]
    host_scans = [np.ascontiguousarray(s) for s in wl["scans"]]
    states0, tables = start_states(wl)

    iters_total = [0]
    search_total = [0]

    def step(k):
        j = k % len(dev_scans)
        hand_over = None
        if args.upload:
            reg.scan_upload(host_scans[j])
        elif args.separate_calls:
            reg.scan_set_device(dev_scans[j])
        else:
            hand_over = dev_scans[j]  # lii_scan_job::scan_dev: the scan is adopted inside the one call
        st = states0[j].copy()
        if args.separate_calls:
            s0 = states0[j]
            reg.undistort_imu(tables[j], s0.rot_end, s0.pos_end, s0.offset_R_L_I, s0.offset_T_L_I)
            if not args.no_downsample:
                reg.downsample(wl["fs_surf"], want_count=False)
            else:
                reg.downsample_skip()
            rep = reg.iekf_update(st, states0[j], max_iterations=wl["max_it"], imu_en=True)
        else:  # the same three stages through the one-call entry point (one host round trip per scan)
            rep = reg.scan_register(st, states0[j], imu_poses=tables[j], leaf=0.0 if args.no_downsample else wl["fs_surf"],
                                    max_iterations=wl["max_it"], imu_en=True, scan_dev=hand_over, scan_sorted=True,
                                    map_update=args.map_update and not args.map_update_separate)
        iters_total[0] += rep["iterations"]
        search_total[0] += rep["searches"]
        if args.map_update and (args.map_update_separate or args.separate_calls):
            reg.map_incremental(st)
        return st

    # The timed loop is the C++ host loop of harness/stream_driver.cpp (one lii_scan_register per scan, the scan handed over
    # in HBM): the reference's host is C++, and a ctypes round trip per scan is ~25 us of interpreter time no deployment
    # pays.  --python-loop / --separate-calls / --upload / LII_BENCH_TRACE keep the loop in Python (same calls).
    native = None
    if not (args.python_loop or args.separate_calls or args.upload or os.environ.get("LII_BENCH_TRACE")):
        import ctypes as C

        class StreamScan(C.Structure):
            _fields_ = [("scan_dev", C.c_void_p), ("n_points", C.c_int32), ("n_poses", C.c_int32), ("poses", C.c_void_p),
                        ("state0", C.c_void_p)]
        drv_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "harness", "libliinit_stream.so")
        if not os.path.exists(drv_path):
            raise SystemExit(f"{drv_path} missing - run `python -c 'import __graft_entry__ as g; g.build()'` (or --python-loop)")
        drv = C.CDLL(drv_path)
        drv.lii_stream_set_map_in_job(0 if args.map_update_separate else 1)
        drv.lii_stream_run.restype = C.c_int
        drv.lii_stream_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        tables_c = [np.ascontiguousarray(t, np.float64) for t in tables]
        stream = (StreamScan * len(dev_scans))()
        for j, d in enumerate(dev_scans):
            stream[j].scan_dev, stream[j].n_points = d[0], d[1]
            stream[j].poses, stream[j].n_poses = tables_c[j].ctypes.data, len(tables_c[j])
            stream[j].state0 = states0[j].pod.ctypes.data
        totals = np.zeros(2, np.int64)
        last_pod = lii.State()

        def native(first, steps, profile_every):
            rc = drv.lii_stream_run(reg.h, C.byref(stream), len(dev_scans), first, steps,
                                    0.0 if args.no_downsample else float(wl["fs_surf"]), int(wl["max_it"]), 1,
                                    int(bool(args.map_update)), int(profile_every), totals.ctypes.data, last_pod.pod.ctypes.data)
            if rc != 0:
                raise SystemExit(f"lii_stream_run: status {rc}: {reg.L.lii_last_error(reg.h).decode()}")

    # The ROCm runtime grows internal pools (signals / staging) once, ~100 steps into a process: a single 30-50 ms
    # stall at a fixed step index.  Prime it out before the W warm-up steps so that it cannot land in the timed region.
    trace = os.environ.get("LII_BENCH_TRACE")
    stamps = []

    def timed_region(prime, n_steps=None, n_warmup=None):
        """W warm-up steps (+ the priming steps the first time), then EXACTLY K timed steps between barrier + synchronize on both
        sides; the MAX over ranks.  Returns seconds.  (n_steps / n_warmup: another region than the command line's, `value_long`)"""
        nonlocal last
        n_steps = args.steps if n_steps is None else n_steps
        n_warmup = args.warmup if n_warmup is None else n_warmup
        # (a cyclic garbage collection of the interpreter - ~1 ms over this process's objects - is kept out of the timed region: it
        # is triggered by allocation counts, i.e. lands at a fixed point of the script, and round 4's found it inside a 20-step region;
        # it stays off for the rest of the run - the separately timed pipeline figures included.  Collected BEFORE the warm-up steps:
        # between them and the timed ones the device must not sit idle for a millisecond - it would start the region from a lower clock)
        gc.collect()
        gc.disable()
        if native:
            native(0, prime + n_warmup, 0)
        else:
            for k in range(prime + n_warmup):
                step(k)
        reg.synchronize()
        reg.set_profiling(1)
        reg.set_profiling(0)
        iters_total[0] = search_total[0] = 0
        if dist is not None:
            dist.barrier()
        if native:
            totals[:] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        # The k-NN launches of every 8th step of the timed region carry HIP events (inside their dispatch; lii_set_profiling(h, 2)).
        # Between the two brackets of the region there is the host loop and nothing else: the interpreter's bookkeeping (the slowest
        # step, the totals) waits until the clock has been read (round 5 did it between the loop and the synchronisation: ~40 us
        # of Python inside a 3 ms region).
        if native:
            native(0, n_steps, args.profile_every)
            t_native = time.perf_counter() - t0
        else:
            for k in range(n_steps):
                reg.set_profiling(2 if (args.profile_every and k % args.profile_every == 0) else 0)
                last = step(k)
                if trace:
                    stamps.append(time.perf_counter() - t0)
        # (the closing bracket is the contract's: a device-wide synchronise - it covers the library's stream like every other - and the
        # barrier; the library's own lii_synchronize, which also settles a map update in flight, follows behind the clock)
        torch.cuda.synchronize()
        t_libsync = time.perf_counter() - t0
        if dist is not None:
            dist.barrier()
        dt = time.perf_counter() - t0
        reg.synchronize()
        if native:
            if hasattr(drv, "lii_stream_last_slowest"):
                sl = np.zeros(3)
                drv.lii_stream_last_slowest(C.c_void_p(sl.ctypes.data))
                slowest_step.update(ms=sl[0] / 1e3, index=int(sl[1]), second_ms=sl[2] / 1e3)
            iters_total[0], search_total[0] = int(totals[0]), int(totals[1])
            last = last_pod
        if os.environ.get("LII_BENCH_DEBUG"):
            t_a = time.perf_counter(); torch.cuda.synchronize(); t_b = time.perf_counter()
            print(f"[bench debug] a second device synchronize right behind: {1e3 * (t_b - t_a):.3f} ms", file=sys.stderr)
            print(f"[bench debug] timed region: host loop {1e3 * (t_native if native else 0):.3f} ms, + device synchronize {1e3 * t_libsync:.3f}, "
                  f"+ barrier {1e3 * dt:.3f}", file=sys.stderr)
        if dist is not None:
            tmax = torch.tensor([dt], dtype=torch.float64, device="cpu" if one_device else "cuda")
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dt = float(tmax.item())
        return dt

    last = None
    slowest_step = {}  # of the most recent timed region (host clock per step, C++ host loop only)
    transports = None
    if world > 1:
        # A sharded job is timed once per transport of the 91-scalar exchange, same steps, same scans: `default_transport` gives
        # `value` (RCCL on distinct devices: ncclAllReduce between a separate final-sum and solve launch); the library's own
        # node-local choice ("auto": the peer-mapped HBM mailbox - a push over xGMI inside the reduce+solve launch) and the host
        # mailbox are timed beside it - on one device only the mailbox forms can run.  LII_BENCH_TRANSPORT pins `value` to one of them.
        first = default_transport
        others = [t for t in (["mailbox_host"] if one_device else ["rccl", "auto", "mailbox_host"]) if t != first]
        transports = dict(attach_errors)
        dt = None
        primed = False
        for n_run, t in enumerate([first] + others):
            if dt is not None and not args.full:  # (a plain run: the transport that carries `value` only)
                break
            try:
                if n_run > 0:
                    attach(t)
                d = timed_region(0 if primed else args.prime)
                primed = True
            except Exception as e:  # a transport that cannot be set up or run here is reported; the next one carries `value`
                transports[t] = {"error": str(e)[:200]}
                continue
            used = reg.comm_transport()
            transports[used if dt is None else t] = {"value": args.steps / d, "ms_per_step": 1e3 * d / args.steps, "transport": used,
                                                     "rccl_ranks": reg.comm_rccl_ranks(), "avg_iterations": iters_total[0] / args.steps,
                                                     "describe": reg.comm_describe()}
            if dt is None:  # the first transport that ran carries `value` (RCCL on distinct devices unless it failed: see transports)
                dt, value_transport, value_rccl_ranks, first = d, used, reg.comm_rccl_ranks(), t
                last_state_value = np.array(last.pod) if last is not None else None
        if dt is None:
            raise SystemExit(f"no transport of the 91-scalar exchange ran: {transports}")
        # ... and once more on the first transport with the OTHER split of the cloud
        partitions = None
        if args.full:
            partitions = {args.partition: {"value": args.steps / dt, "ms_per_step": 1e3 * dt / args.steps, "describe": transports[value_transport].get("describe")}}
            other = "voxel" if args.partition == "index" else "index"
            try:
                if os.environ.get("LII_BENCH_ONE_PARTITION") == "1":
                    raise RuntimeError("not timed (LII_BENCH_ONE_PARTITION=1)")
                partition_now[0] = other
                attach(first)
                d = timed_region(0)
                partitions[other] = {"value": args.steps / d, "ms_per_step": 1e3 * d / args.steps, "describe": reg.comm_describe(),
                                     "avg_iterations": iters_total[0] / args.steps}
            except Exception as e:
                partitions[other] = {"error": str(e)[:200]}
            partition_now[0] = args.partition
            attach(first)  # the rest of the run (parity calls) on the transport and split `value` was measured with
    else:
        dt = timed_region(args.prime)
        value_transport, value_rccl_ranks = "none", 0
        last_state_value = np.array(last.pod) if last is not None else None
    last_pose_value = last_state_value[:12] if last_state_value is not None else None
    tm = reg.timings()
    iters_value, searches_value = iters_total[0], search_total[0]
    slowest_value = dict(slowest_step)
    # The driver's form of this command times 20 steps (~3 ms): a second, longer region of the same steps right behind it gives the
    # line a figure to check `value` against (never `value` itself).
    value_long = None
    if args.full and args.long_steps > 0 and args.long_steps > args.steps:
        dt_long = timed_region(0, n_steps=args.long_steps, n_warmup=0)
        value_long = {"value": args.long_steps / dt_long, "ms_per_step": 1e3 * dt_long / args.long_steps, "steps": args.long_steps,
                      "what": "the same steps, timed the same way (barrier + synchronize on both sides), right behind the region of `value`"}
    # Where the scan's time goes: a third pass with an event in front of EVERY launch (lii_set_profiling(h, 3); each event is a
    # barrier packet, so this pass is slower than the timed ones and is only used for the SHARES and per-launch durations).
    kernel_profile = None
    if args.full and world == 1 and args.kernel_profile_steps > 0 and not (args.separate_calls or args.upload):
        reg.set_profiling(1)
        if native:
            native(0, args.kernel_profile_steps, -1)
        else:
            for k in range(args.kernel_profile_steps):
                reg.set_profiling(3)
                step(k)
        reg.synchronize()
        kernel_profile = reg.kernel_profile()
        reg.set_profiling(0)
    iters_total[0], search_total[0] = iters_value, searches_value
    # size of the down-sampled cloud (the k-NN kernel's query count) and, on one GPU, the final state of every distinct scan
    # for the parity record: one untimed call per distinct scan, on every rank (a sharded call needs all of them)
    n_ds, gpu_results, n_short = [], [], []
    for j in range(len(dev_scans) if args.full else 0):
        st = states0[j].copy()
        rep = reg.scan_register(st, states0[j], imu_poses=tables[j], leaf=0.0 if args.no_downsample else wl["fs_surf"],
                                max_iterations=wl["max_it"], imu_en=True, scan_dev=dev_scans[j], scan_sorted=True)
        n_ds.append(len(reg.scan_download(1)))
        gpu_results.append((st.pod.copy(), rep))
        if args.edge and world == 1:
            n_short.append((int((reg.neighbors(n_ds[-1])[1] < 5).sum()), reg.last_unfinished_queries()))
    # the GPU's neighbour lists of the first scan at its start state (one host-driven search pass, the map as timed): compared
    # with the unmodified reference ikd-Tree in the cpu_baseline leg
    gpu_lists = None
    if args.full and world == 1 and not args.no_cpu_baseline:
        s0 = states0[0]
        reg.scan_set_device(dev_scans[0])
        reg.undistort_imu(tables[0], s0.rot_end, s0.pos_end, s0.offset_R_L_I, s0.offset_T_L_I)
        nq = reg.downsample(wl["fs_surf"])[0] if not args.no_downsample else reg.downsample_skip()
        reg.iekf_iterate(s0, True, True)
        nb, cnt, _ = reg.neighbors(nq)
        gpu_lists = (nb, cnt)
    if trace and rank == 0:
        np.savetxt(trace, np.diff(np.r_[0.0, stamps]) * 1e3, fmt="%.4f")

    # The COMPLETE per-scan pipeline as a second, separately timed figure (never `value`): every scan handed over from HOST
    # memory (lii_scan_upload: PCIe inside the region), registered, and inserted into the map (lii_map_incremental: device-side
    # Add_Points semantics + index update), so the map grows as in a live run.  Measured last: it changes the map.
    pipeline = None
    if args.full and world == 1 and not args.no_pipeline:
        n_pipe = max(10, min(args.steps, 120))
        leaf = 0.0 if args.no_downsample else float(wl["fs_surf"])

        def python_pipeline():
            reg.synchronize()
            tp0 = time.perf_counter()
            for k in range(n_pipe):
                j = k % len(host_scans)
                reg.scan_upload(host_scans[j])
                st = states0[j].copy()
                reg.scan_register(st, states0[j], imu_poses=tables[j], leaf=leaf, max_iterations=wl["max_it"], imu_en=True, scan_sorted=True)
                reg.map_incremental(st)
            reg.synchronize()
            return time.perf_counter() - tp0

        if native is not None:
            # the C++ host loop again (harness/stream_driver.cpp: lii_stream_run_pipeline).  Three forms of the hand-over:
            # overlapped out of pinned host memory (the copy engine reads the caller's buffer while the previous scan registers),
            # overlapped out of pageable memory (the library stages the scan first), and the serial lii_scan_upload.
            drv.lii_stream_run_pipeline.restype = C.c_int
            drv.lii_stream_run_pipeline.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_void_p]
            pinned = [torch.from_numpy(h).pin_memory() for h in host_scans]

            def run_pipe(ptrs, overlap, steps=n_pipe):
                arr = (C.c_void_p * len(ptrs))(*ptrs)
                tot = np.zeros(2, np.int64)
                reg.synchronize()
                tp0 = time.perf_counter()
                rc = drv.lii_stream_run_pipeline(reg.h, C.byref(stream), arr, len(ptrs), steps, leaf, int(wl["max_it"]), 1,
                                                 int(overlap), tot.ctypes.data)
                if rc != 0:
                    raise SystemExit(f"lii_stream_run_pipeline: status {rc}: {reg.L.lii_last_error(reg.h).decode()}")
                return time.perf_counter() - tp0

            # the first pass over the stream is the one that GROWS the map (afterwards the cyclic stream only replaces points):
            # it is timed on its own, the three forms of the hand-over are then compared on the same (settled) map
            reg.scan_upload_next(pinned[0].numpy())  # one-time set-up of the second buffer / copy stream, outside the timing
            reg.scan_advance()
            tp_first = run_pipe([p.data_ptr() for p in pinned], 1, len(host_scans))
            tp_serial = run_pipe([h.ctypes.data for h in host_scans], 0)
            tp_pageable = run_pipe([h.ctypes.data for h in host_scans], 1)
            tp = run_pipe([p.data_ptr() for p in pinned], 1)
            pipeline = {"value": n_pipe / tp, "unit": "scans/s", "ms_per_scan": 1e3 * tp / n_pipe, "steps": n_pipe,
                        "first_pass_growing_map": {"value": len(host_scans) / tp_first, "ms_per_scan": 1e3 * tp_first / len(host_scans),
                                                   "steps": len(host_scans)},
                        "what": "every scan out of HOST memory: lii_scan_upload_next (pinned source, copy stream, overlapping the "
                                "previous scan) + lii_scan_register + lii_map_incremental + lii_scan_advance per step, C++ host loop, "
                                "separately timed",
                        "pageable_source": {"value": n_pipe / tp_pageable, "ms_per_scan": 1e3 * tp_pageable / n_pipe},
                        "serial_upload": {"value": n_pipe / tp_serial, "ms_per_scan": 1e3 * tp_serial / n_pipe},
                        "map_points_after": reg.map_size()}
            if hasattr(drv, "lii_stream_run_wire") and not args.no_downsample:
                try:
                    pipeline["from_wire"] = from_wire_record(args, wl, reg, drv, stream, len(dev_scans), n_pipe)
                except Exception as e:  # reported, never fatal for the line
                    pipeline["from_wire"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        else:
            tp = python_pipeline()
            pipeline = {"value": n_pipe / tp, "unit": "scans/s", "ms_per_scan": 1e3 * tp / n_pipe, "steps": n_pipe,
                        "what": "H2D upload of the scan + lii_scan_register + lii_map_incremental per step (Python host loop), separately timed",
                        "map_points_after": reg.map_size()}

    if rank == 0:
        scans_per_s = args.steps / dt
        M = len(wl["map"])
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, last_state_value)
    if rank == 0 and args.full:
        n_d = float(np.mean(n_ds)) / world
        n_search = max(tm[5], 1.0)
        avg_search_ms = tm[7] / n_search      # the k-NN kernel alone (dominant kernel)
        # algorithmic bytes of one k-NN launch: read query 16 B + write 5 neighbours 80 B per point,
        # the map once (16 B per map point)
        alg_bytes = 96.0 * n_d + 16.0 * M
        achieved = alg_bytes / (avg_search_ms * 1e-3) / 1e9 if avg_search_ms > 0 else 0.0
        # HBM traffic of the dominant kernel per launch: PMC counters cannot be read inside this process - a single-rank line measures
        # them NOW with two rocprofv3 passes around a short run of this command in a child process (measure_traffic_live); otherwise, or
        # when that fails, the figure comes from the committed passes (tools/collect_pmc.sh) and is labelled as such
        traffic, traffic_source = None, None
        live_note = None
        if world == 1 and not args.no_live_traffic and not (args.separate_calls or args.upload or args.python_loop):
            traffic, traffic_source = measure_traffic_live(args)
            if traffic is None:
                live_note, traffic_source = traffic_source, None
        for prof_name in ("r05_pmc_knn.json", "r04_pmc_knn.json"):  # (r04: the per-lane search kernel of round 4 - only until round 5's passes are committed)
            try:
                prof = json.load(open(os.path.join(ROOT, "profiles", prof_name)))
                if traffic is None and prof.get("workload") == args.workload:
                    traffic, traffic_source = prof["hbm_bytes_per_launch"], ("profiles/" + prof_name + " (rocprofv3 --pmc passes of this command; not measured in this run"
                                                                             + (": " + live_note if live_note else "") + ")")
                    break
            except Exception:
                pass
    if rank == 0:
        out = {
            "metric": "ICP+ESKF scans/sec @100k pts/scan", "value": scans_per_s, "unit": "scans/s",
            "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": f"{args.workload}: {n_full} pts/scan (time-sorted) vs {M}-pt local map, max_iteration {wl['max_it']}, "
                                   f"LIO mode (12-col H), {'map_incremental every step' if args.map_update else 'static map'}, "
                                   f"{'voxel-grid leaf %.2f' % wl['fs_surf'] if not args.no_downsample else 'no voxel-grid'}; "
                                   f"{'every scan handed over from host memory (PCIe inside the timed region)' if args.upload else 'scans resident in HBM'}, "
                                   f"{len(dev_scans)} distinct scans cycled, the state reset to the scan's propagated state every step",
                       "points_per_scan": n_full, "map_points": M,
                       "params": f"harness/launch/{WORKLOADS[args.workload][2]} (reference-format yaml + launch)",
                       "avg_iterations": iters_total[0] / args.steps,
                       "avg_knn_passes": search_total[0] / args.steps,
                       "host_loop": "C++ (harness/stream_driver.cpp)" if native else "Python (ctypes)", "parallelism": f"points sharded x{world}" + (f", 91-scalar exchange over {value_transport}"
                                                                    + (f" (ncclCommCount {value_rccl_ranks})" if value_rccl_ranks else "") if world > 1 else ""),
                       "transport": value_transport, "rccl_ranks": value_rccl_ranks},
        }
        if args.full:
            out["config"]["downsampled_points"] = float(np.mean(n_ds))
            out["roofline"] = {"bound": "hbm", "kernel": knn_kernel_name(),
                               "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                               "traffic": traffic, "traffic_source": traffic_source, "avg_launch_ms": avg_search_ms, "alg_bytes_per_launch": alg_bytes,
                               "launches": int(tm[5]),
                               "peak_measured_copy": 6290.0, "frac_of_measured_copy": achieved / 6290.0}
        if args.edge:
            out["config"]["workload"] = out["config"]["workload"].replace(args.workload + ":", args.workload + "_edge:", 1)
        if args.edge and args.full:
            out["edge"] = {"patch_missing_from_the_map_m": EDGE_PATCH_WIDE if args.edge == "wide" else EDGE_PATCH,
                           "queries_with_fewer_than_5_neighbours_per_scan": [a for a, _ in n_short],
                           "queries_left_unfinished_by_the_last_search_pass_per_scan": [b for _, b in n_short],
                           "what": "every scan of the stream looks past the edge of the map (never `value` of the headline line)"}
        if value_long is not None:
            out["value_long"] = value_long
        if slowest_value:  # a one-off stall of the runtime inside the region shows here (and in value vs value_long), not in the kernels
            out["slowest_step"] = dict(slowest_value, what="longest and second-longest step of `value`'s region on the host clock (call to return; "
                                       "steps with event brackets - every --profile-every-th - are the usual holders)")
        if last_pose_value is not None:  # final pose of the last step of `value`'s region (rot_end row-major, pos_end): a sharded job must land where one rank does
            out["last_state_pose"] = [float(v) for v in last_pose_value]
        if world > 1:
            out["config"]["transport_why"] = reg.comm_describe()
    if rank == 0 and args.full:
        # bytes(scan) = 32 N + S (96 N_d + 16 M) + I (32 N_d + 728), achieved = bytes(scan) x scans/s
        I_avg, S_avg = iters_value / args.steps, searches_value / args.steps
        n_in = float(n_full) / 1.0
        bytes_scan = 32.0 * n_in + S_avg * (96.0 * n_d + 16.0 * M) + I_avg * (32.0 * n_d + 728.0)
        ach_scan = bytes_scan * scans_per_s / 1e9
        out["roofline"]["scan"] = {"alg_bytes": bytes_scan, "achieved": ach_scan, "unit": "GB/s", "frac": ach_scan / HBM_PEAK_GBS,
                                   "frac_of_measured_copy": ach_scan / 6290.0,
                                   "formula": "SURVEY.md 8(d): 32 N + S (96 N_d + 16 M) + I (32 N_d + 728) bytes per scan x scans/s "
                                              f"(N {int(n_in)}, N_d {n_d:.0f}, M {M}, S {S_avg:.2f}, I {I_avg:.2f}; per GPU of a sharded job: N_d / ranks)"}
        if kernel_profile is not None:
            kp, kp_scans = kernel_profile
            nb_fit = (n_d + 255) // 256
            # algorithmic bytes of ONE launch of each kind (the corresponding term of the scan formula where it has one)
            alg = {"deskew": 32.0 * n_in, "voxel": 16.0 * n_in + 16.0 * n_d, "knn": 96.0 * n_d + 16.0 * M, "fit_search": 128.0 * n_d + 728.0,
                   "fit": 48.0 * n_d + 728.0, "solve": 728.0 * nb_fit + 5632.0}
            names = {"deskew": "k_deskew_imu (adoption + IMU back-propagation + voxel-hash insert)", "voxel": "k_vhash_emit (voxel centroids)",
                     "knn": "k_knn_ck", "fit_search": "k_fit_reduce behind a k-NN pass (completion + plane fit + row + sums)",
                     "fit": "k_fit_reduce on cached planes", "solve": "k_reduce_solve (final sum + 24-state solve)"}
            tot_ms = sum(v[0] for v in kp.values()) or 1.0
            rows = []
            for k in ("deskew", "voxel", "knn", "fit_search", "fit", "solve"):
                ms, n_l = kp[k]
                if n_l == 0:
                    continue
                avg_us = 1e3 * ms / n_l
                rows.append({"name": names[k], "kind": k, "launches_per_scan": n_l / max(kp_scans, 1), "avg_us": avg_us,
                             "share_of_scan": ms / tot_ms, "alg_bytes": alg[k], "achieved_GBs": alg[k] / (avg_us * 1e-6) / 1e9,
                             "frac": alg[k] / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS})
            out["roofline"]["kernels"] = rows
            out["roofline"]["kernels_note"] = (f"HIP events in front of every launch over {kp_scans} extra scans (lii_set_profiling(h, 3)): event-to-event "
                                               "time = kernel + dispatch, in a pass that runs slower than the timed region (every event is a barrier "
                                               f"packet: {1e3 * tot_ms / max(kp_scans, 1):.1f} us per scan here against ms_per_step); rocprofv3 durations of the same "
                                               "kernels: profiles/r05_timeline.md")
    if rank == 0:
        if transports is not None:
            out["transports"] = transports
            if partitions is not None:
                out["partitions"] = partitions
            out["config"]["partition"] = args.partition
        if pipeline is not None:
            out["complete_pipeline"] = pipeline
        if args.full and not args.no_cpu_baseline and args.gpus == 1:
            out["cpu_baseline"], out["parity"] = cpu_baseline(wl, states0, tables, args.no_downsample, gpu_results, gpu_lists)
        if args.full and args.gpus == 1 and not args.no_calibration:
            # the metric's second half: calibration outputs of the GPU path against the oracle, the reference's result file and
            # ground truth (harness/calibration_bench.py)
            try:
                from harness import calibration_bench
                out["calibration"] = calibration_bench.calibration_record(lii, reg, synthetic=not args.no_calibration_stream)
            except Exception as e:  # reported, never fatal for the throughput line
                out["calibration"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        print(json.dumps(out), flush=True)
    reg.close()
    if dist is not None:
        dist.destroy_process_group()


STATE_FIELDS = ("rot_end", "pos_end", "offset_R_L_I", "offset_T_L_I", "vel_end", "bias_g", "bias_a", "gravity", "cov")


def dump_outputs(directory, state_pod):
    """--dump-outputs: the final lii_state of the last timed step - what lii_scan_register hands its caller - one float64 array per
    field of lidar_imu_init_amd.State (the inputs are seeded: the same arguments give the same scans, map and start states)."""
    import lidar_imu_init_amd as lii
    os.makedirs(directory, exist_ok=True)
    st = lii.State(state_pod)
    for name in STATE_FIELDS:
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(getattr(st, name), np.float64))


def from_wire_record(args, wl, reg, drv, stream, n_stream, n_pipe):
    """complete_pipeline.from_wire: driver messages in, poses out.  Every sweep of the workload packed as sensor_msgs/PointCloud2 bytes
    in the Ouster driver's layout (harness/wire.py: 48-byte records, time as uint32 nanoseconds) -> lii_ingest_pcl2 (H2D of the raw
    bytes, decode, blind / ring filters, time sort, cut into `cut_frame_num` sub-frames: src/preprocess.cpp:115-335) -> per sub-frame
    lii_frame_select + lii_scan_register with the map update in the job (src/laserMapping.cpp:326-379, 909-1134, 516-559), C++ host
    loop (harness/stream_driver.cpp: lii_stream_run_wire).  Never `value`."""
    import ctypes as C
    from harness import wire
    from lidar_imu_init_amd.api import lii_ingest_opts, lii_pc2_fields
    cut = int(wl["cut"])
    prm = wl["params"]
    msgs = []
    for k, sw in enumerate(wl["sweeps"]):
        raw = wire.pack_pcl2(wire.OUSTER, sw[:, :3], (np.arange(len(sw)) % 128).astype(np.int32), sw[:, 3].astype(np.float64), 0.1 * k)
        msgs.append(np.frombuffer(raw, np.uint8).copy())
    n_msgs = max(1, n_stream // cut)  # whole messages whose sub-frames the stream's states cover
    msgs = msgs[:n_msgs]
    ptrs = (C.c_void_p * n_msgs)(*[m.ctypes.data for m in msgs])
    npts = np.array([len(sw) for sw in wl["sweeps"][:n_msgs]], np.int32)
    fields = lii_pc2_fields(*wire.pc2_fields(wire.OUSTER))
    opts = lii_ingest_opts()
    opts.struct_size = C.sizeof(lii_ingest_opts)
    opts.lidar_type, opts.n_scans, opts.point_filter_num = wire.OUSTER, 128, 1
    opts.blind, opts.stamp_s, opts.cut_frame_num, opts.scan_count = 0.01, 0.0, cut, 1000  # (past the first 20 messages, which the reference does not cut)
    if os.environ.get("LII_WIRE_WHOLE") == "1" and cut == 1:  # (measurement: Preprocess::process - no time sort, 5 launches instead of 16)
        opts.cut_frame_num = 0
    drv.lii_stream_run_wire.restype = C.c_int
    drv.lii_stream_run_wire.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]

    import torch
    pinned_msgs = [torch.from_numpy(m).pin_memory() for m in msgs]
    ptrs_pinned = (C.c_void_p * n_msgs)(*[t.data_ptr() for t in pinned_msgs])
    drv.lii_stream_set_wire_overlap.argtypes = [C.c_int32]
    drv.lii_stream_set_wire_overlap.restype = None

    def run(steps, map_update, overlap=0, src=ptrs):
        tot = np.zeros(2, np.int64)
        ing = np.zeros(2)
        drv.lii_stream_set_wire_overlap(int(overlap))
        reg.synchronize()
        t0 = time.perf_counter()
        rc = drv.lii_stream_run_wire(reg.h, C.byref(stream), n_stream, src, npts.ctypes.data, n_msgs, steps, C.byref(fields), C.byref(opts),
                                     float(wl["fs_surf"]), int(wl["max_it"]), 1, int(map_update), tot.ctypes.data, ing.ctypes.data)
        dt = time.perf_counter() - t0
        drv.lii_stream_set_wire_overlap(0)
        if rc != 0:
            raise RuntimeError(f"lii_stream_run_wire: status {rc}: {reg.L.lii_last_error(reg.h).decode()}")
        return dt, ing, tot

    def record(dt, ing, tot, n_m):
        frames = int(ing[1])
        return {"value": frames / dt, "unit": "scans/s", "ms_per_scan": 1e3 * dt / max(frames, 1), "messages": n_m, "sub_frames": frames,
                "ingest_us_per_message": float(ing[0]) / n_m, "ingest_share_of_the_loop": float(ing[0]) * 1e-6 / dt,
                "avg_iterations": float(tot[0]) / max(frames, 1)}

    n_m = max(4, n_pipe // cut)
    if os.environ.get("LII_BENCH_WIRE_STEPS"):  # (soak: this many messages per form)
        n_m = max(4, int(os.environ["LII_BENCH_WIRE_STEPS"]))
    run(min(n_m, 2 * n_msgs), True)  # (untimed: first-time allocations of the ingest)
    run(min(n_m, 2 * n_msgs), True, 1, ptrs_pinned)  # (... and of the overlapped form's ring)
    over_pageable = record(*run(n_m, True, 1, ptrs), n_m)
    over = record(*run(n_m, True, 1, ptrs_pinned), n_m)
    over_early = record(*run(n_m, True, 3, ptrs_pinned), n_m)
    over_behind = record(*run(n_m, True, 4, ptrs_pinned), n_m)
    serial = record(*run(n_m, True), n_m)  # (last: tools/wire_timeline.py reads the launches of one message off the end of a trace)
    out = dict(over)
    out.update({"cut_frame_num": cut, "points_per_message": int(npts[0]), "bytes_per_message": int(len(msgs[0])),
                "what": "PointCloud2 bytes (Ouster layout, page-locked host memory) -> lii_ingest_pcl2_begin ... lii_ingest_end (ABI 9: message "
                        "m + 1 is decoded and the bytes of m + 2 travel on streams of their own while message m is registered) -> lii_frame_select "
                        "-> lii_scan_register with map_update = 1 per sub-frame, C++ host loop; the next message is begun from the registration's "
                        "while_waiting hook (lii_scan_job::while_waiting: inside the call, when its launches are out); ingest_us_per_message = host "
                        "time inside lii_ingest_end (the begin's time lies inside lii_scan_register)",
                "pageable_source": over_pageable,
                "begun_before_the_registrations": over_early,
                "begun_behind_the_registrations": over_behind,
                "serial_ingest": dict(serial, what="one lii_ingest_pcl2 call per message on the handle's own stream (pageable source): H2D of "
                                                   "the raw bytes, its launches and its one synchronisation before the first sub-frame is registered "
                                                   "(the form of the record until ABI 8)"),
                "map_points_after": reg.map_size()})
    return out


def cpu_sweep_worker(args):
    """The oracle's step on 3 / 8 / 32 / 64 OpenMP threads, ~3 s each; prints one JSON object {threads: scans/s}.  Started by
    cpu_baseline with OMP_PROC_BIND=close OMP_PLACES=cores; touches no GPU."""
    from oracle import oracle as O
    wl = build_workload(args.workload, 2, edge=args.edge)
    states0, tables = start_states(wl)
    tree = O.Tree("oracle")
    tree.build(wl["map"])
    leaf = 0.0 if args.no_downsample else wl["fs_surf"]
    out = {}
    for th in (3, 8, 32, 64):
        if th > O.num_procs():
            break
        secs, n = 0.0, 0
        while secs < 3.0 and n < 64:
            j = n % len(wl["scans"])
            t0 = time.perf_counter()
            oracle_scan_register(O, tree, wl["scans"][j], states0[j], tables[j], leaf, wl["max_it"], th)
            secs += time.perf_counter() - t0
            n += 1
        out[str(th)] = n / secs
    print(json.dumps(out), flush=True)


def knn_kernel_name():
    return ("k_knn_ck (exact 5-NN into the block-grid local map, 4 lanes/query scanning every cell together, packed 32-bit keys in both "
            "rounds, winners re-measured exactly)")


def measure_traffic_live(args):
    """HBM bytes per executed launch of the dominant kernel, MEASURED NOW: two `rocprofv3 --pmc <counter> --kernel-trace` passes (FETCH_SIZE,
    WRITE_SIZE - one counter set per pass, no sys / hip / hsa trace domain beside them: MI355X_MICROARCH.md) around a short run of THIS
    command in a child process; per dispatch of k_knn_ck the counter summed over its rows, executed launches = those above a fifth of the
    largest (the device-driven loop enqueues launches that find their pass not due and move nothing); FETCH_SIZE / WRITE_SIZE are in KB and
    gfx950 reports half of the fetched bytes, so the read side is doubled (the guide's correction; tools/summarize_pmc.py does the same on
    the committed passes).  Returns (bytes per launch, description) or (None, why not)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    if os.environ.get("LII_BENCH_CHILD") or any(k.startswith("ROCPROF") for k in os.environ):
        return None, "this process already runs under a profiler"
    tmp = tempfile.mkdtemp(prefix="lii_pmc_", dir="/tmp")
    res = {}
    try:
        for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
            cmd = [exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", os.path.join(tmp, ctr), "-o", "pmc", "--",
                   sys.executable, os.path.abspath(__file__), "--full", "--workload", args.workload, "--steps", "8", "--warmup", "2", "--prime", "0",
                   "--profile-every", "0", "--no-cpu-baseline", "--no-pipeline", "--no-calibration", "--kernel-profile-steps", "0",
                   "--long-steps", "0", "--no-live-traffic"] + (["--no-downsample"] if args.no_downsample else []) + (["--edge-wide"] if args.edge == "wide" else (["--edge"] if args.edge else []))
            subprocess.run(cmd, env={**os.environ, "TMPDIR": "/tmp", "LII_BENCH_CHILD": "1"}, cwd="/tmp", timeout=150,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            per = {}
            for f in glob.glob(os.path.join(tmp, ctr, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if "k_knn_ck" in r["Kernel_Name"] and r["Counter_Name"] == ctr:
                        per[(f, r["Dispatch_Id"])] = per.get((f, r["Dispatch_Id"]), 0.0) + float(r["Counter_Value"])
            vals = sorted(per.values())
            big = [v for v in vals if v > 0.2 * vals[-1]] if vals else []
            if not big:
                return None, f"no {ctr} rows for the search kernel"
            res[ctr] = (sum(big) / len(big), len(big))
    except Exception as e:  # a profiler that cannot run here must not cost the line
        return None, f"{type(e).__name__}: {str(e)[:120]}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    fetch_kb, write_kb = res["FETCH_SIZE"][0], res["WRITE_SIZE"][0]
    return (2.0 * fetch_kb + write_kb) * 1024.0, (
        f"measured in this run: rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (one pass each, --kernel-trace beside it) around "
        f"`bench.py --workload {args.workload} --steps 8` in a child process, mean over {res['FETCH_SIZE'][1]} executed launches; "
        f"(2 x FETCH_SIZE {fetch_kb:.0f} KB + WRITE_SIZE {write_kb:.0f} KB) x 1024 - gfx950 reports half of the fetched bytes (MI355X_MICROARCH.md)")



def cpu_baseline(wl, states0, tables, no_downsample, gpu_results, gpu_lists=None, budget_s=14.0):
    """The oracle restatement of the same step - time sort + IMU back-propagation de-skew, voxel grid, iterated update
    (ikd-Tree-semantics k-NN, per-point QR plane fit, Jacobian, 24-state solve) - on this box's host cores with the
    reference's 3 OpenMP threads for the registration loop (MP_PROC_NUM, CMakeLists.txt:24-27; the de-skew and the voxel
    filter are single-threaded in the reference, as here), plus the same step on 1 thread and on all cores, plus the k-NN
    stage alone through the UNMODIFIED reference ikd-Tree (oracle/_ref) where it was built.  The first pass over the
    distinct scans also yields the parity record: the oracle's final state against the GPU's."""
    from oracle import oracle as O
    tree = O.Tree("oracle")
    tree.build(wl["map"])
    leaf = 0.0 if no_downsample else wl["fs_surf"]
    ncores = O.num_procs()
    parity = []
    knn_parity = None

    def run(threads, budget, max_scans, keep=False):
        secs, n, reg_secs, best, k = 0.0, 0, 0.0, None, 0
        while secs < budget and n < max_scans:
            j = k % len(wl["scans"])
            t0 = time.perf_counter()
            r = oracle_scan_register(O, tree, wl["scans"][j], states0[j], tables[j], leaf, wl["max_it"], threads)
            dt = time.perf_counter() - t0
            if keep and k < len(gpu_results):
                parity.append(parity_against_oracle(O, r, *gpu_results[j], prior_cov=states0[j].cov))
            secs += dt
            reg_secs += r["seconds"]
            best = dt if best is None else min(best, dt)
            n += 1
            k += 1
        return n / secs, n, secs, reg_secs, best

    v3, n3, s3, r3, b3 = run(3, budget_s, 160, keep=True)
    v1, n1, s1, _, _ = run(1, 4.0, 16)
    # thread sweep in a fresh process with OMP_PROC_BIND=close / OMP_PLACES=cores (libgomp reads them when it is loaded, which
    # torch has long done here): the registration loop is the only threaded stage (as in the reference), so this is its scaling
    sweep = {}
    try:
        import subprocess
        env = dict(os.environ, OMP_PROC_BIND="close", OMP_PLACES="cores")
        outp = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-sweep-worker", "--workload", wl["name"]] +
                              (["--no-downsample"] if no_downsample else []) + (["--edge-wide"] if wl.get("edge") == "wide" else (["--edge"] if wl.get("edge") else [])), env=env, capture_output=True, timeout=120, text=True)
        sweep = json.loads(outp.stdout.strip().splitlines()[-1])
    except Exception as e:
        sweep = {"error": str(e)[:200]}
    extra = ""
    t_ref = t_port = None
    if O.ref_available():  # the k-NN stage through the reference's own tree (3 threads), beside the port's tree
        # (the reference tree prints from its rebuild thread - "Multi thread started" / "Rebuild thread terminated normally": its
        # stdout goes to stderr for as long as it lives, the bench's stdout carries the ONE JSON line only)
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            rt = O.Tree("ref")
            rt.build(wl["map"])
            und = O.undistort_imu(wl["scans"][0], tables[0], states0[0].rot_end, states0[0].pos_end, states0[0].offset_R_L_I,
                                  states0[0].offset_T_L_I)
            body = und if not leaf > 0 else O.voxel_grid(und, leaf)[0]
            R, p = states0[0].rot_end, states0[0].pos_end
            q = (body[:, :3].astype(np.float64) @ R.T + p).astype(np.float32)
            t0 = time.perf_counter(); ref_pts, _, ref_cnt = rt.knn(q, threads=3); t_ref = time.perf_counter() - t0
            if gpu_lists is not None and len(gpu_lists[1]) == len(q):  # the GPU's lists against the reference tree's, every query
                nb, cnt = gpu_lists
                same = (cnt == ref_cnt) & ((ref_cnt < 5) | np.all(nb.reshape(len(q), -1) == ref_pts.reshape(len(q), -1), axis=1))
                knn_parity = {"identical": int(same.sum()), "of": int(len(q)),
                              "what": "5-NN lists of every down-sampled point of the first scan at its start state: GPU (k_knn_ck + "
                                      "completion) vs the UNMODIFIED reference ikd-Tree (oracle/_ref) on the same 1 M-point map"}
            t0 = time.perf_counter(); tree.knn(q, threads=3); t_port = time.perf_counter() - t0
            extra = (f"; k-NN stage alone on {len(q)} queries, 3 threads: unmodified reference ikd-Tree {t_ref * 1e3:.0f} ms, "
                     f"the port's tree {t_port * 1e3:.0f} ms")
            rt.close()
        except Exception as e:  # the reference tree is a checker: never let it break the bench line
            extra = f"; reference-tree timing failed: {e}"
        finally:
            time.sleep(0.3)  # its thread prints on the way out
            import ctypes
            ctypes.CDLL(None).fflush(None)  # ... into the C library's stdio buffer: flush it while fd 1 still points at stderr
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
    base = {"value": v3, "unit": "scans/s", "cores": 3, "kind": "port",
            "threads_1": v1, "threads_sweep_bound_close": sweep, "host_cores": ncores,
            "sample": f"{n3} scans of the same workload and the same step (de-skew + voxel grid + iterated update) on 3 OpenMP threads "
                      f"(the reference's MP_PROC_NUM), {s3:.1f} s CPU wall of which {r3:.1f} s in the registration loop, best scan "
                      f"{b3 * 1e3:.0f} ms; 1 thread: {n1} scans in {s1:.1f} s; threads_sweep_bound_close: the same step with 3 / 8 / 32 / 64 "
                      f"threads pinned to neighbouring cores (OMP_PROC_BIND=close), ~3 s each in a fresh process{extra}"}
    if t_ref is not None and t_port is not None and v3 > 0:
        # the same step with the k-NN stage charged at the UNMODIFIED reference tree's rate instead of the port's (two search
        # passes per scan on this stream): the port's tree is faster than the reference's, so `value` flatters the CPU
        passes = 2.0
        base["with_reference_tree"] = {"value": 1.0 / (1.0 / v3 + passes * (t_ref - t_port)), "unit": "scans/s", "kind": "port+reference_tree",
                                       "what": f"1 / (port step time + {passes:.0f} x (reference-tree k-NN pass {t_ref * 1e3:.0f} ms - port-tree pass "
                                               f"{t_port * 1e3:.0f} ms)), 3 threads"}
    par = None
    if parity:
        par = {"scans_compared": len(parity), "dp_max": max(x["dp"] for x in parity), "dtheta_max": max(x["dtheta"] for x in parity),
               "dp_lidar_max": max(x["dp_lidar"] for x in parity), "dtheta_lidar_max": max(x["dtheta_lidar"] for x in parity),
               "dstate_pose_ext_max": max(x["dstate_pose_ext"] for x in parity), "dstate_rest_max": max(x["dstate_rest"] for x in parity),
               "dcov_rel_max": max(x["dcov_rel"] for x in parity),
               "dcov_gpu_vs_exact_max": max(x["dcov_gpu_exact"] for x in parity), "dcov_oracle_vs_exact_max": max(x["dcov_oracle_exact"] for x in parity),
               "dcov_gpu_vs_oracle_max": max(x["dcov_gpu_oracle"] for x in parity),
               "dcov_note": "posterior covariance element-wise relative to sqrt(P_ii P_jj), against the exact (60-digit) posterior "
                            "(P^-1 + H^T R^-1 H)^-1 of the same normal equations: the device's elimination is closer to it than the "
                            "reference's two-inversion algebra (the oracle) is",
               "iters_equal": all(x["iters_equal"] for x in parity),
               "searches_equal": all(x["searches_equal"] for x in parity), "effect_num_max_diff": max(x["effect_diff"] for x in parity),
               "tolerance": "dp <= 1e-6 m, dtheta <= 1e-7 rad (tests/test_gpu_headline_parity.py)",
               "against": "oracle/ (CPU restatement of src/laserMapping.cpp:909-1134) on the same scans, map and start states"}
        if knn_parity is not None:
            par["knn_vs_reference_tree"] = knn_parity
    return base, par


if __name__ == "__main__":
    main()

"""lii_pose_score and the communicator, and the order of its `res` rows behind a real voxel filter.

  * a communicator of MORE than one rank: both forms refuse with LII_ERR_STATE and write nothing (two ranks on one device over the
    mailbox transport, each a child process: tests/pose_score_rank_worker.py);
  * a communicator of ONE rank (attached as the other suites attach it, over RCCL) does not stand in the way: the same bytes as before;
  * behind lii_downsample the cloud lies on the device in the filter's own order: the host form's rows follow lii_scan_download(1), the
    device form's the device's order - the same values, permuted.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_score_cases as psc
from plane_rows_np import _ulp32  # pd2's allowance: one float32 ulp of the value

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STATE = -5  # LII_ERR_STATE


def test_refused_with_two_ranks_attached(tmp_path):
    import lidar_imu_init_amd as lii
    r = lii.Registrar(max_scan_points=1024, max_map_points=1024)
    uid = r.comm_unique_id().hex()
    r.close()
    world, procs, outs = 2, [], []
    for rank in range(world):
        outs.append(str(tmp_path / f"rank{rank}.npz"))
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "pose_score_rank_worker.py"), str(rank), str(world), uid, "mailbox", outs[-1]],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=120)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace"))
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    for o in outs:
        got = dict(np.load(o))
        assert str(got["transport"]) == "mailbox" and int(got["n"]) == 500
        assert (int(got["rc_h"]), int(got["rc_d"])) == (STATE, STATE)
        assert bool(got["host_untouched"]) and bool(got["dev_untouched"])


def test_served_with_a_one_rank_communicator(oracle, small_world):
    import lidar_imu_init_amd as lii
    _, map_pts = small_world
    scan = psc.tiny_scan(small_world)[:2000]
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    reg.scan_upload(scan)
    assert reg.downsample_skip() == len(scan)
    _, _, R, p = psc.parity_poses(small_world)[0]
    base = lii.State(psc.state_at(oracle, R[0], p[0]))
    before = reg.pose_score(base, (R[:5], p[:5]), want_res=True)
    reg.comm_init(1, 0, reg.comm_unique_id(), "rccl")
    with_comm = reg.pose_score(base, (R[:5], p[:5]), want_res=True)
    reg.comm_destroy()
    after = reg.pose_score(base, (R[:5], p[:5]), want_res=True)
    assert before[1][0] > 0.9 * len(scan)
    for got in (with_comm, after):
        assert np.array_equal(got[0], before[0]) and np.array_equal(got[1], before[1])
        assert np.array_equal(got[2].view(np.uint64), before[2].view(np.uint64)) and np.array_equal(got[3].view(np.uint32), before[3].view(np.uint32))
    reg.close()


def test_rows_behind_a_voxel_filter(oracle, small_world):
    """lii_downsample leaves the cloud on the device in the order of the voxels' first points; lii_scan_download(1) hands it out in the
    reference filter's order.  The host form's res rows are held to the oracle's pass over the DOWNLOADED cloud, point by point; the
    device form's row holds the same values in the device's order."""
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd.api import POSE_SCORE_DTYPE, poses_array
    _, map_pts = small_world
    scan = psc.tiny_scan(small_world)
    reg = lii.Registrar(max_scan_points=10_000, max_map_points=400_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    reg.scan_upload(scan)
    n, _ = reg.downsample(0.3)
    body = reg.scan_download(1)
    assert 500 < n < len(scan) and len(body) == n
    Rp, pp = psc.perturbed(False)
    st = psc.state_at(oracle, Rp, pp)
    tree = oracle.Tree("oracle")
    tree.build(map_pts)
    ref = tree.iterate_once(body, st, search=True, imu_en=False, threads=4)
    n_full, eff, tot, res = reg.pose_score(lii.State(st), (Rp[None], pp[None]), want_res=True)
    assert res.shape == (1, n) and n_full[0] == int((ref["nearest_n"] == 5).sum())
    sel, ref_sel = res[0] >= 0, ref["selected"].astype(bool)
    flips = int((sel != ref_sel).sum())
    print(f"{n} points behind the filter: effect {eff[0]} (oracle {int(ref_sel.sum())}), flags that differ {flips}")
    assert flips <= 0.001 * n and eff[0] == int(sel.sum()) > 0.8 * n
    both = sel & ref_sel
    want = np.abs(ref["normvec"][both, 3])
    assert np.all(np.abs(res[0][both].astype(np.float64) - want.astype(np.float64)) <= np.array([_ulp32(v) for v in want]))
    # the device form: the same figures, the row in the device's order - a permutation of the host form's, and not the identity here
    P = poses_array((Rp[None], pp[None]))
    d_P, d_sc, d_res = reg.dev_alloc(P.nbytes), reg.dev_alloc(16), reg.dev_alloc(4 * n)
    reg.dev_upload(d_P, P)
    reg.pose_score_dev(lii.State(st), d_P, 1, d_sc, d_res)
    reg.synchronize()
    hip = C.CDLL(reg.L._name)  # the runtime the library itself uses
    sc, row = np.zeros(1, POSE_SCORE_DTYPE), np.zeros(n, np.float32)
    for o, addr in ((sc, d_sc), (row, d_res)):
        assert hip.hipMemcpy(C.c_void_p(o.ctypes.data), C.c_void_p(int(addr)), C.c_size_t(o.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
    assert (int(sc["n_full"][0]), int(sc["effect_num"][0])) == (int(n_full[0]), int(eff[0]))
    assert np.float64(sc["total_residual"][0]).tobytes() == np.float64(tot[0]).tobytes()
    assert np.array_equal(np.sort(row), np.sort(res[0]))
    assert not np.array_equal(row, res[0]), "the filter kept the reference's order: this cloud does not show the difference"
    reg.close()

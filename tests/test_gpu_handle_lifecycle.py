"""What a handle takes from the device it gives back when it is closed, the buffers, streams and events it creates on first use included.

One cycle: create a handle, build the map, register two scans with the map update inside the call (the map stream), send a scan ahead
from pageable memory (copy stream, the second scan buffer, its pinned staging), put one driver message through the overlapped ingest
(the ring's streams, events and one context), evaluate the calibration residual once (its input buffers), delete a box from the map,
close.  The cycle runs once as warm-up and eight more times in one process; the device memory in use (hipMemGetInfo through
torch.cuda.mem_get_info) is read after every close.

Bound: from the close of cycle 2 to the close of cycle 9 the memory in use grows by no more than ONE scan buffer of the handle,
16 * max_scan_points bytes.  Every array whose size follows the handle's capacities is at least that large, so a single such owner
that is not released would show as eight times the bound.

What this reading cannot see: an allocation smaller than the granule the runtime takes device memory in (the handle's counters,
tickets and flag words: a leak of those passes until enough of them fill a granule), pinned HOST memory (not device memory at all),
and events and streams, which hold no device memory worth the name.  Other work on the same device moves the reading too: it is
printed for every cycle so that a failure can be told from a neighbour."""
import numpy as np
import pytest

from harness import synth, wire

pytestmark = pytest.mark.gpu

MAX_SCAN = 40_000
MAX_MAP = 200_000
CYCLES = 9  # the first one is the warm-up


def _cycle(lii, oracle, map_pts, scan, st_true, msg, cal):
    reg = lii.Registrar(max_scan_points=MAX_SCAN, max_map_points=MAX_MAP, filter_size_map=0.15)
    try:
        reg.map_build(map_pts)
        st0 = oracle.state_boxplus(st_true, np.r_[0.002, -0.002, 0.003, 0.02, -0.02, 0.01, np.zeros(18)])
        for _ in range(2):
            reg.scan_upload(scan)
            s = lii.State(st0)
            rep = reg.scan_register(s, lii.State(st0), leaf=0.1, max_iterations=5, imu_en=False, map_update=True)
            assert rep["effect_num"] > 1000
        reg.map_commit()
        reg.scan_upload_next(scan)  # a plain numpy array: pageable, staged through the handle's second pinned buffer
        reg.scan_advance()
        reg.ingest_pcl2_begin(*msg)
        info = reg.ingest_end()
        assert len(info) >= 1
        reg.calib_set_buffers(*cal)
        JtJ, _, cost = reg.calib_eval(1, np.eye(3).reshape(-1))
        assert np.all(np.isfinite(JtJ)) and np.isfinite(cost)
        lo = map_pts.min(axis=0) - 0.1  # a corner of the hall: floor and two walls
        assert reg.map_delete_boxes(np.r_[lo, lo + 4.0][None, :]) > 0
        assert reg.map_size() > 0
    finally:
        reg.close()


def test_closing_a_handle_returns_its_device_memory(oracle):
    import torch

    import lidar_imu_init_amd as lii
    from conftest import make_state
    hall, map_pts = synth.bench_world(150_000, 0.15)
    R, p = synth.rot_zyx(0.0, 0.01, 0.3), np.array([1.0, 2.0, 0.3])
    scan = synth.make_scan(hall, "vlp16", R, p, noise=0.02, seed=5)
    scan[:, 3] = np.linspace(0, 100, len(scan), dtype=np.float32)
    scan = np.ascontiguousarray(scan, np.float32)
    st_true = make_state(oracle, R, p)
    xyz, ring, t_ms = wire.raw_sweep(hall, "vlp16", R, p, nan_fraction=0.0)
    msg = (wire.pack_pcl2(wire.VELO, xyz, ring, t_ms, 10.0), len(xyz), wire.pc2_fields(wire.VELO), wire.VELO, 16, 1, 0.5, 10.0, 2, 100)
    rng = np.random.default_rng(11)
    cal = (rng.normal(size=(400, 22)), rng.normal(size=(400, 22)))

    used = []
    for k in range(CYCLES):
        _cycle(lii, oracle, map_pts, scan, st_true, msg, cal)
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        used.append(total - free)
        print(f"cycle {k + 1}: device memory in use after close {used[-1]} bytes ({used[-1] - used[0]:+d} against cycle 1)")
    bound = 16 * MAX_SCAN
    growth = used[CYCLES - 1] - used[1]
    print(f"growth from cycle 2 to cycle {CYCLES}: {growth} bytes, bound {bound}")
    assert growth <= bound, (used, bound)

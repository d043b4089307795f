"""One rank of a job that asks for lii_pose_refine with a communicator of `world` ranks attached (run as a subprocess by
tests/test_gpu_pose_refine_ranks.py).

argv: rank world uid_hex transport out.npz
The rank builds a small map, attaches the communicator, loads a cloud (downsample_skip) and calls both forms with outputs filled with a
sentinel.  Saved: the two return codes, whether every output byte is still the sentinel, the transport it ended up with."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    uid, transport, out = bytes.fromhex(sys.argv[3]), sys.argv[4], sys.argv[5]
    import lidar_imu_init_amd as lii
    from lidar_imu_init_amd.api import POSE_REFINED_DTYPE
    from harness import synth

    hall = synth.Hall(size=(8.0, 6.0, 3.0), n_boxes=2, seed=7)
    map_pts = hall.surface_points(0.15, noise=0.01, seed=7)
    scan = synth.make_scan(hall, "tiny", np.eye(3), np.zeros(3), noise=0.02, seed=3)[:500]
    reg = lii.Registrar(max_scan_points=4096, max_map_points=100_000, filter_size_map=0.15)
    reg.map_build(map_pts)
    reg.comm_init(world, rank, uid, transport)
    reg.comm_set_partition(0)  # the caller hands every rank its own points: the cloud below is this rank's, whole
    reg.scan_upload(scan)
    n = reg.downsample_skip()
    K = 5
    P = np.zeros((K, 12))
    P[:, 0] = P[:, 4] = P[:, 8] = 1.0
    P[:, 9] = 0.01 * np.arange(K)
    base = lii.State()
    rec = np.zeros(K, POSE_REFINED_DTYPE)
    rec.view(np.uint8)[:] = 0xA5
    rec0 = rec.copy()
    rc_h = reg.L.lii_pose_refine(reg.h, base.pod.ctypes.data, None, P.ctypes.data, K, 4, 2, rec.ctypes.data)
    host_untouched = bool(np.array_equal(rec.view(np.uint8), rec0.view(np.uint8)))
    d_P, d_rec = reg.dev_alloc(P.nbytes), reg.dev_alloc(rec0.nbytes)
    reg.dev_upload(d_P, P)
    reg.dev_upload(d_rec, rec0)
    rc_d = reg.L.lii_pose_refine_dev(reg.h, base.pod.ctypes.data, None, d_P, K, 4, 2, d_rec)
    reg.synchronize()
    hip = C.CDLL(reg.L._name)  # the runtime the library itself uses
    back = np.zeros_like(rec0)
    assert hip.hipMemcpy(C.c_void_p(back.ctypes.data), C.c_void_p(int(d_rec)), C.c_size_t(back.nbytes), C.c_int(2)) == 0  # hipMemcpyDeviceToHost
    dev_untouched = bool(np.array_equal(back.view(np.uint8), rec0.view(np.uint8)))
    np.savez(out, rc_h=rc_h, rc_d=rc_d, host_untouched=host_untouched, dev_untouched=dev_untouched, n=n, transport=reg.comm_transport())
    reg.close()


if __name__ == "__main__":
    main()

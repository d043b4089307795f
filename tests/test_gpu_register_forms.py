"""The registration call's job reader and scan admission (lii_capi_register.cpp: job_view, claim_staging / admit_scan): what a caller
of an earlier ABI did not fill in is not read, a refused call leaves nothing behind, and lii_scan_job::while_waiting runs exactly once
per call that gets as far as its update.  Every comparison is between two runs of the library that is loaded: np.array_equal on the
final lii_state, plus iterations and effect_num.  Inputs: World of tests/test_gpu_front_end_bits.py (max_scan_points 8 000, scans of 513
and 1 025 points, K = 12, leaf 0.1, three iterations).

Not repeated here: "the hook runs once per lii_scan_register on the device" - tests/test_gpu_ingest_overlap.py asserts it
(test_the_next_message_is_begun_from_inside_the_registration: calls == [0, 1, 2], one per registration that carried a hook).  This
module adds lii_scan_register_imu, lii_scan_register_cv and lii_scan_register under LII_TEST=host_solve."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_front_end_bits import LEAF, MAX_IT, World, _with_env

pytestmark = pytest.mark.gpu

MAX_SCAN = 8_000
SIZES_N = (513, 1025)
T_BEG = 10.0
INVALID, CAPACITY = -1, -4
ENTRIES = ("plain", "imu", "cv")


class Forms:
    """World, a handle with the map built, and the three entry points through raw ctypes (built once per module)."""

    def __init__(self, oracle, small_world):
        from lidar_imu_init_amd import api
        self.w = World(oracle, small_world)
        self.api = api
        self.T12 = np.ascontiguousarray(self.w.table(12), np.float64)
        self.scans = {(n, s): self.w.scan(n, sorted_=s) for n in SIZES_N for s in (True, False)}
        self.cg = np.full(3, 0.01)
        self.ca = np.full(3, 0.01)
        st = self.w.st0
        self.carry0 = dict(last_imu=np.r_[T_BEG - 0.005, np.zeros(3), st.rot_end.T @ -st.gravity], acc_s_last=np.zeros(3), angvel_last=np.zeros(3),
                           last_lidar_end_time=T_BEG)
        self.reg = self.registrar()

    def registrar(self):
        """A handle with the map built and one registration behind it (the first scan of a leaf size is probed for the voxel filter)."""
        reg = self.w.lii.Registrar(max_scan_points=MAX_SCAN, max_map_points=400_000, filter_size_map=0.15)
        reg.map_build(self.w.map_pts)
        reg.set_imu_noise(cov_gyr=0.1, cov_acc=0.1, mean_acc_norm=9.81)
        reg.scan_upload(self.scans[(513, True)])
        st = self.w.st0.copy()
        reg.scan_register(st, self.w.st0, imu_poses=self.T12, leaf=LEAF, max_iterations=MAX_IT, imu_en=True, scan_sorted=True)
        return reg

    def imu_rows(self, pts):
        """A platform at rest: 200 Hz samples up to the sweep's end, the accelerometer reading what cancels the state's gravity."""
        st = self.w.st0
        t = np.arange(T_BEG + 0.005, T_BEG + float(pts[:, 3].max()) / 1000.0 + 1e-9, 0.005)
        return np.ascontiguousarray(np.c_[t, np.tile([1e-3, -2e-3, 1.5e-3], (len(t), 1)), np.tile(st.rot_end.T @ -st.gravity, (len(t), 1))])

    def job(self, entry, size, dev, sorted_=1, **fields):
        """A job as a caller of that ABI leaves it: struct_size `size`, the fields every ABI has, then `fields`."""
        api = self.api
        job = api.lii_scan_job()
        job.struct_size = size
        job.undistort = 2 if entry == "cv" else 1
        if entry == "plain":
            job.imu_poses, job.n_imu_poses = self.T12.ctypes.data, len(self.T12)
        job.leaf = LEAF
        job.opts = api.lii_iekf_opts(MAX_IT, 0 if entry == "cv" else 1)
        job.scan_dev, job.n_scan_dev, job.scan_sorted = dev[0], dev[1], sorted_
        for k, v in fields.items():
            setattr(job, k, v)
        return job

    def call(self, reg, entry, job, pts=None):
        """(return code, final state, iterations, effect_num) of one call through the C entry point."""
        w, L = self.w, reg.L
        rep = self.api.lii_iekf_report()
        st = (w.st_cv if entry == "cv" else w.st0).copy()
        sp = st.pod.ctypes.data_as(C.c_void_p)
        if entry == "plain":
            rc = L.lii_scan_register(reg.h, C.byref(job), sp, w.st0.pod.ctypes.data_as(C.c_void_p), C.byref(rep))
        elif entry == "imu":
            reg.imu_carry = self.carry0
            rows = self.imu_rows(pts)
            rc = L.lii_scan_register_imu(reg.h, C.byref(job), rows.ctypes.data, len(rows), T_BEG, sp, None, C.byref(rep))
        else:
            rc = L.lii_scan_register_cv(reg.h, C.byref(job), 0.1, self.cg.ctypes.data, self.ca.ctypes.data, sp, None, C.byref(rep))
        return rc, st.pod.copy(), int(rep.iterations), int(rep.effect_num)


def same(a, b):
    return a[0] == b[0] == 0 and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


@pytest.fixture(scope="module")
def forms(oracle, small_world):
    f = Forms(oracle, small_world)
    yield f
    f.reg.close()


class Hook:
    """A real WAIT_HOOK that records its calls."""

    def __init__(self, api):
        self.calls = []
        self.fn = api.WAIT_HOOK(lambda _arg: self.calls.append(1))
        self.ptr = C.cast(self.fn, C.c_void_p)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("size", (48, 56, 72, 88))
def test_a_job_of_every_accepted_size_reads_no_byte_behind_it(forms, entry, size):
    """The bytes behind the stated size hold values that would change the call if read: scan_sorted = 1 and map_update = 1 behind 48 (the
    scan is in the sensor's order: claiming it sorted de-skews to the wrong sweep end; a map update changes the map under the next call),
    a valid next_scan_dev / next_n_scan behind 56, a hook behind 72.  Each job gives the bits of the size-88 job with those fields zero,
    before it and again after it, and the hook was not called."""
    reg = forms.reg
    for n in SIZES_N:
        pts = forms.scans[(n, size != 48)]
        dev = reg.device_scan(pts)
        hook = Hook(forms.api)
        behind = {}
        if size < 56:
            behind.update(scan_sorted=1, map_update=1)
        if size < 72:
            behind.update(next_scan_dev=dev[0], next_n_scan=dev[1])
        if size < 88:
            behind.update(while_waiting=hook.ptr)
        plain88 = forms.job(entry, 88, dev, sorted_=0 if size == 48 else 1)
        ref = forms.call(reg, entry, plain88, pts)
        got = forms.call(reg, entry, forms.job(entry, size, dev, sorted_=0 if size == 48 else 1, **behind), pts)
        again = forms.call(reg, entry, plain88, pts)
        assert same(ref, got), (entry, size, n, ref[0], got[0], ref[2:], got[2:])
        assert same(ref, again), (entry, size, n, "the call left something behind")
        assert hook.calls == [], (entry, size, n)


def test_a_refused_call_leaves_nothing_behind(forms):
    """A good call that announces the next scan, three refused calls (each with a hook, never called), the good call for the announced
    scan: both good calls give the bits of the same two calls on a fresh handle with no refused call between."""
    api = forms.api
    a, b = forms.scans[(513, True)], forms.scans[(1025, True)]

    def two_calls(reg, refused):
        da, db = reg.device_scan(a), reg.device_scan(b)
        first = forms.call(reg, "plain", forms.job("plain", 88, da, next_scan_dev=db[0], next_n_scan=db[1]))
        codes, hooks = [], []
        for fields in refused:
            hook = Hook(api)
            job = forms.job("plain", 88, db, while_waiting=hook.ptr)
            for k, v in fields.items():
                setattr(job, k, v)
            codes.append(forms.call(reg, "plain", job)[0])
            hooks.append(hook.calls)
        second = forms.call(reg, "plain", forms.job("plain", 88, db))
        return first, second, codes, hooks

    bad = (dict(undistort=3), dict(n_scan_dev=MAX_SCAN + 1), dict(opts=api.lii_iekf_opts(0, 1)))
    out = []
    for refused in (bad, ()):
        reg = forms.registrar()  # (a handle of its own each: the same history but for the refused calls)
        try:
            out.append(two_calls(reg, refused))
        finally:
            reg.close()
    got, want = out
    assert got[2] == [INVALID, CAPACITY, INVALID]
    assert got[3] == [[], [], []]
    assert same(want[0], got[0]) and same(want[1], got[1])


@pytest.mark.parametrize("entry", ("imu", "cv"))
def test_the_hook_runs_once_per_call_of_the_propagating_entry_points(forms, entry):
    reg, w = forms.reg, forms.w
    calls = []
    for n in SIZES_N:
        pts = forms.scans[(n, True)]
        out = []
        for hook in (None, lambda: calls.append(n)):
            reg.scan_upload(pts)
            if entry == "imu":
                reg.imu_carry = forms.carry0
                st, _, rep = reg.register_imu(forms.imu_rows(pts), T_BEG, w.st0.copy(), leaf=LEAF, max_iterations=MAX_IT, imu_en=True, scan_sorted=True,
                                              while_waiting=hook)
            else:
                st, _, rep = reg.register_cv(0.1, 0.01, 0.01, w.st_cv.copy(), leaf=LEAF, max_iterations=MAX_IT, scan_sorted=True, while_waiting=hook)
            out.append((0, st.pod.copy(), rep["iterations"], rep["effect_num"]))
        assert same(out[0], out[1]), (entry, n)
    assert calls == list(SIZES_N)


def test_the_hook_runs_once_behind_a_host_driven_update(forms):
    """LII_TEST=host_solve (read when the handle is created): no wait inside the update, the hook runs behind it - once."""
    w = forms.w

    def run():
        reg = forms.registrar()
        try:
            calls, out = [], []
            for n in SIZES_N:
                for hook in (None, lambda: calls.append(n)):
                    reg.scan_upload(forms.scans[(n, True)])
                    st = w.st0.copy()
                    rep = reg.scan_register(st, w.st0, imu_poses=forms.T12, leaf=LEAF, max_iterations=MAX_IT, imu_en=True, scan_sorted=True, while_waiting=hook)
                    out.append((0, st.pod.copy(), rep["iterations"], rep["effect_num"]))
            return calls, out
        finally:
            reg.close()
    calls, out = _with_env("host_solve", run)
    assert calls == list(SIZES_N)
    assert same(out[0], out[1]) and same(out[2], out[3])

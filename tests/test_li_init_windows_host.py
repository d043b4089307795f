"""The pure-numpy side of Registrar.li_init_windows (no GPU): li_init_prefix_windows and li_init_sliding_windows on hand-made stamp
arrays - counts, ends, IMU ranges - and li_init_spread on a hand-made record array with one refused record."""
import numpy as np
import pytest

import lidar_imu_init_amd as lii
from lidar_imu_init_amd import api


def _rows(w):
    return [tuple(int(x) for x in r.tolist()[:4]) for r in w]


def test_prefix_windows_aligned():
    t = 0.1 * np.arange(1, 531)
    w = lii.li_init_prefix_windows(t, first=200, step=100)
    assert w.dtype == lii.LI_INIT_WINDOW_IN_DTYPE
    assert _rows(w) == [(0, c, 0, c) for c in (200, 300, 400, 500, 530)]  # the whole accumulation comes last
    assert _rows(lii.li_init_prefix_windows(t[:400], first=200, step=100)) == [(0, c, 0, c) for c in (200, 300, 400)]
    assert _rows(lii.li_init_prefix_windows(t[:200])) == [(0, 200, 0, 200)]
    with pytest.raises(ValueError):
        lii.li_init_prefix_windows(t, first=199)          # the aligned form admits 200 states or more
    with pytest.raises(ValueError):
        lii.li_init_prefix_windows(t[:150], first=200)
    with pytest.raises(ValueError):
        lii.li_init_prefix_windows(t, step=0)


def test_prefix_windows_raw():
    lidar_t = 1.0 + 0.125 * np.arange(50)          # 1.0 .. 7.125 (binary fractions: the comparisons below are exact)
    imu_t = 0.5 + 0.0078125 * np.arange(1000)      # 0.5 .. 8.30: stamp k = 0.5 + k / 128
    w = lii.li_init_prefix_windows(lidar_t, imu_t, first=10, step=20, margin=0.0, move_start_time=1.25)
    assert list(w["lidar_count"]) == [10, 30, 50] and not w["lidar_begin"].any() and not w["imu_begin"].any()
    ends = lidar_t[[9, 29, 49]]
    assert list(w["imu_count"]) == [int((e - 0.5) * 128) + 1 for e in ends]
    for c, e in zip(w["imu_count"], ends):
        assert imu_t[c - 1] == e and imu_t[c] > e   # the last IMU stamp not later than the window's last LiDAR stamp
    assert list(w["move_start_time"]) == [1.25] * 3
    wm = lii.li_init_prefix_windows(lidar_t, imu_t, first=10, step=20, margin=0.254)
    for c, e in zip(wm["imu_count"], ends):
        assert imu_t[c - 1] <= e + 0.254 < imu_t[c]
    assert list(wm["imu_count"] - w["imu_count"]) == [32, 32, 32]
    # a margin beyond the last IMU stamp ends at the sequence's end
    assert lii.li_init_prefix_windows(lidar_t, imu_t, first=50, margin=10.0)["imu_count"][0] == 1000
    assert lii.li_init_prefix_windows(lidar_t, imu_t, first=1, step=100)["lidar_count"].tolist() == [1, 50]  # no 200 floor in the raw form


def test_sliding_windows():
    t = 0.1 * np.arange(1000)
    w = lii.li_init_sliding_windows(t, length=400, step=250)
    assert _rows(w) == [(b, 400, b, 400) for b in (0, 250, 500)]  # 750 + 400 > 1000
    assert _rows(lii.li_init_sliding_windows(t, length=1000, step=1)) == [(0, 1000, 0, 1000)]
    with pytest.raises(ValueError):
        lii.li_init_sliding_windows(t, length=199, step=10)
    with pytest.raises(ValueError):
        lii.li_init_sliding_windows(t, length=1001, step=10)
    imu_t = -1.0 + 0.01 * np.arange(10_300)        # -1.0 .. 101.99
    r = lii.li_init_sliding_windows(t, imu_t, length=300, step=300, margin=0.1)
    assert list(r["lidar_begin"]) == [0, 300, 600] and list(r["lidar_count"]) == [300] * 3
    for k, b in enumerate((0, 300, 600)):
        lo, cnt = int(r["imu_begin"][k]), int(r["imu_count"][k])
        first, last = t[b] - 0.1, t[b + 299] + 0.1
        assert imu_t[lo] >= first - 1e-9 and imu_t[lo - 1] < first - 1e-9
        assert imu_t[lo + cnt - 1] <= last + 1e-9 and imu_t[lo + cnt] > last + 1e-9
        assert r["move_start_time"][k] == t[b]


def test_window_array_forms():
    a = api.li_init_window_array([(3, 200), (1, 2, 3, 4), (5, 6, 7, 8, 9.5)])
    assert [tuple(x.tolist()) for x in a] == [(3, 200, 3, 200, 0.0), (1, 2, 3, 4, 0.0), (5, 6, 7, 8, 9.5)]
    assert api.li_init_window_array(a) is a or np.array_equal(api.li_init_window_array(a), a)
    with pytest.raises(ValueError):
        api.li_init_window_array([(1, 2, 3)])


def _rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def test_spread_with_one_refused_record():
    rec = np.zeros(4, lii.LI_INIT_WINDOW_DTYPE)
    base = _rot_z(30.0)
    for k, (deg, T, lag) in enumerate(((2.0, (0.3, 0.0, 0.4), 0.010), (None, None, None), (-1.0, (0.0, 0.0, 0.1), 0.004), (0.0, (0.0, 0.0, 0.0), 0.001))):
        if deg is None:
            rec[k]["status"] = api.LII_WIN_FILTER61  # refused: zeros behind the status
            continue
        rec[k]["R_LI"], rec[k]["T_LI"], rec[k]["total_time_lag"] = _rot_z(deg) @ base, T, lag
    s = lii.li_init_spread(rec)
    assert list(s["index"]) == [0, 2, 3]
    assert np.allclose(s["rot_deg"], [2.0, 1.0, 0.0], atol=1e-12)
    assert np.allclose(s["dT"], [0.5, 0.1, 0.0], atol=1e-15)
    assert np.allclose(s["dlag"], [0.009, 0.003, 0.0], atol=1e-15)
    assert np.isclose(s["rot_deg_mean"], 1.0) and np.isclose(s["rot_deg_std"], np.std([2.0, 1.0, 0.0]))
    assert np.isclose(s["dT_mean"], 0.2) and np.isclose(s["dlag_mean"], 0.004) and np.isclose(s["dlag_std"], np.std([0.009, 0.003, 0.0]))
    # a rotation of 180 degrees about an axis is measured as such (the trace alone would lose digits there)
    rec[0]["R_LI"] = np.diag([1.0, -1.0, -1.0]) @ rec[3]["R_LI"]
    assert np.isclose(lii.li_init_spread(rec)["rot_deg"][0], 180.0)
    rec["status"] = api.LII_WIN_NO_OVERLAP
    with pytest.raises(ValueError):
        lii.li_init_spread(rec)

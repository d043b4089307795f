"""The reference of the surface-statistics tests, tested itself (no GPU): analytic cases of map_surface_cases.Surface, the selection
hash against a scalar transcription, the probe behind the derived bounds, and the CONDITIONS test_gpu_map_surface.py relies on - how
many normals the comparison may leave out, and how far every used point of the crispness cases is from the degeneracy threshold."""
import numpy as np
import pytest

from map_radius_cases import Balls
from map_surface_cases import (CRISP_WORLD, DEGENERATE, GAP_MIN, MAX_DISTS, Surface, crispness_reference, mix, selected, sheet_map,
                               small_world_crispness, small_world_surface)


def _surface(q, pts, md):
    q, pts = np.asarray(q, np.float32), np.asarray(pts, np.float32)
    return Surface(q, pts, Balls(q, pts, md).case(md), md)


def test_a_dyadic_lattice_plane_is_exact():
    """Points at multiples of 2^-4 in the plane z = 1.5, queries on the lattice: every moment is exactly representable."""
    g = np.arange(-32, 33) / 16.0
    pts = np.array([[x, y, 1.5] for x in g for y in g], np.float32)
    q = np.array([[0.0, 0.0, 1.5], [0.25, -0.5, 1.5], [0.0, 0.0, 1.5 + 1 / 16]], np.float32)
    md = 0.25  # radius 0.5 = 8 lattice steps; the lattice reaches 2.0: no ball is cut
    ref = _surface(q, pts, md)
    on = sum(1 for i in range(-8, 9) for j in range(-8, 9) if i * i + j * j <= 64)
    assert ref.count[0] == ref.count[1] == on
    m2 = sum(i * i for i in range(-8, 9) for j in range(-8, 9) if i * i + j * j <= 64) / 256.0 / on
    for k in (0, 1):
        assert np.array_equal(ref.mean[k], q[k].astype(np.float64))
        assert np.array_equal(ref.c6[k], [m2, 0.0, 0.0, m2, 0.0, 0.0])
        assert np.array_equal(ref.eig[k], [0.0, m2, m2]) and np.array_equal(np.abs(ref.normal[k]), [0.0, 0.0, 1.0])
        assert ref.curvature[k] == 0.0
    # off the plane by one step: the centroid lies in the plane, the covariance is still flat
    assert ref.mean[2, 2] == 1.5 and ref.eig[2, 0] == 0.0 and ref.count[2] < on


def test_a_point_set_with_a_known_covariance():
    """The eight corners of a box around the query, twice over an offset of hundreds of metres: C = diag(a^2, b^2, c^2)."""
    a, b, c = 0.5, 0.25, 0.125
    for centre in ([0.0, 0.0, 0.0], [512.0, -256.0, 64.0]):
        centre = np.array(centre)
        pts = np.array([centre + [sx * a, sy * b, sz * c] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
        ref = _surface(centre[None], pts, 1.0)
        assert ref.count[0] == 8 and np.array_equal(ref.mean[0], centre)
        assert np.array_equal(ref.eig[0], [c * c, b * b, a * a]) and np.array_equal(np.abs(ref.normal[0]), [0, 0, 1])
        assert ref.curvature[0] == (c * c) / (a * a + b * b + c * c)
    # fewer than three points: not valid, everything but count and mean is zero
    ref = _surface(np.zeros((1, 3)), np.array([[0.1, 0, 0], [0, 0.1, 0], [5, 5, 5]]), 0.04)
    assert ref.count[0] == 2 and not ref.valid[0] and not ref.eig[0].any() and not ref.normal[0].any() and ref.mean[0, 0] == np.float32(0.1) / 2


def test_the_selection_hash():
    pts = np.array([[1.0, 2.0, 3.0], [-0.5, 0.25, 1e-3], [0.0, -0.0, 7.5]], np.float32)
    b = pts.view(np.uint32)
    for row, got in zip(b, mix(pts)):
        h = ((int(row[0]) * 0x9E3779B1) ^ (int(row[1]) * 0x85EBCA77) ^ (int(row[2]) * 0xC2B2AE3D)) & 0xFFFFFFFF
        assert int(got) == h ^ (h >> 15)
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-20, 20, (50_000, 3)).astype(np.float32)
    assert selected(cloud, 1).all()
    share = selected(cloud, 16).mean()
    assert abs(share - 1 / 16) < 0.005  # binomial: sigma = 0.0011
    perm = rng.permutation(len(cloud))
    assert np.array_equal(selected(cloud, 16)[perm], selected(cloud[perm], 16))  # a property of the point


@pytest.mark.parametrize("max_dist", MAX_DISTS)
def test_conditions_the_gpu_parity_test_relies_on(small_world, max_dist):
    q, balls, refs = small_world_surface(small_world)
    ref = refs[max_dist]
    v = ref.valid
    small_gap = v & (ref.gap() < GAP_MIN)
    print(f"max_dist {max_dist}: populations 0 - {ref.count.max()}, valid {v.sum()}, gap below {GAP_MIN}: {small_gap.sum()}, smallest gap {ref.gap()[v].min():.3g}")
    assert small_gap.sum() <= 0.01 * v.sum()
    assert ref.count[-1] == ref.count[-2] == 0 and not ref.mean[-2:].any()  # the query at 1e7 m and the NaN query
    assert ref.count.max() > {0.04: 8, 0.25: 64, 1.0: 256}[max_dist]  # more than one trip of 64 points from 0.25 on
    # the probe of the bounds: the same sums in the opposite order
    rev = Surface(q, balls.pts, balls.case(max_dist), max_dist, reverse=True)
    share = (np.abs(rev.c6[v] - ref.c6[v]).max(axis=1) / ref.c_bound()[v]).max()
    print(f"max_dist {max_dist}: reversed sums move C by {share:.3g} of the bound")
    assert share <= 1.0
    assert np.all(np.abs(rev.eig[v] - ref.eig[v]).max(axis=1) <= ref.eig_bound()[v])


def _far_from_the_threshold(ref, who):
    e = ref.eig[~ref.sparse]
    ratio = e[:, 0] / e[:, 2]  # (count >= min_count >= 4 distinct points: eig[2] > 0)
    print(f"{who}: {len(e)} points with count >= min_count, eig0 / eig2 from {ratio.min():.3g}")
    assert np.all((ratio >= 1e6 * DEGENERATE) | (ratio <= 1e-6 * DEGENERATE)), f"{who}: a point within 1e6 of the degeneracy threshold"


def test_conditions_the_gpu_crispness_test_relies_on(small_world):
    out, bounds, ref = small_world_crispness(small_world)
    print(out, bounds)
    assert 3000 < out["n_selected"] < 6000 and out["n_used"] > 0.9 * out["n_selected"] and CRISP_WORLD["min_count"] == 5
    _far_from_the_threshold(ref, "small_world")
    assert bounds["mme"] < 1e-9 and bounds["mpv"] < 1e-12 * out["mpv"] * 1e3
    flat, _, rf = crispness_reference(sheet_map(), 0.25, 5, 1)
    rough, _, rr = crispness_reference(sheet_map(noise=0.03), 0.25, 5, 1)
    _far_from_the_threshold(rf, "sheets")
    _far_from_the_threshold(rr, "sheets + 3 cm")
    for fig in (flat, rough):
        assert (fig["n_selected"], fig["n_sparse"], fig["n_degenerate"]) == (5049, 40, 9) and fig["n_used"] == 5000
    assert rough["mme"] > flat["mme"] and rough["mpv"] > flat["mpv"]  # the property the figures are for

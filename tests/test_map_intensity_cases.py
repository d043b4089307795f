"""The cases of the map-intensity tests are what they claim to be (no GPU): distinct triples, the voxel populations of the fold case, which
batch point is closest to its voxel centre, the one-cell growth batch; and the lookup table refuses a triple given twice."""
import numpy as np
import pytest

import map_intensity_cases as IC


def test_fold_case_is_what_it_says():
    case = IC.fold_case()
    IC.check_fold_case(case)
    # the survivors carry the intensity of the input point with the same bits
    t = IC.Table(case["stored"], case["batch"])
    t.check(case["survivors"])


def test_fold_case_on_a_small_cell_grid():
    IC.check_fold_case(IC.fold_case(seed=6))


def test_growth_batch_shares_one_cell():
    IC.check_growth_batches(IC.growth_batches())


def test_clouds_have_distinct_triples_and_intensities():
    rng = np.random.default_rng(1)
    a = IC.distinct_cloud(rng, 257)
    b = IC.distinct_cloud(rng, 300, lo=20, hi=30, first=1 + len(a))
    IC.assert_distinct_triples(a, b)
    w = np.r_[a[:, 3], b[:, 3]]
    assert len(np.unique(w)) == len(w) and (w != 0).all()
    rec = IC.as_xyzinormal(a)
    assert rec.shape == (len(a), 12) and rec.strides[0] == 48 and np.array_equal(rec[:, 8], a[:, 3]) and (rec[:, 3:8] == -7.5).all()


def test_table_looks_rows_up_by_their_bits():
    rng = np.random.default_rng(2)
    a = IC.distinct_cloud(rng, 50)
    t = IC.Table(a)
    t.check(a[::-1])
    wrong = a.copy()
    wrong[7, 3] += 1
    with pytest.raises(AssertionError):
        t.check(wrong)
    with pytest.raises(AssertionError):
        IC.Table(a, a[:1])
    assert IC.same_rows_as_set(a, a[rng.permutation(len(a))]) and not IC.same_rows_as_set(a, wrong)

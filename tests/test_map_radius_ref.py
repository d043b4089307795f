"""The yardstick of lii_map_radius, checked on the CPU: the UNMODIFIED reference tree's Nearest_Search with k above the ball's population
- the reference's form of the ball query - returns exactly the float32 brute-force ball for max_dist >= 1: counts, d2 bits and point rows
as multisets per query.  Below 1 the tree's large-k answer is incomplete (it cuts sub-trees at box_d2 > max_dist^2): the range where the
device test holds the library to the brute force alone."""
import numpy as np
import pytest

from map_radius_cases import FAR_EVERY_REF, MAX_DISTS_TREE, check_radius, small_world_balls, tree_balls


@pytest.fixture(scope="module")
def ref_tree(oracle, small_world):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref is not built (the reference sources are not on this machine)")
    tree = oracle.Tree("ref")
    tree.build(np.ascontiguousarray(small_world[1], np.float32))
    yield tree
    tree.close()


@pytest.mark.parametrize("max_dist", MAX_DISTS_TREE)
def test_reference_tree_with_large_k_equals_the_brute_force_ball(ref_tree, small_world, max_dist):
    q, balls = small_world_balls(small_world)
    sel = np.arange(0, len(q), FAR_EVERY_REF if max_dist > 5.0 else 1)
    expected = balls.case(max_dist, sel)
    k = int(np.diff(expected[0]).max()) + 1
    off, pts, d2 = tree_balls(ref_tree, q[sel], max_dist, k)
    check_radius(off, pts, d2, expected, balls.pts, f"reference tree, k = {k}, max_dist = {max_dist}", q=q[sel])


def test_the_query_set_covers_empty_small_and_large_balls(small_world):
    q, balls = small_world_balls(small_world)
    cnt1, cnt5 = np.diff(balls.case(1.0)[0]), np.diff(balls.case(5.0)[0])
    cnt30 = np.diff(balls.case(30.0, np.arange(0, len(q), 4))[0])
    assert (cnt1 == 0).sum() >= 100 and cnt1.max() > 64 and cnt5.sum() > 1 << 20 and cnt30.max() > 4096 and cnt30.sum() > 2 << 20
    assert cnt5[-1] == 0 and cnt5[-2] == 0 and np.isnan(q[-1, 1]) and q[-2, 0] == np.float32(1e7)


def test_below_one_the_large_k_answer_of_the_tree_is_incomplete(ref_tree, small_world):
    """max_dist = 0.25: the tree accepts points at d2 <= 0.25 and cuts sub-trees at box_d2 > 0.0625 - some balls come back short."""
    q, balls = small_world_balls(small_world)
    eo, _, _ = balls.case(0.25)
    bc = np.diff(eo)
    _, _, cnt = ref_tree.knn(q, k=int(bc.max()) + 1, max_dist=0.25, threads=3)
    short = int(np.count_nonzero(cnt < bc))
    print(f"max_dist = 0.25: {short} of {len(q)} balls of the tree hold fewer points than the brute force's")
    assert short > 0 and np.all(cnt <= bc)

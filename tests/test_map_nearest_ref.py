"""The yardstick of lii_map_nearest, checked on the CPU: KD_TREE::Nearest_Search of the UNMODIFIED reference tree equals a float32 brute
force (calc_dist's evaluation order) for any k and any max_dist >= 1 - counts, d2 bit for bit, points wherever the distances are distinct.
That is the rule the device code reproduces (tests/test_gpu_map_nearest.py holds it to the same brute force).  Below max_dist = 1 the
tree prunes sub-trees at box_d2 > max_dist^2, tighter than it accepts points: its answer depends on its shape - the range the library refuses."""
import numpy as np
import pytest

from map_nearest_cases import CASES, TIED_SHARE_MAX, check_answer, small_world_brute


@pytest.fixture(scope="module")
def ref_tree(oracle, small_world):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref is not built (the reference sources are not on this machine)")
    tree = oracle.Tree("ref")
    tree.build(np.ascontiguousarray(small_world[1], np.float32))
    yield tree
    tree.close()


@pytest.mark.parametrize("k,max_dist", CASES)
def test_reference_tree_equals_brute_force(ref_tree, small_world, k, max_dist):
    q, brute = small_world_brute(small_world)
    pts, d2, cnt = ref_tree.knn(q, k=k, max_dist=max_dist, threads=3)
    share = check_answer(brute, k, max_dist, pts, d2, cnt, "reference tree", pad=np.inf)
    assert share <= TIED_SHARE_MAX  # the cap the device test relies on


def test_query_set_covers_the_cases(small_world):
    """d2 = 0, empty, short and full lists, the far query and the NaN one are all in the set."""
    q, brute = small_world_brute(small_world)
    cnt, d2, _, _ = brute.case(64, 1.0)
    assert (d2[:, 0] == 0).sum() >= 400 and (cnt == 0).sum() >= 100 and ((cnt > 0) & (cnt < 64)).sum() >= 50 and (cnt == 64).sum() >= 100
    assert brute.case(5, 30.0)[0][-2:].tolist() == [0, 0] and q[-2, 0] == np.float32(1e7) and np.isnan(q[-1, 1])
    assert (brute.case(1, 30.0)[0] == 0).sum() >= 10  # 8 m outside: nothing within sqrt(30) m


def test_below_one_the_tree_depends_on_its_shape(ref_tree, small_world):
    """max_dist = 0.25: points at d2 <= 0.25 are accepted, sub-trees are cut at box_d2 > 0.0625 - some queries lose neighbours the brute force finds."""
    q, brute = small_world_brute(small_world)
    _, _, cnt = ref_tree.knn(q, k=5, max_dist=0.25, threads=3)
    bc = brute.case(5, 0.25)[0]
    differ = int(np.count_nonzero(cnt != bc))
    print(f"max_dist = 0.25, k = 5: {differ} of {len(q)} counts differ from the brute force")
    assert differ > 0 and np.all(cnt <= bc)

"""The refit's definition (tests/lbvh_refit_ref.py) against the builder's restatement (oracle/lbvh_ref.py): a refit of
unmoved geometry gives the build back (triangles and topology bitwise, boxes as values), a refit of displaced geometry
is a valid tree with exact boxes, and the fold's operand order is the one written down."""
import numpy as np
import pytest

import lbvh_refit_ref as R
from lbvh_refit_ref import L


def _random_tris(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 45), np.float32)
    t[:, :9] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    t[:, 42] = np.arange(n)
    return t


def _displaced(t, seed):
    rng = np.random.default_rng(seed)
    out = t.copy()
    out[:, :9] += rng.uniform(-0.3, 0.3, (t.shape[0], 9)).astype(np.float32)  # every vertex by its own vector
    return out


@pytest.mark.parametrize("n,leaf_n,ploc", [(1, 4, 0), (3, 4, 0), (17, 1, 0), (1000, 4, 16), (1000, 3, 32)])
def test_refit_restatement_against_the_build(n, leaf_n, ploc):
    t = _random_tris(n, seed=n + leaf_n)
    tri, nodes = L.lbvh(t, leaf_n, ploc)
    order = R.recover_order(tri)
    assert np.array_equal(np.sort(order), np.arange(n))
    assert np.array_equal(t[order].view(np.uint32), tri.view(np.uint32))
    # unmoved: the build comes back
    tri2, nodes2 = R.refit(t, order, nodes)
    assert np.array_equal(tri2.view(np.uint32), tri.view(np.uint32))
    assert np.array_equal(nodes2[:, :6].view(np.uint32), nodes[:, :6].view(np.uint32))
    assert np.array_equal(nodes2[0].view(np.uint32), nodes[0].view(np.uint32))
    assert np.array_equal(nodes2[:, 6:], nodes[:, 6:])
    # displaced: a valid tree over the new positions, every box exact
    moved = _displaced(t, seed=n)
    tri3, nodes3 = R.refit(moved, order, nodes)
    assert np.array_equal(tri3.view(np.uint32), moved[order].view(np.uint32))
    assert np.array_equal(nodes3[:, :6].view(np.uint32), nodes[:, :6].view(np.uint32))
    L.check_tree(tri3, nodes3, leaf_n)
    assert not np.array_equal(nodes3[1:, 6:], nodes[1:, 6:])


def test_refit_fold_keeps_the_first_operand_on_ties():
    """glm's min / max return the first operand unless the second compares less / greater; +0.0 == -0.0, so a leaf
    whose triangles hold +0.0 then -0.0 in one coordinate keeps +0.0 in both corners, and -0.0 the other way round."""
    t = np.zeros((2, 45), np.float32)
    t[:, :9] = np.float32([[0.0, 1.0, 2.0] * 3, [-0.0, 1.0, 2.0] * 3])
    t[:, 42] = np.arange(2)
    nodes = np.zeros((2, 12), np.float32)
    nodes[0] = L.DUMMY_NODE
    nodes[1, 3], nodes[1, 4] = 2, 0  # one leaf: both triangles, from position 0
    for order, sign in (([0, 1], False), ([1, 0], True)):
        _, out = R.refit(t, np.array(order), nodes)
        assert out[1, 6] == 0.0 and out[1, 9] == 0.0
        assert bool(np.signbit(out[1, 6])) is sign and bool(np.signbit(out[1, 9])) is sign
        assert np.array_equal(out[1, 7:9], np.float32([1.0, 2.0])) and np.array_equal(out[1, 10:12], np.float32([1.0, 2.0]))
    # an interior node takes its left child (childs.x) first
    nodes = np.zeros((4, 12), np.float32)
    nodes[0] = L.DUMMY_NODE
    nodes[1, 0], nodes[1, 1] = 3, 2  # left = node 3, right = node 2
    nodes[2, 3], nodes[2, 4] = 1, 0  # node 2: triangle 0 (+0.0)
    nodes[3, 3], nodes[3, 4] = 1, 1  # node 3: triangle 1 (-0.0)
    _, out = R.refit(t, np.array([0, 1]), nodes)
    assert np.signbit(out[1, 6]) and np.signbit(out[1, 9])  # the left child's -0.0
    # a NaN first operand stays, a NaN second operand is ignored: comparisons with NaN are false
    t2 = t.copy()
    t2[0, 0] = np.nan
    nodes1 = np.zeros((2, 12), np.float32)
    nodes1[0] = L.DUMMY_NODE
    nodes1[1, 3] = 2
    _, a = R.refit(t2, np.array([0, 1]), nodes1)
    _, b = R.refit(t2, np.array([1, 0]), nodes1)
    assert np.isnan(a[1, 6]) and not np.isnan(b[1, 6])

"""The restatement of the device-derived walk trees (tests/lbvh_trees_ref.py) checked against their definitions on
trees of the CPU LBVH / PLOC builder (oracle/lbvh_ref.py), without a GPU: the properties below are computed from the
produced buffers alone, so they check the restatement rather than repeat it. tests/test_gpu_lbvh_trees.py then holds
the device stage and the library's host functions to the restatement bit for bit."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import lbvh_ref as L  # noqa: E402

import lbvh_trees_ref as T  # noqa: E402


def _random_tris(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 45), np.float32)
    t[:, :9] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    t[:, 42] = np.arange(n)
    return t


_CASES = [(n, leaf_n, ploc) for n in (1, 2, 3, 5, 17, 1000) for leaf_n in (1, 4) for ploc in (0, 16)]
_cache = {}


def _trees(n, leaf_n, ploc):
    key = (n, leaf_n, ploc)
    if key not in _cache:
        _, nodes = L.lbvh(_random_tris(n, seed=n + 11), leaf_n, ploc)
        nodes.setflags(write=False)
        _cache[key] = (nodes, T.trees(nodes))
    return _cache[key]


def _irefs(rec, lo, hi):
    return rec[:, lo:hi].copy().view(np.int32)


def _leaf_boxes(nodes):
    """leaf ref -> (AA, BB) bits, from the texels."""
    out = {}
    for f in nodes[1:]:
        if f[3] > 0:
            ref = -(int(f[4]) * 16 + int(f[3])) - 1
            assert ref not in out
            out[ref] = f[6:12].view(np.uint32).tolist()
    return out


@pytest.mark.parametrize("n,leaf_n,ploc", _CASES)
def test_binary_tree_and_leaf_list(n, leaf_n, ploc):
    nodes, tr = _trees(n, leaf_n, ploc)
    boxes = _leaf_boxes(nodes)
    lv = tr["leaves"]
    assert tr["nleaves"] == len(lv) == len(boxes)
    refs = _irefs(lv, 3, 4)[:, 0].tolist()
    assert sorted(refs) == sorted(boxes)
    for row, ref in zip(lv, refs):  # node order, each with its own box
        assert np.r_[row[0:3], row[4:7]].view(np.uint32).tolist() == boxes[ref]
        assert row[7] == 0
    order = [r for r in (-(int(f[4]) * 16 + int(f[3])) - 1 for f in nodes[1:] if f[3] > 0)]
    assert refs == order
    b = tr["binary"]
    if nodes[1, 3] > 0:
        assert len(b) == 0 and tr["root_ref"] == refs[0] and tr["need"] == 0
        return
    assert tr["root_ref"] == 0
    kids = _irefs(b, 12, 14)
    seen, visited, need = [], [], 0
    st = [(0, 1)]
    while st:  # preorder, left first: an interior left child is the next record
        k, depth = st.pop()
        assert k == len(visited)
        visited.append(k)
        need = max(need, depth)
        for side in (1, 0):
            r = int(kids[k, side])
            box = b[k, 6 * side:6 * side + 6].view(np.uint32).tolist()
            if r < 0:
                seen.append(r)
                assert box == boxes[r]
            else:
                st.append((r, depth + 1))
        assert b[k, 14] == 0 and b[k, 15] == 0
    assert len(visited) == len(b) and need == tr["need"]
    assert sorted(seen) == sorted(boxes)


def _union(a, b):
    return np.r_[np.minimum(a[:3], b[:3]), np.maximum(a[3:], b[3:])]


@pytest.mark.parametrize("n,leaf_n,ploc", _CASES)
def test_wide_tree(n, leaf_n, ploc):
    nodes, tr = _trees(n, leaf_n, ploc)
    boxes = _leaf_boxes(nodes)
    w = tr["wide"]
    assert tr["wide_nodes"] == len(w) and tr["nan"] == 0
    if nodes[1, 3] > 0:
        assert len(w) == 0 and tr["root4"] == tr["root_ref"] < 0 and tr["need4"] == 0
        return
    assert tr["root4"] == 0
    refs = _irefs(w, 24, 28)
    assert w.shape[1] == 4 * T.WIDE_STRIDE and np.all(w[:, 28:] == 0)  # padding past the refs, if any, is 0
    seen, count = [], [0]
    need = [0]
    area = lambda bx: np.float32(np.float32(np.float32(bx[3] - bx[0]) * np.float32(bx[4] - bx[1]))  # noqa: E731
                                 + np.float32(np.float32(bx[4] - bx[1]) * np.float32(bx[5] - bx[2]))) + \
        np.float32(np.float32(bx[5] - bx[2]) * np.float32(bx[3] - bx[0]))

    def walk(k, acc):
        """Returns the exact union of the leaf boxes below 4-wide node k; checks numbering, slots and boxes."""
        assert k == count[0]  # depth-first preorder in slot order
        count[0] += 1
        used = [c for c in range(4) if refs[k, c] != T.NONE_REF]
        nc = len(used)
        assert used == list(range(nc)) and nc >= 2
        for c in range(nc, 4):  # empty slots: a box no ray enters
            assert np.all(w[k, [c, 8 + c, 16 + c]] == np.inf) and np.all(w[k, [4 + c, 12 + c, 20 + c]] == -np.inf)
        here = acc + nc - 1
        need[0] = max(need[0], here + 1)
        total = None
        areas = []
        for c in used:
            box = w[k, [c, 8 + c, 16 + c, 4 + c, 12 + c, 20 + c]]
            r = int(refs[k, c])
            if r < 0:
                seen.append(r)
                assert box.view(np.uint32).tolist() == boxes[r]
                below = box
            else:
                below = walk(r, here)
                assert np.array_equal(box, below)  # min / max are exact: the binary node's box is this union
            areas.append(area(box))
            total = below if total is None else _union(total, below)
        assert all(a >= b for a, b in zip(areas, areas[1:]))  # PT_WIDE_ORDER: largest first
        # the greedy collapse left no interior child it could still have opened
        assert nc == 4 or all(int(refs[k, c]) < 0 for c in used)
        return total

    sys.setrecursionlimit(10000)
    root_box = walk(0, 0)
    assert count[0] == len(w)
    assert sorted(seen) == sorted(boxes)  # every binary leaf exactly once
    assert np.array_equal(root_box, nodes[1, 6:12])
    assert need[0] == tr["need4"]


def test_collapse_opens_the_larger_child_and_ties_go_to_the_first():
    """A hand-made tree: root 1 = (2, 3); 2 = (4, 5) small, 3 = (6, 7) large; 6 = (8, 9). The root opens 3 first (the
    larger area), then, of {2, 6, 7}, node 2 and node 6 are interior: 6 is larger and is opened."""
    def leaf(first, lo, hi):
        return [0, 0, 0, 1, first, 0, *lo, *hi]

    def inner(l, r, lo, hi):
        return [l, r, 0, 0, 0, 0, *lo, *hi]

    nodes = np.array([
        np.zeros(12),
        inner(2, 3, (0, 0, 0), (8, 8, 8)),
        inner(4, 5, (0, 0, 0), (1, 1, 1)),
        inner(6, 7, (1, 1, 1), (8, 8, 8)),
        leaf(0, (0, 0, 0), (1, 1, 0.5)),
        leaf(1, (0, 0, 0.5), (1, 1, 1)),
        inner(8, 9, (1, 1, 1), (6, 6, 6)),
        leaf(2, (6, 6, 6), (8, 8, 8)),
        leaf(3, (1, 1, 1), (6, 6, 3)),
        leaf(4, (1, 1, 3), (6, 6, 6)),
    ], np.float32)
    w, root4, need4, lists = T.wide(nodes)
    assert root4 == 0
    # {2, 3} -> open 3 -> {2, 6, 7} -> open 6 -> {2, 8, 9, 7}; sorted by area, descending, stable:
    # areas: 2 -> 3, 8 -> 25 + 10 + 10 = 45, 9 -> 25 + 15 + 15 = 55, 7 -> 12
    assert lists[0] == [9, 8, 7, 2]
    assert lists[1] == [4, 5]
    assert len(w) == 2 and need4 == 5  # root: 4 children (3 beside the one taken), then 2 more
    refs = w[:, 24:28].copy().view(np.int32)
    assert refs[0].tolist() == [-(4 * 16 + 1) - 1, -(3 * 16 + 1) - 1, -(2 * 16 + 1) - 1, 1]
    assert refs[1].tolist() == [-(0 * 16 + 1) - 1, -(1 * 16 + 1) - 1, T.NONE_REF, T.NONE_REF]
    # equal areas (every box the same): the first in the current order is opened, and the sort keeps the order
    flat = nodes.copy()
    flat[1:, 6:9] = 0
    flat[1:, 9:12] = [1, 1, 0]
    _, _, _, lists = T.wide(flat)
    assert lists[0] == [4, 5, 6, 7]  # {2, 3} -> 2 opened (first) -> {4, 5, 3} -> 3 opened -> {4, 5, 6, 7}
    assert lists[1] == [8, 9]
    b, root, need = T.binary(nodes)
    assert root == 0 and need == 3 and len(b) == 4
    assert b[:, 12:14].copy().view(np.int32).tolist() == [[1, 2], [-2, -18], [3, -34], [-50, -66]]


def test_debug_entry_point_is_declared_exported_and_bound():
    from ptsvgf import _lib

    txt = open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf_debug.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(set(re.findall(r"\b(pt_\w+)\s*\(", txt)))
    assert declared == ["pt_debug_lbvh_trees"]
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    assert all(hasattr(lib, n) for n in declared)
    assert set(declared) <= set(_lib.exported_symbols()[0])
    # the drop-in boundary stays free of diagnostics
    assert "pt_debug" not in open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf.h")).read()
    from ptsvgf import gl
    from ptsvgf.renderer import Renderer
    assert callable(gl.lbvh_trees) and callable(Renderer.set_lbvh_wide)

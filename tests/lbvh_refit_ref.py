"""CPU restatement of the BVH refit (pt_bvh_refit, csrc/kernels_bvh.hip refit_nodes): the definition the device
kernel is checked against bit for bit.

TEST INFRASTRUCTURE ONLY: nothing in the product imports it.

A refit keeps a built tree's topology (every node's childs and leafInfo texels) and recomputes the boxes for
triangles that moved but are the same triangles in the same order:
  triangles  tri_sorted = tri_new[order], order being the build's leaf order (order[p] = input index of position p)
  leaf       starting from its first triangle's min(p1, min(p2, p3)) / max(p1, max(p2, p3)), every later triangle t of
             the leaf, in leaf order: lo = gmin(lo, lo_t), hi = gmax(hi, hi_t)
  interior   gmin(left, right) / gmax(left, right), left being childs.x
in float32 with glm's min / max (oracle/lbvh_ref.py _gmin / _gmax: the second operand only where it compares less /
greater). The operand order fixes the result bit for bit, also for +-0 and NaN. The dummy node 0 is untouched.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import lbvh_ref as L  # noqa: E402


def tri_boxes(t: np.ndarray):
    """Per triangle (n, 45): glm min / max over its three vertices, as the build and the refit evaluate them."""
    with np.errstate(invalid="ignore"):
        lo = L._gmin(t[:, 0:3], L._gmin(t[:, 3:6], t[:, 6:9]))
        hi = L._gmax(t[:, 0:3], L._gmax(t[:, 3:6], t[:, 6:9]))
    return lo.astype(np.float32), hi.astype(np.float32)


def refit(tri_new: np.ndarray, order: np.ndarray, nodes_old: np.ndarray):
    """(tri_sorted (n, 45), nodes (m, 12)) after a refit of the tree `nodes_old` (BVHNode_encoded, dummy node 0, root
    node 1) whose build had the leaf order `order`, for the triangles `tri_new` in that build's input order."""
    t = np.asarray(tri_new, np.float32).reshape(-1, 45)
    order = np.asarray(order, np.int64)
    tri_sorted = np.ascontiguousarray(t[order])
    nodes = np.array(nodes_old, np.float32).reshape(-1, 12).copy()
    tlo, thi = tri_boxes(tri_sorted)
    # children before parents: a depth-first walk from the root, boxes on the way back
    stack = [(1, False)]
    with np.errstate(invalid="ignore"):
        while stack:
            i, done = stack.pop()
            f = nodes[i]
            cnt, first = int(f[3]), int(f[4])
            if cnt > 0:
                lo, hi = tlo[first].copy(), thi[first].copy()
                for k in range(first + 1, first + cnt):
                    lo = L._gmin(lo, tlo[k])
                    hi = L._gmax(hi, thi[k])
            elif not done:
                stack += [(i, True), (int(f[1]), False), (int(f[0]), False)]
                continue
            else:
                a, b = nodes[int(f[0])], nodes[int(f[1])]
                lo, hi = L._gmin(a[6:9], b[6:9]), L._gmax(a[9:12], b[9:12])
            f[6:9] = lo
            f[9:12] = hi
    return tri_sorted, nodes


def recover_order(tri_sorted: np.ndarray) -> np.ndarray:
    """The leaf order of a build whose input rows carried their index in column 42 (tests' _random_tris)."""
    return np.asarray(tri_sorted, np.float32).reshape(-1, 45)[:, 42].astype(np.int64)

"""CPU restatement of a skin (pt_pose_apply_skin, csrc/kernels_bvh.hip skin_tris / skin_raster): the definition the
device kernels are checked against bit for bit.

TEST INFRASTRUCTURE ONLY: nothing in the product imports it.

Linear blend skinning of rest-pose corners by up to four bone matrices. A bone is a glm column-major mat4 (16 floats,
the layout of ptsvgf.scene.transform); every operation below is one float32 operation with one rounding, none
contracted (the project builds with -ffp-contract=off). The expressions for a position and a normal are those of
tests/pose_ref.py, whose _cross this module reuses.

  influences a corner (one of the three vertices of a Triangle_encoded row, or of a raster triangle) has four bone
             indices (uint16) and four weights (float32). Weights are not normalised; unused slots carry weight 0
             and any valid index
  kept       a corner whose four weights all compare == 0 keeps the bits of its position and normal. A NaN weight
             is not == 0: that corner is skinned, to NaN. (A corner that names a bone >= n_bones is kept as well: the
             library refuses such a table before it launches, the kernels do not depend on that.)
  blend      over the 12 floats j in {0,1,2, 4,5,6, 8,9,10, 12,13,14} of a mat4:
             M[j] = ((w0 B0[j] + w1 B1[j]) + w2 B2[j]) + w3 B3[j]
             All four terms are always evaluated, so a non-finite float in a bone named with weight 0 yields NaN
             (0 * inf). Floats 3, 7, 11, 15 of a bone are not read: bones are affine
  position   pose_ref.points' expression with M: r[k] = (M[k] x + M[4+k] y) + (M[8+k] z + M[12+k] 1)
  normal     pose_ref.normals' with the cofactor columns of the blended matrix, computed per corner:
             a0 = cross(c1, c2), a1 = cross(c2, c0), a2 = cross(c0, c1) from M's columns,
             v[k] = (a0[k] x + a1[k] y) + a2[k] z, result = v * (1 / sqrt((v.x^2 + v.y^2) + v.z^2)): right under
             non-uniform scale and mirrors; a singular blend gives NaN normals and finite positions
  the rest   every other float of a record is copied

Matrices are absolute: every call skins the rest records.
"""
from __future__ import annotations

import numpy as np

from pose_ref import _cross

F = np.float32
AFFINE = (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)


def _bones(bones) -> np.ndarray:
    return np.ascontiguousarray(bones, np.float32).reshape(-1, 16)


def _influences(idx, w):
    return np.ascontiguousarray(idx).astype(np.int64).reshape(-1, 4), np.ascontiguousarray(w, np.float32).reshape(-1, 4)


def skinned(idx: np.ndarray, w: np.ndarray, n_bones: int) -> np.ndarray:
    """Per corner whether it is skinned: not all four weights == 0, and every index names a bone."""
    with np.errstate(invalid="ignore"):
        kept = np.all(w == F(0.0), axis=1)
    return ~kept & np.all((idx >= 0) & (idx < n_bones), axis=1)


def blend(bones, idx, w) -> np.ndarray:
    """(n, 16) blended matrices for (n, 4) influences; floats 3, 7, 11, 15 are left 0 and mean nothing."""
    bones = _bones(bones)
    idx, w = _influences(idx, w)
    m = np.zeros((len(idx), 16), np.float32)
    with np.errstate(all="ignore"):
        for j in AFFINE:
            b = bones[:, j]
            mul0, mul1, mul2, mul3 = (w[:, s] * b[idx[:, s]] for s in range(4))
            add0 = mul0 + mul1
            add1 = add0 + mul2
            m[:, j] = add1 + mul3
    return m


def points(m: np.ndarray, p: np.ndarray) -> np.ndarray:
    """(n, 3) positions, corner i through its own matrix m[i] (pose_ref.points' expression)."""
    p = np.asarray(p, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for k in range(3):
            add0 = m[:, k] * x + m[:, 4 + k] * y
            add1 = m[:, 8 + k] * z + m[:, 12 + k] * F(1.0)
            out[:, k] = add0 + add1
    return out


def normals(m: np.ndarray, n: np.ndarray) -> np.ndarray:
    """(n, 3) normals, corner i through the normalised cofactor matrix of m[i] (pose_ref.normals' expression)."""
    n = np.asarray(n, np.float32)
    c0, c1, c2 = m[:, 0:3].T, m[:, 4:7].T, m[:, 8:11].T  # (3, n): _cross indexes the components
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    v = np.empty_like(n)
    with np.errstate(all="ignore"):
        a0, a1, a2 = _cross(c1, c2), _cross(c2, c0), _cross(c0, c1)
        for k in range(3):
            v[:, k] = (a0[k] * x + a1[k] * y) + a2[k] * z
        inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        return (v * inv[:, None]).astype(np.float32)


def corners(pos: np.ndarray, nrm: np.ndarray, idx, w, bones):
    """(n, 3) positions and normals of n corners skinned; kept corners keep their bits."""
    bones = _bones(bones)
    idx, w = _influences(idx, w)
    pos, nrm = np.array(pos, np.float32), np.array(nrm, np.float32)
    sel = np.nonzero(skinned(idx, w, len(bones)))[0]
    if sel.size:
        m = blend(bones, idx[sel], w[sel])
        pos[sel] = points(m, pos[sel])
        nrm[sel] = normals(m, nrm[sel])
    return pos, nrm


def tris(rest: np.ndarray, idx, w, bones) -> np.ndarray:
    """(n, 45) Triangle_encoded rows skinned: p1-p3 (floats 0-8), n1-n3 (floats 9-17); idx / w hold 12 entries per
    row (3 corners x 4)."""
    rest = np.asarray(rest, np.float32).reshape(-1, 45)
    out = rest.copy()
    pos, nrm = corners(rest[:, 0:9].reshape(-1, 3), rest[:, 9:18].reshape(-1, 3), idx, w, bones)
    out[:, 0:9] = pos.reshape(-1, 9)
    out[:, 9:18] = nrm.reshape(-1, 9)
    return out


def raster(rest: np.ndarray, idx, w, bones) -> np.ndarray:
    """The raster vertex list (pos3 + nrm3 per vertex, three vertices per triangle, flat) skinned; idx / w hold 12
    entries per triangle."""
    rest = np.asarray(rest, np.float32).reshape(-1, 6)
    pos, nrm = corners(rest[:, 0:3], rest[:, 3:6], idx, w, bones)
    return np.concatenate([pos, nrm], axis=1).reshape(-1)

"""CPU restatement of a pose (pt_pose_apply, csrc/kernels_bvh.hip pose_tris / pose_raster): the definition the device
kernels are checked against bit for bit.

TEST INFRASTRUCTURE ONLY: nothing in the product imports it.

A pose places rest-pose records by one matrix per object. `m` is a glm column-major mat4 (16 floats, the layout of
ptsvgf.scene.transform); every operation below is one float32 operation with one rounding, none contracted (the
project builds with -ffp-contract=off).

  object     a record's objIndex f (float 42 of a Triangle_encoded row; an int per raster triangle) names object
             k = int(f) when f >= 0 and f < n_obj and f == floor(f); otherwise (NaN included) it names none
  kept       a record of no object, and a record whose object's 16 floats all compare == to the identity's, is
             copied bit for bit
  position   glm's mat4 * vec4(p, 1) (scene_prep.cpp xform_point):
             r[k] = (m[k] x + m[4+k] y) + (m[8+k] z + m[12+k] 1)
  normal     with the columns c_j = (m[4j], m[4j+1], m[4j+2]) of the upper 3x3 and the cofactor columns
             a0 = cross(c1, c2), a1 = cross(c2, c0), a2 = cross(c0, c1) (glsl::cross's expressions):
             v[k] = (a0[k] x + a1[k] y) + a2[k] z, result = v * (1 / sqrt((v.x^2 + v.y^2) + v.z^2)) (glsl::normalize)
             -- the inverse transpose up to a scale of either sign: right under non-uniform scale, and flipping with
             the winding under a mirror
  the rest   every other float of a Triangle_encoded row (material, uv, objIndex, padding) is copied

Matrices are absolute: every pose starts from the rest records.
"""
from __future__ import annotations

import numpy as np

IDENTITY = np.eye(4, dtype=np.float32).reshape(16)
F = np.float32


def _cross(a, b):
    """glsl::cross: (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x), each product and difference rounded."""
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float32)


def cofactors(m) -> np.ndarray:
    """The 9 floats a0 | a1 | a2 of one matrix."""
    m = np.asarray(m, np.float32).reshape(16)
    c0, c1, c2 = m[0:3], m[4:7], m[8:11]
    with np.errstate(all="ignore"):
        return np.concatenate([_cross(c1, c2), _cross(c2, c0), _cross(c0, c1)]).astype(np.float32)


def points(m, p: np.ndarray) -> np.ndarray:
    """(n, 3) positions through m."""
    m = np.asarray(m, np.float32).reshape(16)
    p = np.asarray(p, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for k in range(3):
            add0 = m[k] * x + m[4 + k] * y
            add1 = m[8 + k] * z + m[12 + k] * F(1.0)
            out[:, k] = add0 + add1
    return out


def normals(m, n: np.ndarray) -> np.ndarray:
    """(n, 3) normals through the normalised cofactor matrix of m."""
    a = cofactors(m)
    n = np.asarray(n, np.float32)
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    v = np.empty_like(n)
    with np.errstate(all="ignore"):
        for k in range(3):
            v[:, k] = (a[k] * x + a[3 + k] * y) + a[6 + k] * z
        inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        return (v * inv[:, None]).astype(np.float32)


def _mats(mats) -> np.ndarray:
    return np.ascontiguousarray(mats, np.float32).reshape(-1, 16)


def objects_of(f: np.ndarray, n_obj: int) -> np.ndarray:
    """Per record the object its objIndex names, or -1."""
    f = np.asarray(f)
    with np.errstate(invalid="ignore"):
        ok = (f >= 0) & (f < n_obj) & (f == np.floor(f))
    out = np.full(f.shape, -1, np.int64)
    out[ok] = f[ok].astype(np.int64)
    return out


def _moving(mats: np.ndarray):
    """Objects whose matrix is not the identity (any float comparing != to the identity's)."""
    return [k for k in range(len(mats)) if not np.all(mats[k] == IDENTITY)]


def tris(rest: np.ndarray, mats) -> np.ndarray:
    """(n, 45) Triangle_encoded rows posed: p1-p3 (floats 0-8), n1-n3 (floats 9-17), objIndex float 42."""
    mats = _mats(mats)
    rest = np.asarray(rest, np.float32).reshape(-1, 45)
    out = rest.copy()
    obj = objects_of(rest[:, 42], len(mats))
    for k in _moving(mats):
        sel = np.nonzero(obj == k)[0]
        if not sel.size:
            continue
        for v in range(3):
            out[sel, 3 * v:3 * v + 3] = points(mats[k], rest[sel, 3 * v:3 * v + 3])
            out[sel, 9 + 3 * v:12 + 3 * v] = normals(mats[k], rest[sel, 9 + 3 * v:12 + 3 * v])
    return out


def raster(rest: np.ndarray, raster_obj: np.ndarray, mats) -> np.ndarray:
    """The raster vertex list (pos3 + nrm3 per vertex, three vertices per triangle, flat) posed; raster_obj holds one
    int per triangle."""
    mats = _mats(mats)
    rest = np.asarray(rest, np.float32).reshape(-1, 3, 6)
    out = rest.copy()
    obj = objects_of(np.asarray(raster_obj, np.int64), len(mats))
    for k in _moving(mats):
        sel = np.nonzero(obj == k)[0]
        if not sel.size:
            continue
        r = rest[sel].reshape(-1, 6)
        posed = np.concatenate([points(mats[k], r[:, 0:3]), normals(mats[k], r[:, 3:6])], axis=1)
        out[sel] = posed.reshape(-1, 3, 6)
    return out.reshape(-1)


def table(mats: dict, n_obj: int) -> np.ndarray:
    """(n_obj, 16): the named objects' matrices, identity for the others."""
    t = np.tile(IDENTITY, (n_obj, 1))
    for k, m in mats.items():
        t[int(k)] = np.asarray(m, np.float32).reshape(16)
    return t

"""What a caller without a rig needs for Renderer.set_skin / Renderer.skin_objects: the rest positions of the corners
of the two lists, and a chain of bones along a segment that bends (a stem, an arm) with the weights that go with it.

A corner is one vertex of a Triangle_encoded row or of a raster triangle; the arrays here hold one row per corner, in
the order the library reads them (three corners per triangle), and reshape(-1) to the 12 entries per triangle of
Renderer.set_skin.
"""
from __future__ import annotations

import numpy as np


def corner_positions(tri_enc) -> np.ndarray:
    """(3 n, 3) rest positions of the corners of n Triangle_encoded rows (p1, p2, p3: floats 0-8 of 45)."""
    return np.asarray(tri_enc, np.float32).reshape(-1, 45)[:, 0:9].reshape(-1, 3)


def corner_positions_raster(raster) -> np.ndarray:
    """(3 n, 3) rest positions of the corners of a raster vertex list (pos3 + nrm3 per vertex)."""
    return np.asarray(raster, np.float32).reshape(-1, 6)[:, 0:3]


def chain_weights(positions, base, tip, n_bones: int, mask=None):
    """Influences of a chain of n_bones bones from `base` to `tip` for (n, 3) rest positions: with
    s = clamp(dot(p - base, tip - base) / |tip - base|^2, 0, 1), u = s (n_bones - 1), i = min(floor(u), n_bones - 2)
    and f = u - i, a corner gets (i, 1 - f) and (i + 1, f); the other slots are bone 0 with weight 0. n_bones == 1
    gives (0, 1). Corners outside `mask` ((n,) bool) get all-zero weights: they stay where they are. A function of the
    rest position only, so the triangle list and the raster list agree at the vertices they share.
    Returns (bones (n, 4) uint16, weights (n, 4) float32)."""
    if n_bones < 1:
        raise ValueError("chain_weights: n_bones must be >= 1")
    p = np.asarray(positions, np.float64).reshape(-1, 3)
    base, tip = np.asarray(base, np.float64).reshape(3), np.asarray(tip, np.float64).reshape(3)
    d = tip - base
    dd = float(np.dot(d, d))
    if not dd > 0.0:
        raise ValueError("chain_weights: base and tip coincide")
    bones = np.zeros((len(p), 4), np.uint16)
    weights = np.zeros((len(p), 4), np.float32)
    if n_bones == 1:
        weights[:, 0] = 1.0
    else:
        s = np.clip((p - base) @ d / dd, 0.0, 1.0)
        u = s * (n_bones - 1)
        i = np.minimum(np.floor(u), n_bones - 2)
        f = (u - i).astype(np.float32)
        bones[:, 0] = i.astype(np.uint16)
        bones[:, 1] = bones[:, 0] + 1
        weights[:, 0] = np.float32(1.0) - f
        weights[:, 1] = f
    if mask is not None:
        out = ~np.asarray(mask, bool).reshape(-1)
        bones[out] = 0
        weights[out] = 0.0
    return bones, weights


def _rotation(axis, deg: float) -> np.ndarray:
    """3x3 rotation by deg about axis (Rodrigues)."""
    a = np.asarray(axis, np.float64).reshape(3)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(deg)
    return np.eye(3) + np.sin(t) * k + (1.0 - np.cos(t)) * (k @ k)


def chain_bones(base, tip, n_bones: int, bend_deg: float, axis) -> np.ndarray:
    """(n_bones, 16) float32 glm column-major matrices of a chain that bends by bend_deg in all, about `axis`: bone 0
    is the identity, and bone i is bone i - 1 followed down the chain by a rotation of bend_deg / (n_bones - 1) about
    the joint at parameter i / (n_bones - 1) of the rest segment base-tip. A bend of 0 returns exact identities."""
    if n_bones < 1:
        raise ValueError("chain_bones: n_bones must be >= 1")
    out = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n_bones, 1))
    if n_bones == 1 or bend_deg == 0:
        return out
    base, tip = np.asarray(base, np.float64).reshape(3), np.asarray(tip, np.float64).reshape(3)
    step = _rotation(axis, bend_deg / (n_bones - 1))
    m = np.eye(4)
    for i in range(1, n_bones):
        joint = base + (tip - base) * (i / (n_bones - 1))
        local = np.eye(4)
        local[:3, :3] = step
        local[:3, 3] = joint - step @ joint  # a rotation about the rest joint
        m = m @ local
        out[i] = m.T.reshape(16).astype(np.float32)  # column-major
    return out

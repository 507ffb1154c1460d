"""Object motion vectors, restated in float64 numpy from their definition (DESIGN.md "Dynamic scenes"; the device
form is gb_finish, csrc/kernels_pt.hip): a surface point P on a triangle whose vertices were at `prev` one frame ago
and are at `cur` now was at prevP = P + D, D = the vertices' displacements prev - cur blended with P's barycentrics in
`cur`; its motion texel is

    xy = proj(M P) - proj(PV prevP)          (uv units; M = this frame's projection * view, PV = last frame's)
    z  = lin_z_PV(prevP) - lin_z_PV(P)       (the object's own share of the change of linear depth)
    w  = 1

Matrices are 16 floats, column-major (glm::value_ptr order). Everything is vectorised over leading axes."""
import numpy as np


def _clip(m, P):
    m = np.asarray(m, np.float64).reshape(4, 4).T  # column-major -> rows
    P = np.asarray(P, np.float64)
    return P @ m[:, :3].T + m[:, 3]


def proj(m, P):
    """uv of P under m: ndc.xy * 0.5 + 0.5 (rasterize_vert.vert)."""
    c = _clip(m, P)
    return c[..., :2] / c[..., 3:4] * 0.5 + 0.5


def lin_z(m, P):
    """gl_FragCoord.z / gl_FragCoord.w of P under m (rasterize_frag.frag's linear depth)."""
    c = _clip(m, P)
    return (c[..., 2] / c[..., 3] * 0.5 + 0.5) * c[..., 3]


def barycentrics(P, tri):
    """(u, v) of P in the plane of tri (..., 3, 3): P = p1 (1 - u - v) + p2 u + p3 v (least squares)."""
    P = np.asarray(P, np.float64)
    tri = np.asarray(tri, np.float64)
    e1, e2, q = tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :], P - tri[..., 0, :]
    a, b, c = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    d, e = (q * e1).sum(-1), (q * e2).sum(-1)
    det = a * c - b * b
    return (c * d - b * e) / det, (a * e - b * d) / det


def displacement(P, cur, prev):
    """D at P: (d1 w0 + d2 u) + d3 v with d_j = prev_j - cur_j and w0 = (1 - u) - v."""
    cur = np.asarray(cur, np.float64)
    dd = np.asarray(prev, np.float64) - cur
    u, v = barycentrics(P, cur)
    w0 = (1.0 - u) - v
    return (dd[..., 0, :] * w0[..., None] + dd[..., 1, :] * u[..., None]) + dd[..., 2, :] * v[..., None]


def motion_from_displacement(P, D, M, PV):
    """The motion texel's xyz for surface points P (..., 3) that were at P + D one frame ago."""
    P = np.asarray(P, np.float64)
    prevP = P + np.asarray(D, np.float64)
    xy = proj(M, P) - proj(PV, prevP)
    z = lin_z(PV, prevP) - lin_z(PV, P)
    return np.concatenate([xy, z[..., None]], axis=-1)


def motion(P, cur, prev, M, PV):
    """The motion texel's xyz for surface points P on triangles `cur` (..., 3, 3) that were at `prev`."""
    return motion_from_displacement(P, displacement(P, cur, prev), M, PV)

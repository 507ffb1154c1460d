"""The ray queries' definition (include/ptsvgf.h "ray queries"): hitBVH (path_tracing.frag:372-424) over the encoded
buffers, restated in Python with every box and triangle test done by the oracle's exported hitAABB / hitTriangle
(oracle_ref.lib().orc_hit_aabb / orc_hit_triangle). It keeps the reference's push order (:408-420: the nearer child
is popped first, the right one on equal distances), the strict '<' of hitArray and hitBVH, and INF.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_ref as O

INF = np.float32(114514.0)  # path_tracing.frag's INF, what a miss reports as t
HIT_DTYPE = np.dtype({"names": ["t", "tri", "obj", "inside", "P"], "formats": ["<f4", "<i4", "<i4", "<i4", ("<f4", (3,))],
                      "offsets": [0, 4, 8, 12, 16], "itemsize": 32})
_fp = C.POINTER(C.c_float)


def obj_of(tri_enc: np.ndarray, tri: int) -> int:
    """(int)objIndex of a record (float 42); -1 for a value that is not finite or lies outside +-2^24."""
    f = np.float32(tri_enc[tri, 42])
    return int(f) if np.isfinite(f) and abs(float(f)) <= 16777216.0 else -1


class Walker:
    """hitBVH over (tri_enc (n, 45), node_enc (m, 12)) float32 arrays: node 0 a dummy, the root node 1."""

    def __init__(self, tri_enc, node_enc):
        self.tri = np.ascontiguousarray(tri_enc, np.float32).reshape(-1, 45)
        self.node = np.ascontiguousarray(node_enc, np.float32).reshape(-1, 12)
        self.L = O.lib()
        self._tp = self.tri.ctypes.data
        self._np = self.node.ctypes.data
        self._out = (C.c_float * 5)()
        # getBVHNode's (int) casts (:193-210)
        self.left = self.node[:, 0].astype(np.int64).tolist()
        self.right = self.node[:, 1].astype(np.int64).tolist()
        self.n = self.node[:, 3].astype(np.int64).tolist()
        self.index = self.node[:, 4].astype(np.int64).tolist()

    def _aabb(self, S, d, k: int) -> float:
        base = self._np + 48 * k
        return self.L.orc_hit_aabb(S, d, C.cast(base + 24, _fp), C.cast(base + 36, _fp))

    def _tri(self, S, d, i: int):
        base = self._tp + 180 * i
        hit = self.L.orc_hit_triangle(S, d, C.cast(base, _fp), C.cast(base + 36, _fp), self._out)
        return bool(hit), np.float32(self._out[0]), self._out[4] != 0.0

    def closest(self, origin, direction):
        """(t, tri, inside) of hitBVH's result; (INF, -1, False) for a miss."""
        o = np.ascontiguousarray(origin, np.float32)
        dd = np.ascontiguousarray(direction, np.float32)
        S, d = o.ctypes.data_as(_fp), dd.ctypes.data_as(_fp)
        best_t, best, best_in = INF, -1, False
        stack = [1]                                            # :381
        while stack:
            top = stack.pop()
            if self.n[top] > 0:                                # a leaf: hitArray (:298-313)
                lt, li, lin = INF, -1, False
                for i in range(self.index[top], self.index[top] + self.n[top]):
                    hit, t, inside = self._tri(S, d, i)
                    if hit and t < lt:
                        lt, li, lin = t, i, inside
                if li >= 0 and lt < best_t:                    # :391
                    best_t, best, best_in = lt, li, lin
                continue
            d1 = d2 = float(INF)
            if self.left[top] > 0:
                d1 = self._aabb(S, d, self.left[top])
            if self.right[top] > 0:
                d2 = self._aabb(S, d, self.right[top])
            if d1 > 0 and d2 > 0:                              # :408-420
                if d1 < d2:
                    stack += [self.right[top], self.left[top]]
                else:
                    stack += [self.left[top], self.right[top]]
            elif d1 > 0:
                stack.append(self.left[top])
            elif d2 > 0:
                stack.append(self.right[top])
        return best_t, int(best), bool(best_in)

    def hits(self, rays) -> np.ndarray:
        """pt_rays_closest's records for rays (n, 8) float32: P = S + d * t in float32, two operations."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], HIT_DTYPE)
        for k, r in enumerate(rays):
            t, tri, inside = self.closest(r[0:3], r[4:7])
            if tri < 0:
                out[k] = (INF, -1, -1, 0, (0.0, 0.0, 0.0))
                continue
            with np.errstate(all="ignore"):
                P = (r[0:3] + (r[4:7] * np.float32(t)).astype(np.float32)).astype(np.float32)
            out[k] = (t, tri, obj_of(self.tri, tri), 1 if inside else 0, tuple(P))
        return out

    def occluded(self, rays, hits=None) -> np.ndarray:
        """pt_rays_occluded's verdicts, derived from the closest hit: it exists and its t < tmax (float 7)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        h = self.hits(rays) if hits is None else hits
        with np.errstate(invalid="ignore"):
            return (h["tri"] >= 0) & (h["t"] < rays[:, 7])


def primary_dir(cameraRotate, W: int, H: int, aspect_corrected: bool, x: int, y: int) -> np.ndarray:
    """primary_dir (csrc/wf_common.h; path_tracing.frag's main) restated in float32, operation by operation. Python's
    normalize need not match the device's last bit (inversesqrt), so tests compare it away from silhouettes."""
    f = np.float32
    m = np.asarray(cameraRotate, np.float32).reshape(16)
    pixx = f(f(2 * x + 1) / f(W)) - f(1.0)
    pixy = f(f(2 * y + 1) / f(H)) - f(1.0)
    if aspect_corrected:
        pixx = f(pixx * f(f(W) / f(H)))
    v = np.empty(3, np.float32)
    for c in range(3):
        a = f(f(m[c] * pixx) + f(m[4 + c] * pixy))
        b = f(f(m[8 + c] * f(-1.0)) + f(m[12 + c] * f(0.0)))
        v[c] = f(a + b)
    n2 = f(f(f(v[0] * v[0]) + f(v[1] * v[1])) + f(v[2] * v[2]))
    return (v * f(f(1.0) / np.sqrt(n2))).astype(np.float32)


def bits(h: np.ndarray) -> np.ndarray:
    """The eight 32-bit words of every hit record."""
    return np.ascontiguousarray(h).view(np.uint32).reshape(-1, 8)

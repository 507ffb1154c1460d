"""Definition of adaptive sample counts (DESIGN.md "Adaptive sample counts") over spp_ref.py's per-sample colours, in
float32 with one rounding per operation and no contraction.

  counts    a uint8 c per frame pixel; the pixel takes n = min(max(c, 1), N) samples (0 counts as 1, 255 as N).
            Sample s exists iff s < n and is spp_ref's sample s: its counter is F * N + s with the uniform N, not n.
  colour    rgb = (...(c_0 + c_1) + ... + c_{n-1}) / float(n), alpha 1; then the accumulate mix as spp_ref's.
            Emission and albedo are sample 0's.
  stats     l_s = lum(c_s.rgb), svgf_reproject.frag's luminance: (0.2125 r + 0.7154 g) + 0.0721 b.
            n < 2: (l_0, -1). Otherwise m = (...(l_0 + l_1) + ...) / float(n), M2 = sum_s (l_s - m) * (l_s - m) in
            sample order, v = M2 / float(n - 1).
  derive    the next counts from (stats, this frame's gMotion and gNormalAndLinearZ, lag L, tolerance tau, N):
            derive_counts below.
TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

from spp_ref import mix_last

f32 = np.float32


def effective(counts, N: int) -> np.ndarray:
    return np.minimum(np.maximum(np.asarray(counts).astype(np.int32), 1), int(N))


def lum(rgb) -> np.ndarray:
    rgb = np.asarray(rgb, f32)
    with np.errstate(all="ignore"):
        a = (f32(0.2125) * rgb[..., 0]).astype(f32)
        b = (f32(0.7154) * rgb[..., 1]).astype(f32)
        c = (f32(0.0721) * rgb[..., 2]).astype(f32)
        return ((a + b).astype(f32) + c).astype(f32)


def fold_counts(samples, counts) -> np.ndarray:
    """The colour rule: `samples` a list of N (..., 4) float32 sample colours, `counts` the raw uint8 plane."""
    N = len(samples)
    n = effective(counts, N)
    total = np.array(samples[0][..., :3], f32)
    with np.errstate(all="ignore"):
        for s in range(1, N):
            nxt = (total + np.asarray(samples[s][..., :3], f32)).astype(f32)
            total = np.where((s < n)[..., None], nxt, total)
        out = np.empty(samples[0].shape, f32)
        out[..., :3] = (total / n.astype(f32)[..., None]).astype(f32)
    out[..., 3] = f32(1.0)
    return out


def stats_counts(samples, counts) -> np.ndarray:
    """(..., 2) float32: the pair (m, v) per pixel."""
    N = len(samples)
    n = effective(counts, N)
    ls = [lum(c[..., :3]) for c in samples]
    with np.errstate(all="ignore"):
        m = np.array(ls[0], f32)
        for s in range(1, N):
            m = np.where(s < n, (m + ls[s]).astype(f32), m)
        m = (m / n.astype(f32)).astype(f32)
        m2 = np.zeros(m.shape, f32)
        for s in range(N):
            d = (ls[s] - m).astype(f32)
            m2 = np.where(s < n, (m2 + (d * d).astype(f32)).astype(f32), m2)
        v = (m2 / np.maximum(n - 1, 1).astype(f32)).astype(f32)
    out = np.empty(m.shape + (2,), f32)
    out[..., 0] = np.where(n < 2, ls[0], m)
    out[..., 1] = np.where(n < 2, f32(-1.0), v)
    return out


def need(m, v, tau, N: int) -> np.ndarray:
    """r of one statistics texel (step 3 of derive_counts), elementwise, int32."""
    m, v = np.asarray(m, f32), np.asarray(v, f32)
    tau = f32(tau)
    with np.errstate(all="ignore"):
        none = (v < 0) | np.isnan(m) | np.isnan(v)
        d = (tau * np.maximum(m, f32(1e-4))).astype(f32)
        k = np.ceil((v / (d * d).astype(f32)).astype(f32)).astype(f32)
        small = k < f32(N)  # False for NaN
        ki = np.where(small, k, f32(0)).astype(np.int32)
    return np.where(none | ~small, np.int32(N), np.maximum(2, ki)).astype(np.int32)


def derive_counts(stats, motion, nd, L, tau, N: int) -> np.ndarray:
    """stats (H, W, 2), motion (H, W, >= 2) (gMotion.xy), nd (H, W, 4) (gNormalAndLinearZ) -> (H, W) uint8.
    1. nd.w == 1 (background now): 1.
    2. fx = (float(x) + 0.5) - (L * motion.x) * float(W), fy likewise with H; q = (floor fx, floor fy). Non-finite fx
       or fy, or q outside the frame: N.
    3. r(q') = N if v < 0 or m or v is NaN; else d = tau * max(m, 1e-4), k = ceil(v / (d * d)); r = N if
       !(k < float(N)) else max(2, int(k)).
    4. the maximum of r over the texels q' of the 3 x 3 block around q inside the frame."""
    stats, motion, nd = np.asarray(stats, f32), np.asarray(motion, f32), np.asarray(nd, f32)
    H, W = nd.shape[:2]
    L = f32(L)
    r = need(stats[..., 0], stats[..., 1], tau, N)
    pad = np.zeros((H + 2, W + 2), np.int32)
    pad[1:-1, 1:-1] = r
    block = np.zeros((H, W), np.int32)  # the 3 x 3 maximum inside the frame (r >= 2 > 0)
    for dy in range(3):
        for dx in range(3):
            block = np.maximum(block, pad[dy:dy + H, dx:dx + W])
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        fx = ((xs.astype(f32) + f32(0.5)) - ((L * motion[..., 0]).astype(f32) * f32(W)).astype(f32)).astype(f32)
        fy = ((ys.astype(f32) + f32(0.5)) - ((L * motion[..., 1]).astype(f32) * f32(H)).astype(f32)).astype(f32)
        inside = np.isfinite(fx) & np.isfinite(fy) & (fx >= 0) & (fx < f32(W)) & (fy >= 0) & (fy < f32(H))
        qx = np.where(inside, np.floor(fx), 0).astype(np.int64)
        qy = np.where(inside, np.floor(fy), 0).astype(np.int64)
    out = np.where(inside, block[qy, qx], np.int32(N))
    out = np.where(nd[..., 3] == f32(1.0), np.int32(1), out)
    return out.astype(np.uint8)


def adaptive_ref(samples, counts, F: int = 0, accumulate=False, last_frame=None, bind_stats=True):
    """(colour, stats) of a draw whose per-sample colours are `samples` (spp_ref's, whole frames)."""
    color = fold_counts(samples, counts)
    if accumulate and last_frame is not None:
        color = mix_last(np.asarray(last_frame, f32), color, F)
    return color, (stats_counts(samples, counts) if bind_stats else None)

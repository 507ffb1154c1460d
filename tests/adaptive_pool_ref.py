"""Definition of pooled adaptive sample counts (DESIGN.md "Pooled sample statistics"; pt_sample_counts_pool), in
float32 with one rounding per operation and no contraction, beside adaptive_ref.py.

A pool plane holds one float4 (m, v, w, z) per frame pixel: mean and unbiased variance of the pooled luminances, the
pooled sample weight (w = 0: empty) and gNormalAndLinearZ.z of the pixel when the texel was written.

One step at a frame takes (any of the first three may be None)
  stats        the slot's previous draw's statistics plane (H, W, 2), in that draw's pixel coordinates
  counts_prev  the count plane that draw read (H, W) uint8, and N_prev, that draw's spp
  pool_in      the pool plane written at that draw's step (H, W, 4)
  motion, nd   this frame's gMotion (H, W, >= 2) and gNormalAndLinearZ (H, W, 4)
  L, w_max >= 2, zeta > 0, rule (0 relative, 1 absolute), tau > 0, N in 2 .. 8
and gives (pool_out, counts): pool_step below.

Texel T(p) of a frame pixel p, with z = nd(p).z:
  1. nd(p).w == 1: background, T = (0, 0, 0, z).
  2. fx = (float(x) + 0.5) - (L * motion.x) * float(W), fy likewise with H (adaptive_ref.derive_counts step 2);
     q = (floor fx, floor fy). Non-finite fx or fy, or q outside the frame: empty, T = (0, 0, 0, z).
  3. history a = pool_in[q]. pool_in bound and !(|a.z - z| <= zeta * max(|z|, 1e-4)): empty (a NaN fails the test;
     stats[q] is of another surface too). Otherwise a is valid iff pool_in is bound, a.w >= 1, a.m and a.v finite.
  4. new samples: n_s = min(max(counts_prev[q], 1), N_prev) (N_prev without a plane); (m_s, v_s) = stats[q]; s is
     valid iff stats is bound, m_s is finite and (n_s < 2 or v_s is finite and >= 0); v_s' = v_s if n_s >= 2 else 0.
  5. neither valid: empty. Only s: (m_s, v_s', float(n_s)). Only a: a. Both (Chan's pairwise update), in this order:
       w = a.w + n_s;  d = m_s - a.m;  m = a.m + d * (n_s / w)
       M2 = (a.v * (a.w - 1) + v_s' * (n_s - 1)) + (d * d) * ((a.w * n_s) / w)
       v = M2 / (w - 1);  w = min(w, w_max)
     and z = nd(p).z in every case.
Need r(T): background 0 (it takes no part in the maximum); !(w >= 2): N; else d = tau * max(m, 1e-4) (relative; a NaN
  m stays NaN) or d = tau (absolute), k = ceil(v / (d * d)), r = N if !(k < float(N)) else max(1, int(k)) (1 for k < 1).
Outputs: pool_out[x] = T(x); counts[x] = 1 on the background, elsewhere the maximum of r(T(p)) over the p of the 3 x 3
  block around x inside the frame (this frame's coordinates; each p reprojects for itself).
TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
RELATIVE, ABSOLUTE = 0, 1


def combine(a_m, a_v, a_w, m_s, v_s, n_s):
    """Step 5's pairwise update of valid a and s, elementwise: (m, v, w) before the cap on w. n_s as float32."""
    a_m, a_v, a_w = np.asarray(a_m, f32), np.asarray(a_v, f32), np.asarray(a_w, f32)
    m_s, v_s, n_s = np.asarray(m_s, f32), np.asarray(v_s, f32), np.asarray(n_s, f32)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        w = (a_w + n_s).astype(f32)
        d = (m_s - a_m).astype(f32)
        m = (a_m + (d * (n_s / w).astype(f32)).astype(f32)).astype(f32)
        within = ((a_v * (a_w - one).astype(f32)).astype(f32) + (v_s * (n_s - one).astype(f32)).astype(f32)).astype(f32)
        between = ((d * d).astype(f32) * ((a_w * n_s).astype(f32) / w).astype(f32)).astype(f32)
        v = ((within + between).astype(f32) / (w - one).astype(f32)).astype(f32)
    return m, v, w


def need_pool(m, v, w, rule: int, tau, N: int) -> np.ndarray:
    """r of surface texels (m, v, w), elementwise, int32 (the background's 0 is the caller's)."""
    m, v, w = np.asarray(m, f32), np.asarray(v, f32), np.asarray(w, f32)
    tau = f32(tau)
    with np.errstate(all="ignore"):
        d = np.full(m.shape, tau, f32) if rule == ABSOLUTE else (tau * np.maximum(m, f32(1e-4))).astype(f32)
        k = np.ceil((v / (d * d).astype(f32)).astype(f32)).astype(f32)
        small = k < f32(N)  # False for NaN
        ki = np.where(small & (k >= f32(1.0)), k, f32(1.0)).astype(np.int32)
    return np.where(~(w >= f32(2.0)) | ~small, np.int32(N), ki).astype(np.int32)


def pool_texels(stats, counts_prev, N_prev: int, pool_in, motion, nd, L, w_max, zeta):
    """(T, background): T (H, W, 4) float32, background (H, W) bool."""
    motion, nd = np.asarray(motion, f32), np.asarray(nd, f32)
    H, W = nd.shape[:2]
    L, w_max, zeta = f32(L), f32(w_max), f32(zeta)
    z = nd[..., 2]
    bg = nd[..., 3] == f32(1.0)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        fx = ((xs.astype(f32) + f32(0.5)) - ((L * motion[..., 0]).astype(f32) * f32(W)).astype(f32)).astype(f32)
        fy = ((ys.astype(f32) + f32(0.5)) - ((L * motion[..., 1]).astype(f32) * f32(H)).astype(f32)).astype(f32)
        inside = np.isfinite(fx) & np.isfinite(fy) & (fx >= 0) & (fx < f32(W)) & (fy >= 0) & (fy < f32(H))
        qx = np.where(inside, np.floor(fx), 0).astype(np.int64)
        qy = np.where(inside, np.floor(fy), 0).astype(np.int64)
        live = inside & ~bg
        # 3. the history
        if pool_in is not None:
            a = np.asarray(pool_in, f32)[qy, qx]
            near = np.abs((a[..., 3] - z).astype(f32)) <= (zeta * np.maximum(np.abs(z), f32(1e-4))).astype(f32)
            live &= near  # (False for a NaN on either side)
            a_ok = live & (a[..., 2] >= f32(1.0)) & np.isfinite(a[..., 0]) & np.isfinite(a[..., 1])
        else:
            a = np.zeros((H, W, 4), f32)
            a_ok = np.zeros((H, W), bool)
        # 4. the new samples
        if counts_prev is not None:
            n_i = np.minimum(np.maximum(np.asarray(counts_prev).astype(np.int32)[qy, qx], 1), int(N_prev))
        else:
            n_i = np.full((H, W), int(N_prev), np.int32)
        n_s = n_i.astype(f32)
        if stats is not None:
            st = np.asarray(stats, f32)[qy, qx]
            m_s, v_s = st[..., 0], st[..., 1]
            s_ok = live & np.isfinite(m_s) & ((n_i < 2) | (np.isfinite(v_s) & (v_s >= 0)))
            v_s = np.where(n_i >= 2, v_s, f32(0.0)).astype(f32)
        else:
            m_s = v_s = np.zeros((H, W), f32)
            s_ok = np.zeros((H, W), bool)
        # 5. combine
        m, v, w = combine(a[..., 0], a[..., 1], a[..., 2], m_s, v_s, n_s)
        w = np.minimum(w, w_max)
    both, only_s, only_a = a_ok & s_ok, s_ok & ~a_ok, a_ok & ~s_ok
    T = np.zeros((H, W, 4), f32)
    for i, (vb, vs) in enumerate(((m, m_s), (v, v_s), (w, n_s))):
        T[..., i] = np.select([both, only_s, only_a], [vb, vs, a[..., i]], f32(0.0))
    T[..., 3] = z
    return T, bg


def pool_step(stats, counts_prev, N_prev: int, pool_in, motion, nd, L, w_max, zeta, rule: int, tau, N: int):
    """One step: (pool_out (H, W, 4) float32, counts (H, W) uint8)."""
    T, bg = pool_texels(stats, counts_prev, N_prev, pool_in, motion, nd, L, w_max, zeta)
    H, W = bg.shape
    r = np.where(bg, np.int32(0), need_pool(T[..., 0], T[..., 1], T[..., 2], rule, tau, N))
    pad = np.zeros((H + 2, W + 2), np.int32)
    pad[1:-1, 1:-1] = r
    block = np.zeros((H, W), np.int32)
    for dy in range(3):
        for dx in range(3):
            block = np.maximum(block, pad[dy:dy + H, dx:dx + W])
    return T, np.where(bg, np.int32(1), block).astype(np.uint8)

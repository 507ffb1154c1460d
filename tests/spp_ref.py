"""Definition of a path-tracing draw with `spp` = N samples per pixel (DESIGN.md "Samples per pixel"), in float32
with one rounding per operation, over the CPU oracle's path tracer (oracle_ref.OracleScene.path_trace).

A draw with the uniforms frameCounter = F and spp = N (1 <= N <= 8):

  samples   sample s = 0 .. N-1 is the reference's main() (path_tracing.frag:1056-1128) with its frameCounter
            replaced by Fs = F * N + s (uint32, wrapping) wherever that path reads it (the seed :433-436, both
            sobolVec2(frameCounter + 1u, ...)), accumulation off: its colour c_s carries the clamp to
            clamp_threshold and the NaN -> 0 rule (:1110-1113)
  colour    sum = c_0; for s = 1 .. N-1: sum = sum + c_s (per channel, in that order); rgb = sum / float(N); a = 1
  accumulate  when the draw's accumulate is on: rgb = mix(lastFrame.rgb, rgb, 1.0 / float(F + 1u)) afterwards, with
            the frame's own counter F (:1116-1119)
  emission, albedo  sample 0's; the primary ray does not depend on the sample (:1060-1062 computes the jitter and
            never applies it), so every sample's are the same bits, which is asserted here

N = 1 is the oracle's own draw bit for bit (c / 1.0f == c; NaN never reaches the division).
TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import numpy as np

MAX_SPP = 8
f32 = np.float32


def sample_counter(F: int, N: int, s: int) -> int:
    return (F * N + s) & 0xFFFFFFFF


def fold_mean(colors) -> np.ndarray:
    """The colour rule on a list of (..., 4) float32 sample colours: the rgb mean in sample order, alpha 1."""
    n = len(colors)
    total = np.array(colors[0][..., :3], f32)
    with np.errstate(all="ignore"):
        for c in colors[1:]:
            total = (total + np.asarray(c[..., :3], f32)).astype(f32)
        out = np.empty(colors[0].shape, f32)
        out[..., :3] = (total / f32(n)).astype(f32)
    out[..., 3] = f32(1.0)
    return out


def mix_last(last, color, F: int) -> np.ndarray:
    """mix(lastFrame.rgb, color.rgb, 1.0 / float(F + 1u)): GLSL's x * (1 - a) + y * a in float32; alpha kept."""
    a = f32(1.0) / f32((F + 1) & 0xFFFFFFFF)
    out = np.array(color, f32)
    with np.errstate(all="ignore"):
        x = (np.asarray(last[..., :3], f32) * (f32(1.0) - a)).astype(f32)
        y = (np.asarray(color[..., :3], f32) * a).astype(f32)
        out[..., :3] = (x + y).astype(f32)
    return out


def spp_ref(oscene, W, H, F, N, eye, cameraRotate, clamp_threshold=10.0, max_depth=2, aspect_corrected=False,
            accumulate=False, last_frame=None, rows=None, use_normal_map=False, samples=None, **kw):
    """(colour, emission, albedo) of the draw, each (H, W, 4) float32; rows outside `rows` stay zero as the oracle
    leaves them. `samples` (a list) receives the per-sample colours."""
    if int(N) != N or not 1 <= N <= MAX_SPP:
        raise ValueError(f"spp must lie in 1 .. {MAX_SPP}, got {N!r}")
    cols, em, al = [], None, None
    for s in range(N):
        c, e, a = oscene.path_trace(W, H, sample_counter(F, N, s), eye, cameraRotate, clamp_threshold, max_depth,
                                    aspect_corrected, accumulate=False, rows=rows, use_normal_map=use_normal_map,
                                    **kw)
        if s == 0:
            em, al = e, a
        else:  # the primary hit is the sample's own only in name
            assert np.array_equal(e.view(np.uint32), em.view(np.uint32)), ("emission differs in sample", s)
            assert np.array_equal(a.view(np.uint32), al.view(np.uint32)), ("albedo differs in sample", s)
        cols.append(c)
    if samples is not None:
        samples.extend(cols)
    y0, y1 = rows if rows else (0, H)
    color = np.zeros((H, W, 4), f32)
    color[y0:y1] = fold_mean([c[y0:y1] for c in cols])
    if accumulate and last_frame is not None:
        color[y0:y1] = mix_last(np.asarray(last_frame, f32)[y0:y1], color[y0:y1], F)
    return color, em, al

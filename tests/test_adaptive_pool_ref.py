"""The definition of pooled adaptive sample counts (tests/adaptive_pool_ref.py): the pairwise combination against
numpy's float64 statistics, the cap on the weight, depth rejection and silhouettes, both rules, invalid inputs, and
the C and Python boundary of the feature. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from adaptive_pool_ref import ABSOLUTE, RELATIVE, combine, need_pool, pool_step, pool_texels

f32 = np.float32
H, W = 5, 7
EPS = float(np.finfo(f32).eps)


def _planes(h=H, w=W, m=1.0, v=0.0, z=2.0):
    stats = np.empty((h, w, 2), f32)
    stats[..., 0], stats[..., 1] = m, v
    motion = np.zeros((h, w, 4), f32)
    nd = np.zeros((h, w, 4), f32)
    nd[..., 2], nd[..., 3] = z, 0.5
    return stats, motion, nd


def _pool(h=H, w=W, m=1.0, v=0.0, wt=4.0, z=2.0):
    p = np.empty((h, w, 4), f32)
    p[..., 0], p[..., 1], p[..., 2], p[..., 3] = m, v, wt, z
    return p


def _mv(x):
    """(mean, unbiased variance, count) of a float32 sample set, float32 as a draw's statistics hold them."""
    x = np.asarray(x, np.float64)
    return f32(x.mean()), f32(x.var(ddof=1) if len(x) > 1 else 0.0), f32(len(x))


# ------------------------------------------------------------- combine by hand ---
@pytest.mark.parametrize("na,nb", [(4, 4), (7, 2), (2, 8), (1, 3), (5, 1), (1, 1), (30, 4)])
def test_combine_equals_the_statistics_of_the_union(na, nb):
    """Pooling (m, v, w) of A with the statistics of B is mean and var(ddof=1) of A u B. The bound: the same formula
    in float64 on the same float32 inputs differs from the float32 evaluation by the roundings of its ~6 operations
    per output, each relative to the largest term (all terms of M2 are >= 0, so none cancels): 8 eps of the scale."""
    rng = np.random.default_rng(na * 16 + nb)
    A = rng.random(na).astype(f32) * f32(2.0)
    B = (rng.random(nb).astype(f32) * f32(0.5) + f32(1.0)).astype(f32)
    am, av, aw = _mv(A)
    bm, bv, bn = _mv(B)
    m, v, w = combine(am, av, aw, bm, bv, bn)
    assert m.dtype == v.dtype == w.dtype == f32 and w == na + nb
    # the float64 restatement on the float32 inputs
    a_m, a_v, a_w, m_s, v_s, n_s = (float(t) for t in (am, av, aw, bm, bv, bn))
    w64 = a_w + n_s
    d = m_s - a_m
    m64 = a_m + d * (n_s / w64)
    M2 = (a_v * (a_w - 1) + v_s * (n_s - 1)) + (d * d) * ((a_w * n_s) / w64)
    v64 = M2 / (w64 - 1)
    assert abs(float(m) - m64) <= 8 * EPS * max(abs(a_m), abs(m_s))
    assert abs(float(v) - v64) <= 8 * EPS * max(v64, 1e-30)
    # ... and the restatement is the union's statistics, up to the float32 rounding of its four inputs
    U = np.concatenate([A, B]).astype(np.float64)
    assert abs(m64 - U.mean()) <= 4 * EPS * 2.0
    assert abs(v64 - U.var(ddof=1)) <= 16 * EPS * max(U.var(ddof=1), 1.0)


def test_step_combines_history_and_new_samples():
    """The step's texel for a.w = 1 (a one-sample history) and n_s = 1 (a one-sample draw, whose v_s = -1 counts as
    0), against the union's statistics."""
    rng = np.random.default_rng(2)
    for na, nb in ((1, 3), (3, 1), (1, 1), (6, 4)):
        A, B = rng.random(na).astype(f32), rng.random(nb).astype(f32)
        am, av, aw = _mv(A)
        bm, bv, _ = _mv(B)
        stats, motion, nd = _planes(m=bm, v=bv if nb > 1 else -1.0)
        counts = np.full((H, W), nb, np.uint8)
        T, cnt = pool_step(stats, counts, 8, _pool(m=am, v=av, wt=aw), motion, nd, 1.0, 64.0, 0.1, RELATIVE, 1.0, 8)
        U = np.concatenate([A, B]).astype(np.float64)
        assert T[2, 3, 2] == na + nb and T[2, 3, 3] == f32(2.0)
        assert abs(float(T[2, 3, 0]) - U.mean()) < 1e-6
        assert abs(float(T[2, 3, 1]) - U.var(ddof=1)) < 1e-6
        assert np.all(T == T[0, 0])


# ------------------------------------------------------------------ the cap on w ---
def test_weight_stops_at_w_max_and_the_pool_converges():
    rng = np.random.default_rng(5)
    sigma2 = 0.25  # the population: normal, mean 1, variance 0.25
    n, w_max = 4, 16.0
    _, motion, nd = _planes(h=32, w=32)
    pool, err = None, []
    for step in range(16):
        x = (rng.standard_normal((n, 32, 32)) * 0.5 + 1.0).astype(f32)
        stats = np.stack([x.mean(0), x.var(0, ddof=1)], -1).astype(f32)
        pool, _ = pool_step(stats, None, n, pool, motion, nd, 1.0, w_max, 0.1, RELATIVE, 1.0, n)
        assert np.all(pool[..., 2] == min(n * (step + 1), w_max))
        err.append(float(np.sqrt(np.mean((pool[..., 1].astype(np.float64) - sigma2) ** 2))))
    assert err[15] < err[0], err


# ---------------------------------------------------------------- depth rejection ---
def test_depth_test_is_relative_and_rejection_gives_n():
    stats, motion, nd = _planes(z=2.0)
    pool = _pool(z=2.0)
    pool[1, 1, 3] = 2.0 + 0.19   # |dz| <= 0.1 * 2: kept
    pool[1, 2, 3] = 2.0 + 0.21   # rejected
    pool[1, 3, 3] = 2.0 - 0.21
    pool[1, 4, 3] = np.nan       # a NaN fails the test
    nd[3, 3, 2] = 1e-6           # the floor on |z|: tolerance 0.1 * 1e-4
    pool[3, 3, 3] = 5e-6         # |dz| = 4e-6 <= 1e-5: kept
    nd[3, 5, 2] = 1e-6
    pool[3, 5, 3] = 2e-5         # |dz| = 1.9e-5: rejected
    T, cnt = pool_step(stats, None, 4, pool, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    rejected = np.zeros((H, W), bool)
    for y, x in ((1, 2), (1, 3), (1, 4), (3, 5)):
        rejected[y, x] = True
    assert np.all(T[rejected][:, :3] == 0)              # empty although stats[q] is valid: another surface
    assert np.all(T[~rejected][:, 2] == 8.0)            # 4 pooled + 4 new
    assert np.array_equal(T[..., 3], nd[..., 2])        # z is this frame's in every case
    want = np.ones((H, W), int)
    want[0:3, 1:6] = 4
    want[2:5, 4:7] = 4
    assert np.array_equal(cnt, want)
    nd2 = nd.copy()
    nd2[0, 0, 2] = np.nan        # ... on this frame's side too
    T2, cnt2 = pool_step(stats, None, 4, pool, motion, nd2, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    assert np.all(T2[0, 0, :3] == 0) and np.isnan(T2[0, 0, 3]) and cnt2[0, 0] == 4


def test_background_neighbour_does_not_raise_a_silhouette_but_a_noisy_one_does():
    stats, motion, nd = _planes()
    nd[2, 3, 3] = 1.0
    stats[2, 3] = (np.nan, -1.0)  # whatever the background's statistics say
    T, cnt = pool_step(stats, None, 4, _pool(), motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 8)
    assert np.all(cnt == 1) and np.all(T[2, 3] == (0, 0, 0, 2.0))
    stats[1, 1, 1] = 8.0  # m = 1: pooled with (1, 0, 4): v = 8 * 3 / 7 = 3.43 -> 4 at tau = 1
    T, cnt = pool_step(stats, None, 4, _pool(), motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 8)
    want = np.ones((H, W), int)
    want[0:3, 0:3] = 4
    assert np.array_equal(cnt, want)
    # an empty neighbour (no history, no samples) does: there is no estimate
    T, cnt = pool_step(None, None, 4, None, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 8)
    want = np.full((H, W), 8)
    want[2, 3] = 1
    assert np.array_equal(cnt, want) and np.all(T[..., :3] == 0)


def test_history_follows_the_motion_vectors():
    stats, motion, nd = _planes()
    pool = _pool()
    stats[2, 1, 1] = 8.0
    motion[..., 0] = 1.0 / W  # everything moved one texel right per frame, two frames ago: x looks at x - 2
    T, cnt = pool_step(stats, None, 4, pool, motion, nd, 2.0, 32.0, 0.1, RELATIVE, 1.0, 8)
    want = np.ones((H, W), int)
    want[1:4, 2:5] = 4
    want[:, :3] = 8  # x = 0, 1 came from outside the frame (empty) and raise x = 2
    assert np.array_equal(cnt, want)
    assert np.all(T[:, :2, :3] == 0) and np.all(T[:, 2:, 2] == 8.0)


# ------------------------------------------------------------------- both rules ---
def test_rules_by_hand_and_monotone_in_tau():
    one = lambda m, v, w, rule, tau, N=8: int(need_pool(f32(m), f32(v), f32(w), rule, tau, N))  # noqa: E731
    assert one(1.0, 0.0, 2.0, RELATIVE, 0.1) == 1      # v = 0 and w >= 2: one sample
    assert one(1.0, 0.0, 2.0, ABSOLUTE, 0.1) == 1
    assert one(1.0, 0.0, 1.0, RELATIVE, 0.1) == 8      # w < 2: no estimate
    assert one(1.0, 0.0, 0.0, ABSOLUTE, 0.1) == 8
    assert one(1.0, 0.03, 4.0, RELATIVE, 0.1) == 3     # 0.03 / 0.01
    assert one(4.0, 0.03, 4.0, RELATIVE, 0.1) == 1     # 0.03 / 0.16
    assert one(4.0, 0.03, 4.0, ABSOLUTE, 0.1) == 3     # the absolute rule does not look at m
    assert one(0.01, 0.03, 4.0, ABSOLUTE, 0.1) == 3
    assert one(0.01, 0.03, 4.0, RELATIVE, 0.1) == 8    # the relative rule sends samples to the dark pixel
    assert one(1.0, 0.079, 4.0, RELATIVE, 0.1) == 8    # ceil(7.9) = 8: not < N
    assert one(1.0, 0.069, 4.0, ABSOLUTE, 0.1) == 7
    assert one(0.0, 1e-9, 4.0, RELATIVE, 0.1) == 8     # the floor on m: d = 1e-5, need 10
    assert one(1.0, -1.0, 4.0, RELATIVE, 0.1) == 1     # a negative k is held to 1
    assert one(1.0, -1e30, 4.0, ABSOLUTE, 1e-4) == 1
    assert one(np.nan, 0.0, 4.0, RELATIVE, 0.1) == 8   # a NaN m stays a NaN
    assert one(1.0, np.inf, 4.0, ABSOLUTE, 0.1) == 8
    rng = np.random.default_rng(3)
    m = rng.random(4096, dtype=f32) * f32(2.0) + f32(0.5)  # (away from the relative rule's floor on m)
    v = rng.random(4096, dtype=f32) * f32(0.2)
    w = np.full(4096, 4.0, f32)
    for rule in (RELATIVE, ABSOLUTE):
        prev = None
        for tau in (0.05, 0.1, 0.2, 0.4, 0.8, 4.0):
            r = need_pool(m, v, w, rule, tau, 8)
            assert r.min() >= 1 and r.max() <= 8
            if prev is not None:
                assert np.all(r <= prev)
            prev = r
        assert prev.max() == 1 and need_pool(m, v, w, rule, 0.05, 8).max() == 8


def test_surface_with_zero_variance_gets_one_sample():
    stats, motion, nd = _planes()
    for rule in (RELATIVE, ABSOLUTE):
        _, cnt = pool_step(stats, None, 4, None, motion, nd, 1.0, 8.0, 0.1, rule, 0.5, 4)
        assert np.all(cnt == 1)


# --------------------------------------------------------------- invalid inputs ---
@pytest.mark.parametrize("bad", [(np.nan, 0.5), (np.inf, 0.5), (1.0, np.nan), (1.0, np.inf), (1.0, -1.0)])
def test_invalid_statistics_leave_the_history(bad):
    stats, motion, nd = _planes()
    stats[2, 3] = bad
    pool = _pool(m=3.0, v=0.0, wt=5.0)
    T, cnt = pool_step(stats, None, 4, pool, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    assert np.array_equal(T[2, 3], np.array([3.0, 0.0, 5.0, 2.0], f32))  # only a valid: a
    assert T[2, 2, 2] == 9.0
    T, cnt = pool_step(stats, None, 4, None, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    assert np.all(T[2, 3, :3] == 0)  # neither valid: empty, N around it
    want = np.ones((H, W), int)
    want[1:4, 2:5] = 4
    assert np.array_equal(cnt, want)


def test_one_sample_statistics_need_no_variance():
    stats, motion, nd = _planes(m=0.75, v=-1.0)
    counts = np.ones((H, W), np.uint8)
    counts[0, 0] = 0  # counts as 1
    T, cnt = pool_step(stats, counts, 4, None, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    assert np.all(T[..., :3] == np.array([0.75, 0.0, 1.0], f32)) and np.all(cnt == 4)
    T2, cnt2 = pool_step(stats, counts, 4, T, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    assert np.all(T2[..., :3] == np.array([0.75, 0.0, 2.0], f32)) and np.all(cnt2 == 1)
    counts[:] = 255  # N_prev samples: v = -1 is then no estimate
    T3, _ = pool_step(stats, counts, 4, None, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    assert np.all(T3[..., :3] == 0)


@pytest.mark.parametrize("bad", [(np.nan, 0.0, 4.0), (1.0, np.inf, 4.0), (1.0, 0.0, 0.0), (1.0, 0.0, 0.5),
                                 (1.0, 0.0, np.nan), (-np.inf, 0.0, 4.0)])
def test_invalid_history_leaves_the_new_samples(bad):
    stats, motion, nd = _planes(m=0.5, v=0.125)
    pool = _pool()
    pool[2, 3, :3] = bad
    T, _ = pool_step(stats, None, 4, pool, motion, nd, 1.0, 32.0, 0.1, RELATIVE, 1.0, 4)
    assert np.array_equal(T[2, 3], np.array([0.5, 0.125, 4.0, 2.0], f32))  # only s valid
    assert T[2, 2, 2] == 8.0


def test_bad_motion_and_off_frame_are_empty():
    stats, motion, nd = _planes()
    motion[0, 0, 0] = np.nan
    motion[0, 1, 1] = np.inf
    motion[0, 2, 0] = -np.inf
    motion[2, 2, 0] = 1.0        # fx = 2.5 - 7 < 0
    motion[2, 3, 1] = -1.0       # fy = 2.5 + 5 >= H
    motion[4, 6, 0] = -1.0 / W   # fx = 7.5: one texel past the right edge
    motion[3, 0, 0] = 0.5 / W    # fx = 0: inside
    T, bg = pool_texels(stats, None, 4, _pool(), motion, nd, 1.0, 32.0, 0.1)
    empty = np.zeros((H, W), bool)
    for y, x in ((0, 0), (0, 1), (0, 2), (2, 2), (2, 3), (4, 6)):
        empty[y, x] = True
    assert not bg.any()
    assert np.all(T[empty][:, :3] == 0) and np.all(T[~empty][:, 2] == 8.0) and np.all(T[..., 3] == 2.0)
    _, cnt = pool_step(stats, None, 4, _pool(), motion, nd, 1.0, 32.0, 0.1, ABSOLUTE, 1.0, 8)
    assert cnt[2, 2] == 8 and cnt[1, 1] == 8 and cnt[4, 0] == 1 and cnt[3, 0] == 1


# --------------------------------------------------- exports and refusals ---
def test_library_exports_and_header_declares_the_call():
    from ptsvgf import _lib, gl

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ptsvgf.h")).read()
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    assert re.search(r"\bint\s+pt_sample_counts_pool\s*\(", text)
    assert hasattr(lib, "pt_sample_counts_pool")
    assert "pt_sample_counts_pool" in _lib.exported_symbols()[0]
    assert callable(gl.sample_counts_pool)


def test_renderer_refuses_the_arguments():
    """The refusals come before the renderer touches the device (no scene, no library call)."""
    from ptsvgf.renderer import Renderer

    for kw, word in ((dict(adaptive_pool=8.0), "needs adaptive"),
                     (dict(spp=4, adaptive=1.0, adaptive_rule="absolute"), "needs adaptive_pool"),
                     (dict(spp=4, adaptive=1.0, adaptive_pool=1.5), ">= 2"),
                     (dict(spp=4, adaptive=1.0, adaptive_pool=float("nan")), ">= 2"),
                     (dict(spp=4, adaptive=1.0, adaptive_pool=8.0, adaptive_rule="both"), "adaptive_rule"),
                     (dict(spp=4, adaptive=1.0, adaptive_pool=8.0, adaptive_zeta=0.0), "adaptive_zeta")):
        with pytest.raises(ValueError, match=word):
            Renderer(None, 16, 16, **kw)
    assert Renderer._check_adaptive_pool(1.0, None, "relative", 0.1) is None
    assert Renderer._check_adaptive_pool(1.0, 8, "absolute", 0.1) == dict(wmax=8.0, rule=1, zeta=0.1)


def test_multi_rank_renderers_still_refuse_adaptive():
    from ptsvgf.dist import BandRenderer

    with pytest.raises(ValueError, match="adaptive"):
        BandRenderer(None, 16, 16, None, 0, 1, None, adaptive=0.5, adaptive_pool=8.0)

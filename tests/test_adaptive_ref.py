"""The definition of adaptive sample counts (tests/adaptive_ref.py): its own properties, hand-computed statistics
and derive cases, and the C boundary of the feature. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from adaptive_ref import adaptive_ref, derive_counts, effective, fold_counts, lum, need, stats_counts
from spp_ref import fold_mean

f32 = np.float32
H, W = 5, 7


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def samples():
    rng = np.random.default_rng(7)
    out = [rng.random((H, W, 4), dtype=f32) * f32(3.0) for _ in range(4)]
    for c in out:
        c[..., 3] = 1.0
    return out


# ------------------------------------------------------------- the fold ---
@pytest.mark.parametrize("c", [4, 255, 200])
def test_full_counts_are_the_plain_mean(samples, c):
    got = fold_counts(samples, np.full((H, W), c, np.uint8))
    assert np.array_equal(_bits(got), _bits(fold_mean(samples)))


@pytest.mark.parametrize("c", [1, 0])
def test_one_sample_is_sample_zero(samples, c):
    got = fold_counts(samples, np.full((H, W), c, np.uint8))
    assert np.array_equal(_bits(got[..., :3]), _bits(samples[0][..., :3]))
    assert np.all(got[..., 3] == 1.0)


def test_mixed_counts_fold_a_prefix(samples):
    counts = (np.arange(H * W).reshape(H, W) % 6).astype(np.uint8)  # 0 .. 5 at N = 4
    n = effective(counts, 4)
    assert set(n.ravel()) == {1, 2, 3, 4}
    got = fold_counts(samples, counts)
    for k in (1, 2, 3, 4):
        want = fold_mean(samples[:k])
        assert np.array_equal(_bits(got[n == k]), _bits(want[n == k])), k
    col, st = adaptive_ref(samples, counts)
    assert np.array_equal(_bits(col), _bits(got)) and st.shape == (H, W, 2)


# ------------------------------------------------------------ statistics ---
def _grey(*ls):
    """One-pixel samples whose luminances are the given values up to lum's own rounding."""
    return [np.array([[[l, l, l, 1.0]]], f32) for l in ls]


def test_stats_by_hand():
    # lum of a grey g: (0.2125 g + 0.7154 g) + 0.0721 g, evaluated in float32 as the definition orders it
    def L(g):
        g = f32(g)
        return f32(f32(f32(0.2125) * g) + f32(f32(0.7154) * g)) + f32(f32(0.0721) * g)

    assert lum(np.array([2.0, 2.0, 2.0], f32)) == L(2.0)
    one = stats_counts(_grey(2.0, 9.0, 9.0), np.array([[1]], np.uint8))[0, 0]
    assert one[0] == L(2.0) and one[1] == f32(-1.0)
    l0, l1, l2 = L(1.0), L(3.0), L(8.0)
    two = stats_counts(_grey(1.0, 3.0, 8.0), np.array([[2]], np.uint8))[0, 0]
    m = f32(f32(l0 + l1) / f32(2.0))
    d0, d1 = f32(l0 - m), f32(l1 - m)
    v = f32(f32(f32(d0 * d0) + f32(d1 * d1)) / f32(1.0))
    assert two[0] == m and two[1] == v
    assert abs(float(m) - 2.0) < 1e-6 and abs(float(v) - 2.0) < 1e-5  # mean 2, unbiased variance 2
    three = stats_counts(_grey(1.0, 3.0, 8.0), np.array([[255]], np.uint8))[0, 0]
    m = f32(f32(f32(l0 + l1) + l2) / f32(3.0))
    d = [f32(x - m) for x in (l0, l1, l2)]
    v = f32(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])) / f32(2.0))
    assert three[0] == m and three[1] == v
    assert abs(float(m) - 4.0) < 1e-5 and abs(float(v) - 13.0) < 1e-4


# ---------------------------------------------------------------- derive ---
def _planes(h=H, w=W, m=1.0, v=0.0):
    stats = np.empty((h, w, 2), f32)
    stats[..., 0], stats[..., 1] = m, v
    motion = np.zeros((h, w, 4), f32)
    nd = np.zeros((h, w, 4), f32)
    nd[..., 3] = 0.5
    return stats, motion, nd


def test_derive_background_and_zero_variance():
    stats, motion, nd = _planes()
    nd[1, 2, 3] = 1.0
    stats[1, 2] = (np.nan, -1.0)  # the background pixel itself is 1 whatever its statistics say
    got = derive_counts(stats, motion, nd, 1.0, 0.1, 8)
    assert got[1, 2] == 1
    want = np.full((H, W), 2)
    want[0:3, 1:4] = 8  # ... but its neighbours see a texel without an estimate
    want[1, 2] = 1
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bad", [(1.0, -1.0), (np.nan, 0.5), (1.0, np.nan), (1.0, np.inf)])
def test_derive_no_estimate_gives_n(bad):
    stats, motion, nd = _planes()
    stats[2, 3] = bad
    got = derive_counts(stats, motion, nd, 1.0, 0.1, 4)
    want = np.full((H, W), 2)
    want[1:4, 2:5] = 4
    assert np.array_equal(got, want)


def test_derive_bad_motion_and_off_frame():
    stats, motion, nd = _planes()
    motion[0, 0, 0] = np.nan
    motion[0, 1, 1] = np.inf
    motion[0, 2, 0] = -np.inf
    motion[2, 2, 0] = 1.0    # fx = 2.5 - 7 < 0
    motion[2, 3, 1] = -1.0   # fy = 2.5 + 5 >= H
    motion[4, 6, 0] = -1.0 / W  # fx = 6.5 + 1 = 7.5: one texel past the right edge
    motion[3, 0, 0] = 0.5 / W   # fx = 0: inside
    got = derive_counts(stats, motion, nd, 1.0, 0.1, 8)
    want = np.full((H, W), 2)
    for y, x in ((0, 0), (0, 1), (0, 2), (2, 2), (2, 3), (4, 6)):
        want[y, x] = 8
    assert np.array_equal(got, want)


def test_derive_noisy_texel_raises_its_neighbours_and_follows_motion():
    stats, motion, nd = _planes()
    # m = 1, tau = 0.5: d * d = 0.25, v = 1.2 -> need 4.8 -> 5
    stats[2, 3, 1] = 1.2
    got = derive_counts(stats, motion, nd, 1.0, 0.5, 8)
    want = np.full((H, W), 2)
    want[1:4, 2:5] = 5
    assert np.array_equal(got, want)
    # everything moved one texel right per frame, two frames ago: pixel x looks at x - 2
    motion[..., 0] = 1.0 / W
    got = derive_counts(stats, motion, nd, 2.0, 0.5, 8)
    want = np.full((H, W), 2)
    want[1:4, 4:7] = 5
    want[:, :2] = 8  # came from outside the frame
    assert np.array_equal(got, want)
    # half a texel: floor(x + 0.5 - 0.5) = x
    motion[..., 0] = 0.5 / W
    got = derive_counts(stats, motion, nd, 1.0, 0.5, 8)
    want = np.full((H, W), 2)
    want[1:4, 2:5] = 5
    assert np.array_equal(got, want)


def test_need_by_hand_and_monotone_in_tau():
    assert need(1.0, 0.0, 0.1, 8) == 2
    assert need(1.0, 0.03, 0.1, 8) == 3          # 0.03 / 0.01
    assert need(1.0, 0.079, 0.1, 8) == 8         # ceil(7.9) = 8: not < N
    assert need(1.0, 0.069, 0.1, 8) == 7
    assert need(0.0, 1e-9, 0.1, 8) == 8          # the floor on m: d = 1e-5, need 10
    assert need(0.0, 1e-10, 0.1, 8) == 2
    rng = np.random.default_rng(3)
    m = rng.random(4096, dtype=f32) * f32(2.0)
    v = rng.random(4096, dtype=f32) * f32(0.2)
    prev = None
    for tau in (0.05, 0.1, 0.2, 0.4, 0.8):
        r = need(m, v, tau, 8)
        assert r.min() >= 2 and r.max() <= 8
        if prev is not None:
            assert np.all(r <= prev)
        prev = r
    assert prev.min() == 2 and need(m, v, 0.05, 8).max() == 8


# ------------------------------------------------------------ C boundary ---
NEW = ("pt_pass_set_sample_counts", "pt_pass_set_sample_stats", "pt_sample_counts_derive")


def test_library_exports_and_header_declares_the_calls():
    from ptsvgf import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ptsvgf.h")).read()
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
    assert set(NEW) <= set(_lib.exported_symbols()[0])


def test_multi_rank_renderers_refuse_adaptive():
    from ptsvgf.dist import BandRenderer

    with pytest.raises(ValueError, match="adaptive"):
        BandRenderer(None, 16, 16, None, 0, 1, None, adaptive=0.5)

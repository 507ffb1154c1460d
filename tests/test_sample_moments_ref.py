"""The definition of "SVGF from sample moments" (tests/sample_moments_ref.cpp) on the CPU: tied to the
oracle where the two must agree, and checked for the statistical claim it exists for. No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_ref as O
import sample_moments_ref as SM
from adaptive_ref import effective, lum
from spp_ref import fold_mean

f32 = np.float32
W, H = 40, 24


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _eq(got, want, tag):
    idx = np.argwhere(np.any(_bits(got) != _bits(want), axis=-1))
    assert len(idx) == 0, (tag, len(idx), idx[:5].tolist())


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SM.load(tmp_path_factory.mktemp("sample_moments_ref"))


def random_frame(seed, w=W, h=H):
    """A G-buffer, a colour draw and a history with every case of the two passes in them: background holes, a history
    that moved (sub-texel and whole-texel motion, some of it out of the frame), depth and normal discontinuities that
    invalidate some taps and all taps, NaN colours, zero albedo, and history lengths on both sides of 4 (and of 32)."""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.random(s, dtype=f32)  # noqa: E731
    nrm = r(h, w, 3) - f32(0.5)
    nrm[:, : w // 2] = (0.1, 0.2, 0.97)  # a flat half, where the history validates
    nd = np.concatenate([nrm, np.full((h, w, 1), 0.4, f32)], axis=-1)
    nd[:, w // 2:, 3] = f32(0.2) + r(h, w - w // 2) * f32(0.5)
    prev_nd = nd.copy()
    prev_nd[h // 3: h // 2, : w // 3, 3] += f32(0.3)  # a depth step in the history
    prev_nd[:, w // 2:] += (r(h, w - w // 2, 4) - f32(0.5)) * f32(0.02)
    for a in (nd, prev_nd):  # background holes, not the same in the two frames
        y, x = rng.integers(0, h - 4), rng.integers(0, w - 6)
        a[y:y + 4, x:x + 6, 3] = 1.0
    nd[0, 0, 3] = nd[h - 1, w - 1, 3] = 1.0
    motion = np.zeros((h, w, 4), f32)
    motion[..., 0] = (r(h, w) - f32(0.5)) * f32(3.0 / w)
    motion[..., 1] = (r(h, w) - f32(0.5)) * f32(3.0 / h)
    motion[: h // 4, :, :2] = (f32(1.0) / f32(w), f32(-1.0) / f32(h))  # whole texels
    motion[h // 4: h // 4 + 2] = 0.0
    motion[h - 3:, : w // 4, 0] = 0.7  # out of the frame
    motion[..., 3] = r(h, w)  # (.z stays 0: no object motion, which the oracle does not model)
    fwidth = r(h, w, 4) * f32(0.05)
    albedo = r(h, w, 4)
    albedo[1, 1:4, :3] = 0.0
    emission = r(h, w, 4) * f32(0.1)
    color = r(h, w, 4) * f32(2.0)
    color[2, 5, 0] = np.nan
    color[3, 6, :3] = np.inf
    emission[3, 7, 1] = np.inf
    color[3, 7, 1] = np.inf  # inf - inf
    prev_illum = r(h, w, 4)
    prev_moments = r(h, w, 4)
    prev_moments[..., 1] = prev_moments[..., 0] ** 2 + r(h, w) * f32(0.1)
    prev_moments[..., 2] = np.floor(r(h, w) * f32(40.0))  # history lengths 0 .. 39
    prev_moments[:, : w // 2, 2] = rng.integers(0, 6, (h, w // 2)).astype(f32)
    return dict(motion=motion, color=color, albedo=albedo, emission=emission, prev_illum=prev_illum,
                prev_moments=prev_moments, nd=nd, prev_nd=prev_nd, fwidth=fwidth)


ORDER = ("motion", "color", "albedo", "emission", "prev_illum", "prev_moments", "nd", "prev_nd", "fwidth")


def _both(ref, fr, sm=None, w=W, h=H):
    args = [fr[k] for k in ORDER] + [f32(1.0) / f32(w), f32(1.0) / f32(h)]
    oi, om = ref.reproject(*args, sm=sm)
    return oi, om, ref.variance(oi, om, fr["nd"], fr["fwidth"], sm=sm)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plane_off_equals_the_oracle(ref, seed):
    fr = random_frame(seed)
    oi, om, v = _both(ref, fr)
    args = [fr[k] for k in ORDER] + [f32(1.0) / f32(W), f32(1.0) / f32(H)]
    wi, wm = O.reproject(*args)
    _eq(oi, wi, "reproject illum")
    _eq(om, wm, "reproject moments")
    _eq(v, O.variance(wi, wm, fr["nd"], fr["fwidth"]), "variance")
    surf = fr["nd"][..., 3] != 1.0
    hist = om[..., 2][surf]
    assert np.any(hist == 1.0) and np.any((hist > 1.0) & (hist < 4.0)) and np.any(hist >= 4.0)  # every branch ran
    assert np.any(~surf)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_one_sample_plane_equals_plane_off(ref, seed):
    """n = 1 everywhere, no accumulation: sm = (lum(illum), lum(illum)^2, 1, 1) and every output of both passes is the
    plane-off output bit for bit, so (with the test above) the oracle's."""
    fr = random_frame(seed)
    sm = ref.resolve_plane([fr["color"]], fr["emission"], fr["albedo"])
    assert np.all(sm[..., 2] == 1.0) and np.all(sm[..., 3] == 1.0)
    with np.errstate(all="ignore"):
        _eq(sm[..., 1:2], (sm[..., 0] * sm[..., 0]).astype(f32)[..., None], "nu = mu * mu")
    off = _both(ref, fr)
    on = _both(ref, fr, sm=sm)
    for name, a, b in zip(("illum", "moments", "variance"), on, off):
        _eq(a, b, name)
    # the same with a count plane of ones under N = 3
    sm3 = ref.resolve_plane([fr["color"]] * 3, fr["emission"], fr["albedo"], counts=np.ones((H, W), np.uint8))
    _eq(sm3, sm, "counts = 1")


def test_resolve_plane_follows_the_definition(ref):
    """The plane against a numpy restatement on finite inputs: counts 0 .. N and 255, with and without the
    accumulation weight."""
    rng = np.random.default_rng(7)
    N = 5
    samples = [rng.random((H, W, 4), dtype=f32) * f32(3.0) for _ in range(N)]
    e = rng.random((H, W, 4), dtype=f32) * f32(0.2)
    a = rng.random((H, W, 4), dtype=f32)
    a[0, :5, :3] = 0.0
    counts = rng.choice(np.array([0, 1, 2, 3, 4, 5, 255], np.uint8), (H, W))
    n = effective(counts, N)
    den = np.maximum(a[..., :3], f32(0.001))
    ls = [lum(((c[..., :3] - e[..., :3]).astype(f32) / den).astype(f32)) for c in samples]
    mu, nu = ls[0].copy(), (ls[0] * ls[0]).astype(f32)
    for s in range(1, N):
        mu = np.where(s < n, (mu + ls[s]).astype(f32), mu)
        nu = np.where(s < n, (nu + (ls[s] * ls[s]).astype(f32)).astype(f32), nu)
    nf = n.astype(f32)
    for acc, F in ((False, 0), (True, 0), (True, 6)):
        got = ref.resolve_plane(samples, e, a, counts, accumulate=acc, F=F)
        r = (f32(1.0) / nf).astype(f32)
        if acc:
            r = (r * (f32(1.0) / f32(F + 1))).astype(f32)
        want = np.stack([(mu / nf).astype(f32), (nu / nf).astype(f32), r, nf], axis=-1)
        _eq(got, want, ("plane", acc, F))
    full = ref.resolve_plane(samples, e, a)
    assert np.all(full[..., 3] == N)


def test_first_frame_variance_is_the_measured_one(ref):
    """The claim: with n h >= 4 on the first frame after a reset, the variance is (nu - mu^2) r, whose expectation for
    n iid samples of variance s2 is (n - 1) / n * s2 / n. The spatial guess of the plane-off passes on the same input
    is something else, and a luminance ramp goes into it as if it were noise.

    A flat surface (constant normal, depth, albedo; no emission), no history (zero planes: every tap fails the depth
    test, so hist = 1 and alpha = 1), n = 4, sample illumination l = ramp(x) + U(-0.5, 0.5): s2 = 1 / 12, central
    fourth moment mu4 = 1 / 80. Expected mean of the plane: 3/4 * (1/12) / 4 = 1 / 64 = 0.015625.
    Tolerance: 2 % of that, 3.125e-4. Standard error: the unbiased sample variance S2 of n iid values has
    Var(S2) = (mu4 - s2^2 (n - 3) / (n - 1)) / n = (0.0125 - 0.0069444 / 3) / 4 = 2.5463e-3; the biased one is
    3/4 S2 and the plane holds a quarter of it, so a pixel's standard deviation is (3/16) sqrt(2.5463e-3) = 9.4615e-3.
    Pixels are independent; 128 x 96 = 12288 of them give a standard error of 9.4615e-3 / sqrt(12288) = 8.535e-5, and
    three of those are 2.56e-4 < 3.125e-4. float32 rounding of nu - mu^2 (values near 1.2, differences near 0.06) is
    below 1e-6 of the result."""
    w, h, n = 128, 96, 4
    rng = np.random.default_rng(2026)
    ramp = (f32(1.0) + f32(0.4) * (np.arange(w, dtype=f32) / f32(w)))[None, :, None]
    albedo = np.zeros((h, w, 4), f32)
    albedo[..., :3] = 0.5  # (c / 0.5 is exact)
    albedo[..., 3] = 1.0
    emission = np.zeros((h, w, 4), f32)
    emission[..., 3] = 1.0
    samples = []
    for _ in range(n):
        x = (ramp + (rng.random((h, w, 1), dtype=f32) - f32(0.5))).astype(f32)
        c = np.ones((h, w, 4), f32)
        c[..., :3] = (x * f32(0.5)).astype(f32)
        samples.append(c)
    nd = np.zeros((h, w, 4), f32)
    nd[..., 2] = 1.0
    nd[..., 3] = 0.5
    zero = np.zeros((h, w, 4), f32)
    fr = dict(motion=zero, color=fold_mean(samples), albedo=albedo, emission=emission, prev_illum=zero,
              prev_moments=zero, nd=nd, prev_nd=zero, fwidth=zero)
    sm = ref.resolve_plane(samples, emission, albedo)
    oi, om, v_on = _both(ref, fr, sm=sm, w=w, h=h)
    assert np.all(om[..., 2] == 1.0)  # no history anywhere
    _eq(v_on, oi, "n h = 4: the variance pass copies")
    with np.errstate(all="ignore"):
        measured = np.maximum(f32(0.0), (sm[..., 1] - (sm[..., 0] * sm[..., 0]).astype(f32)).astype(f32))
        _eq(v_on[..., 3:], (measured * sm[..., 2]).astype(f32)[..., None], "(nu - mu^2) r")
    expected = (n - 1) / n * (1.0 / 12.0) / n
    tol = 0.02 * expected
    mean_on = float(np.mean(v_on[..., 3], dtype=np.float64))
    _, _, v_off = _both(ref, fr, w=w, h=h)
    mean_off = float(np.mean(v_off[..., 3], dtype=np.float64))
    print(f"first-frame variance: expected {expected:.6e}, plane on {mean_on:.6e}, plane off {mean_off:.6e}")
    assert abs(mean_on - expected) <= tol, (mean_on, expected)
    assert abs(mean_off - expected) > 10 * tol, (mean_off, expected)


def test_the_c_abi_declares_and_exports_the_setter():
    from ptsvgf import _lib

    txt = open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf.h")).read()
    assert "int pt_pass_set_sample_moments(uint32_t pass, void* device_f32x4);" in txt
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    assert hasattr(lib, "pt_pass_set_sample_moments")
    assert "pt_pass_set_sample_moments" in _lib.exported_symbols()[0]
    from ptsvgf.gl import RenderPass

    assert callable(RenderPass.set_sample_moments)

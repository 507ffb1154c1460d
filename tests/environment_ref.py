"""The environment's importance cache, restated in the order the device builds it (DESIGN.md "Environment edits",
csrc/kernels_environment.hip). The definition is pts_hdr_cache (csrc/scene_prep.cpp; ptsvgf.scene.hdr_cache); this is
the same arithmetic in numpy float32, one rounding per operation, arranged as the kernels are: luminance per texel, one
sequential total, pdf = lum / total, one chain per column for the marginal and for the conditional CDF, the marginal
CDF as a sequential prefix sum, and libstdc++'s lower_bound for both inversions. Any other order gives other bits.

Also the maps and the comparison the tests of pt_environment_update share."""
import numpy as np

SIZES = [(1, 1), (7, 5), (96, 40), (300, 130)]  # (W, H)
MAPS = ["random", "spike", "zero_columns", "negative_patch", "nan_texel", "all_zero"]


def lower_bound(a, v):
    """Per query q the index std::lower_bound(a[q], a[q] + n, v[q]) returns, by libstdc++'s own bisection: on plateaus,
    NaNs and rows that are not monotone no other search returns the same index. a: (m, n) or (n,); v: (m,)."""
    a = np.asarray(a, np.float32)
    v = np.asarray(v, np.float32)
    m = v.shape[0]
    n = a.shape[-1]
    rows = np.arange(m)
    first = np.zeros(m, np.int64)
    length = np.full(m, n, np.int64)
    with np.errstate(invalid="ignore"):
        while np.any(length > 0):
            act = length > 0
            half = length >> 1
            idx = np.minimum(first + half, n - 1)
            probe = a[idx] if a.ndim == 1 else a[rows, idx]
            less = act & (probe < v)
            first = np.where(less, first + half + 1, first)
            length = np.where(less, length - half - 1, np.where(act, half, length))
    return first


def environment_ref(hdr):
    """(h, w, 3) float32 map -> (h, w, 3) float32 cache texels (x, y, pdf)."""
    hdr = np.ascontiguousarray(hdr, np.float32)
    H, W, _ = hdr.shape
    f32 = np.float32
    with np.errstate(all="ignore"):
        d = hdr.astype(np.float64)
        lum = ((0.2 * d[..., 0] + 0.7 * d[..., 1]) + 0.1 * d[..., 2]).astype(f32)
        # ((0 + l0) + l1) + ...: ufunc accumulation is strictly sequential
        total = np.add.accumulate(np.concatenate([np.zeros(1, f32), lum.ravel()]), dtype=f32)[-1]
        pdf = lum / total
        margin = np.add.accumulate(np.vstack([np.zeros((1, W), f32), pdf]), axis=0, dtype=f32)[-1]
        cdfx = np.add.accumulate(margin, dtype=f32)
        cdfy = np.add.accumulate(pdf / margin[None, :], axis=0, dtype=f32)  # [i][j]: row i of column j's CDF
        xi_1 = np.arange(H, dtype=f32) / f32(H)
        xi_2 = np.arange(W, dtype=f32) / f32(W)
        x = np.minimum(lower_bound(cdfx, xi_1), W - 1)  # per row
        out = np.empty((H, W, 3), f32)
        for i in range(H):
            col = np.ascontiguousarray(cdfy[:, x[i]])
            y = np.minimum(lower_bound(col, xi_2), H - 1)
            out[i, :, 0] = f32(x[i]) / f32(W)
            out[i, :, 1] = y.astype(f32) / f32(H)
        out[..., 2] = pdf
    return out


def make_map(kind, w, h, seed=0):
    """The maps the issue names, (h, w, 3) float32; seeded."""
    rng = np.random.default_rng(1000 * seed + 31 * w + h)
    a = rng.uniform(0.05, 4.0, (h, w, 3)).astype(np.float32)
    if kind == "random":
        pass
    elif kind == "spike":  # one texel far above the rest: the CDFs plateau in float32
        a[h // 3, (2 * w) // 3] = 3e5
    elif kind == "zero_columns":  # their conditional CDFs are NaN
        cols = [c for c in range(20, 30) if c < w] or [w // 2]
        a[:, cols] = 0.0
    elif kind == "negative_patch":  # CDFs that are not monotone
        a[h // 4:h // 4 + max(1, h // 5), w // 4:w // 4 + max(1, w // 5)] *= -1.5
    elif kind == "nan_texel":
        a[h // 2, w // 2, 1] = np.nan
    elif kind == "all_zero":
        a[:] = 0.0
    else:
        raise ValueError(kind)
    return a


def texels_equal(got, want):
    """Bit for bit, except that in `want`'s NaN texels of channel 2 (the pdf) any NaN matches. got, want: (h, w, >= 3)
    float32 of one shape. Returns the number of texel channels that differ."""
    g = np.ascontiguousarray(got, np.float32)
    w = np.ascontiguousarray(want, np.float32)
    assert g.shape == w.shape, (g.shape, w.shape)
    diff = g.view(np.uint32) != w.view(np.uint32)
    both_nan = np.isnan(g[..., 2]) & np.isnan(w[..., 2])
    diff[..., 2] &= ~both_nan
    return int(diff.sum())


def upload_route(hdr):
    """What pt_texture2d_upload(hdr_tex, rgb) and pt_texture2d_upload(cache_tex, hdr_cache(rgb)) leave: two (h, w, 4)
    planes with 1 in the fourth channel."""
    from ptsvgf.scene import hdr_cache

    hdr = np.ascontiguousarray(hdr, np.float32)
    one = np.ones(hdr.shape[:2] + (1,), np.float32)
    return np.concatenate([hdr, one], axis=2), np.concatenate([hdr_cache(hdr), one], axis=2)

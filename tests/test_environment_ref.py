"""tests/environment_ref.py, the importance cache in the order the device builds it, against its definition
pts_hdr_cache (ptsvgf.scene.hdr_cache): bit for bit, a NaN pdf matching a NaN, on the sizes and maps the GPU tests of
pt_environment_update use. No device."""
import numpy as np
import pytest

import environment_ref as E
from ptsvgf.scene import hdr_cache


@pytest.mark.parametrize("size", E.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", E.MAPS)
def test_ref_equals_host_cache(kind, size):
    w, h = size
    m = E.make_map(kind, w, h)
    want = hdr_cache(m)
    got = E.environment_ref(m)
    assert np.all(np.isfinite(want[..., :2]))  # x and y are indices over the size, whatever the CDFs hold
    assert E.texels_equal(got, want) == 0


def test_spike_plateaus_and_nan_columns_are_exercised():
    # the maps do what they are for: a spike leaves few distinct (x, y), zero columns and a NaN texel give NaN pdfs or
    # CDFs, a negative patch a CDF that is not monotone
    w, h = 96, 40
    c = hdr_cache(E.make_map("spike", w, h))
    assert len({(a, b) for a, b in c[..., :2].reshape(-1, 2).tolist()}) < w * h // 20
    assert np.all(np.isnan(hdr_cache(E.make_map("nan_texel", w, h))[..., 2]))
    assert np.all(np.isnan(hdr_cache(E.make_map("all_zero", w, h))[..., 2]))
    z = E.make_map("zero_columns", w, h)
    assert np.all(hdr_cache(z)[:, 20:30, 2] == 0.0)
    n = hdr_cache(E.make_map("negative_patch", w, h))
    assert (n[..., 2] < 0).any()


def test_lower_bound_is_libstdcxx_bisection():
    # on a row that is not monotone the bisection's own probes decide
    a = np.array([0.1, 0.9, 0.2, np.nan, 0.3, 0.8, 0.4], np.float32)
    for v in (0.0, 0.15, 0.25, 0.5, 0.85, 1.0):
        first, n = 0, len(a)
        while n > 0:
            half = n >> 1
            if a[first + half] < np.float32(v):
                first += half + 1
                n -= half + 1
            else:
                n = half
        assert E.lower_bound(a, np.array([v], np.float32))[0] == first

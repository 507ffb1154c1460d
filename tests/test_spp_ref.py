"""The definition of an spp draw (tests/spp_ref.py) against the CPU oracle it is built on: no GPU."""
import numpy as np
import pytest

import oracle_ref as O
from spp_ref import fold_mean, mix_last, sample_counter, spp_ref

W, H = 160, 96
F = 5
f32 = np.float32


def _cam():
    from ptsvgf.camera import Camera, rigid_inverse

    cam = Camera(W, H)
    cam.update()
    return cam.cam_position, rigid_inverse(cam.cam_view_mat)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(a, b, tag):
    bad = np.argwhere(np.any(_bits(a) != _bits(b), axis=-1))
    assert len(bad) == 0, (tag, len(bad), bad[:5].tolist())


@pytest.fixture(scope="module")
def small(scene_small):
    """The oracle scene, the camera and the four sample draws of frame F at N = 4, computed once."""
    os_ = O.OracleScene(scene_small)
    eye, rot = _cam()
    kw = dict(aspect_corrected=True)
    four = [os_.path_trace(W, H, 4 * F + s, eye, rot, **kw) for s in range(4)]
    return os_, eye, rot, kw, four


def test_one_sample_is_the_oracle_draw(small):
    os_, eye, rot, kw, _ = small
    want = os_.path_trace(W, H, F, eye, rot, **kw)
    got = spp_ref(os_, W, H, F, 1, eye, rot, **kw)
    for g, w, k in zip(got, want, ("color", "emission", "albedo")):
        _same(g, w, k)
    last = np.random.default_rng(1).random((H, W, 4), dtype=f32)
    want = os_.path_trace(W, H, F, eye, rot, accumulate=True, last_frame=last, **kw)
    got = spp_ref(os_, W, H, F, 1, eye, rot, accumulate=True, last_frame=last, **kw)
    _same(got[0], want[0], "accumulate")


def test_four_samples(small):
    os_, eye, rot, kw, four = small
    one = spp_ref(os_, W, H, F, 1, eye, rot, **kw)
    got = spp_ref(os_, W, H, F, 4, eye, rot, **kw)
    assert not np.array_equal(_bits(got[0]), _bits(one[0]))
    _same(got[1], one[1], "emission")
    _same(got[2], one[2], "albedo")
    # the fold written out: counters 4F .. 4F + 3, float32, in order, one division
    c = [x[0][..., :3] for x in four]
    rgb = (((c[0] + c[1]).astype(f32) + c[2]).astype(f32) + c[3]).astype(f32) / f32(4.0)
    assert rgb.dtype == f32
    _same(got[0][..., :3], rgb, "fold")
    assert np.all(got[0][..., 3] == f32(1.0))
    for s in range(4):  # every sample's first-hit planes are one set of bits
        _same(four[s][1], four[0][1], ("emission", s))
        _same(four[s][2], four[0][2], ("albedo", s))
    # less noise, not another image: the mean of 4 lies nearer to the mean of 8 other samples than one sample does
    ref8 = spp_ref(os_, W, H, F + 100, 8, eye, rot, **kw)[0][..., :3]
    assert np.mean(np.abs(got[0][..., :3] - ref8)) < np.mean(np.abs(one[0][..., :3] - ref8))


def test_nan_rule_is_per_sample(scene_nan):
    """The oracle applies :1110-1113 to every sample, so a sample whose radiance was NaN arrives as 0 and the pixel
    is the mean of the others and 0: no NaN reaches the sum."""
    os_ = O.OracleScene(scene_nan)
    eye, rot = _cam()
    samples = []
    col = spp_ref(os_, W, H, F, 4, eye, rot, aspect_corrected=True, samples=samples)[0]
    assert len(samples) == 4 and not any(np.isnan(s).any() for s in samples)
    assert not np.isnan(col).any()
    zero = [~s[..., :3].any(axis=-1) for s in samples]
    some = np.any(zero, axis=0) & ~np.all(zero, axis=0)  # a black sample beside lit ones
    assert some.any()
    _same(col, fold_mean(samples), "fold")
    y, x = np.argwhere(some)[0]
    lit = [s[y, x, :3] for s in samples]
    want = (((lit[0] + lit[1]).astype(f32) + lit[2]).astype(f32) + lit[3]).astype(f32) / f32(4.0)
    assert np.array_equal(_bits(col[y, x, :3]), _bits(want))


def test_accumulate_uses_the_frame_counter(small):
    os_, eye, rot, kw, _ = small
    last = np.random.default_rng(2).random((H, W, 4), dtype=f32)
    plain = spp_ref(os_, W, H, F, 4, eye, rot, **kw)[0]
    got = spp_ref(os_, W, H, F, 4, eye, rot, accumulate=True, last_frame=last, **kw)[0]
    a = f32(1.0) / f32(F + 1)  # F, not 4F + s
    want = (last[..., :3] * (f32(1.0) - a)).astype(f32) + (plain[..., :3] * a).astype(f32)
    _same(got[..., :3], want.astype(f32), "mix at F")
    _same(got, mix_last(last, plain, F), "mix_last")
    wrong = mix_last(last, plain, 4 * F)
    assert not np.array_equal(_bits(got), _bits(wrong))


def test_counter_wraps(small):
    os_, eye, rot, kw, _ = small
    Fmax = 2 ** 32 - 1
    assert [sample_counter(Fmax, 2, s) for s in range(2)] == [2 ** 32 - 2, 2 ** 32 - 1]
    assert sample_counter(2 ** 31, 2, 1) == 1
    c0 = os_.path_trace(W, H, 2 ** 32 - 2, eye, rot, **kw)[0]
    c1 = os_.path_trace(W, H, 2 ** 32 - 1, eye, rot, **kw)[0]
    got = spp_ref(os_, W, H, Fmax, 2, eye, rot, **kw)[0]
    _same(got, fold_mean([c0, c1]), "wrap")
    # accumulation at F = 2^32 - 1: float(F + 1u) = 0, as the reference's uint arithmetic gives
    with np.errstate(all="ignore"):
        acc = spp_ref(os_, W, H, Fmax, 2, eye, rot, accumulate=True, last_frame=np.zeros((H, W, 4), f32), **kw)[0]
    assert acc.shape == (H, W, 4)


def test_range():
    for n in (0, -1, 9, 1.5):
        with pytest.raises(ValueError):
            spp_ref(None, W, H, F, n, None, None)

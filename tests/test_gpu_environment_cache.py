"""pt_environment_update's texels (DESIGN.md "Environment edits"): after one update the readbacks of the hdrMap and
hdrCache textures equal, bit for bit (a NaN pdf matching a NaN), what pt_texture2d_upload of the map and of
pts_hdr_cache's cache leave; from a host array and from device memory, which is consumed in stream order."""
import ctypes as C

import numpy as np
import pytest

import environment_ref as E

pytestmark = pytest.mark.gpu


def _device(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.fixture(scope="module")
def pairs(gpu):
    """Per size one (hdrMap, hdrCache) pair, created as a renderer creates them."""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            m0 = E.make_map("random", w, h, seed=7)
            hdr, cache = gpu.getTextureRGB32F(w, h), gpu.getTextureRGB32F(w, h)
            a, b = E.upload_route(m0)
            gpu.upload_rgb32f(hdr, a[..., :3])
            gpu.upload_rgb32f(cache, b[..., :3])
            made[w, h] = (hdr, cache)
        return made[w, h]

    yield get
    for hdr, cache in made.values():
        gpu.destroy_texture(hdr)
        gpu.destroy_texture(cache)


def _check(gpu, pair, m, tag):
    want_hdr, want_cache = E.upload_route(m)
    got_hdr, got_cache = gpu.readback(pair[0]), gpu.readback(pair[1])
    bad = np.argwhere(got_hdr.view(np.uint32) != want_hdr.view(np.uint32))
    assert len(bad) == 0, (tag, "hdr", len(bad), bad[:5].tolist())
    n = E.texels_equal(got_cache, want_cache)
    if n:
        d = got_cache.view(np.uint32) != want_cache.view(np.uint32)
        d[..., 2] &= ~(np.isnan(got_cache[..., 2]) & np.isnan(want_cache[..., 2]))
        at = np.argwhere(d)[:5]
        print(tag, n, [(tuple(i), got_cache[tuple(i)], want_cache[tuple(i)]) for i in at.tolist()])
    assert n == 0, (tag, "cache", n)


@pytest.mark.parametrize("source", ["host", "device"])
@pytest.mark.parametrize("size", E.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", E.MAPS)
def test_texels_equal_the_upload_route(gpu, pairs, kind, size, source):
    w, h = size
    pair = pairs(w, h)
    m = E.make_map(kind, w, h)
    v0 = gpu.environment_state(pair[0])["version"]
    gpu.environment_update(pair[0], pair[1], m if source == "host" else _device(m))
    assert gpu.environment_state(pair[0])["version"] == v0 + 1
    _check(gpu, pair, m, f"{kind}/{w}x{h}/{source}")


@pytest.mark.parametrize("source", ["host", "device"])
def test_bench_size(gpu, source):
    from ptsvgf.scene import env_map

    w, h = 2048, 1024
    m = env_map(w, h)
    hdr, cache = gpu.getTextureRGB32F(w, h), gpu.getTextureRGB32F(w, h)
    try:
        gpu.environment_update(hdr, cache, m if source == "host" else _device(m))
        _check(gpu, (hdr, cache), m, f"env_map/{source}")
    finally:
        gpu.destroy_texture(hdr)
        gpu.destroy_texture(cache)


def test_device_source_is_consumed_in_stream_order(gpu, pairs):
    """A torch op on the library's current stream writes the map just before the call and overwrites it just after:
    the textures hold the map as it was at the call."""
    import torch

    from ptsvgf._lib import check, pt

    w, h = 300, 130
    pair = pairs(w, h)
    a, b = _device(E.make_map("random", w, h, seed=3)), _device(E.make_map("spike", w, h, seed=4))
    big = torch.zeros(1 << 24, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    check(pt().pt_set_stream(C.c_void_p(s.cuda_stream)))
    try:
        with torch.cuda.stream(s):
            src = torch.empty_like(a)
            big.add_(1.0)  # (the stream is busy when the copy below is queued)
            src.copy_(a)
            gpu.environment_update(pair[0], pair[1], src)
            src.copy_(b)
    finally:
        check(pt().pt_use_own_stream())
    _check(gpu, pair, a.cpu().numpy(), "stream order")
    torch.cuda.synchronize()
    assert torch.equal(src, b)


def test_sequence_with_the_upload_route(gpu):
    """An update before any draw; an old-route upload after an update; an update after that. The device pointer is
    the current version's, another after every update."""
    w, h = 96, 40
    maps = [E.make_map(k, w, h, seed=s) for s, k in enumerate(("random", "spike", "negative_patch"))]
    hdr, cache = gpu.getTextureRGB32F(w, h), gpu.getTextureRGB32F(w, h)
    try:
        assert gpu.environment_state(hdr) == {"version": 1, "device_versions": 1, "staging_slots": 0}
        p0 = gpu.device_ptr(hdr)
        gpu.environment_update(hdr, cache, maps[0])
        _check(gpu, (hdr, cache), maps[0], "first")
        p1 = gpu.device_ptr(hdr)
        assert p1 != p0
        a, b = E.upload_route(maps[1])
        gpu.upload_rgb32f(hdr, a[..., :3])
        gpu.upload_rgb32f(cache, b[..., :3])
        _check(gpu, (hdr, cache), maps[1], "upload after update")
        assert gpu.device_ptr(hdr) == p1
        gpu.environment_update(hdr, cache, _device(maps[2]))
        _check(gpu, (hdr, cache), maps[2], "update after upload")
        st = gpu.environment_state(hdr)
        assert st["version"] == 4 and st["device_versions"] <= 3 and st["staging_slots"] == 1, st
        assert gpu.environment_state(cache)["device_versions"] == st["device_versions"]
        # a new size goes the old route, and ends the versions
        small = E.make_map("random", 7, 5)
        a, b = E.upload_route(small)
        gpu.upload_rgb32f(hdr, a[..., :3])
        assert gpu.environment_state(hdr)["device_versions"] == 1
        want_cache = E.upload_route(maps[2])[1]
        assert E.texels_equal(gpu.readback(cache), want_cache) == 0  # the partner keeps its texels
        gpu.upload_rgb32f(cache, b[..., :3])
        gpu.environment_update(hdr, cache, small)
        _check(gpu, (hdr, cache), small, "after a new size")
    finally:
        gpu.destroy_texture(hdr)
        gpu.destroy_texture(cache)


def test_error_returns_leave_everything_untouched(gpu, pairs, scene_small):
    import torch

    from ptsvgf._lib import PtError

    w, h = 96, 40
    pair = pairs(w, h)
    m = E.make_map("random", w, h, seed=11)
    gpu.environment_update(pair[0], pair[1], m)
    before = (gpu.environment_state(pair[0]), gpu.environment_state(pair[1]), gpu.device_ptr(pair[0]),
              gpu.device_ptr(pair[1]))
    other = gpu.getTextureRGB32F(7, 5)
    buf = gpu.texture_buffer(scene_small.lights)
    mem = torch.zeros(h, w, 4, device="cuda")
    wrapped = gpu.wrap_device_texture(mem.data_ptr(), w, h)
    gpu.set_band(w, h, 0, h // 2, 0, h // 2)
    try:
        banded = gpu.getTextureRGB32F(w, h)
    finally:
        gpu.set_band(w, h, 0, h, 0, h)
    bad = E.make_map("spike", w, h)
    try:
        for hdr, cache, data, code in ((pair[0], pair[0], bad, -6), (pair[0], pair[1], bad[:, :7], -6),
                                       (pair[0], other, bad, -6), (other, pair[1], bad, -6),
                                       (pair[0], buf, bad, -1), (987654, pair[1], bad, -1),
                                       (pair[0], wrapped, bad, -9), (wrapped, pair[1], bad, -9),
                                       (pair[0], banded, bad, -9)):
            with pytest.raises(PtError) as e:
                gpu.environment_update(hdr, cache, data)
            assert e.value.code == code, (hdr, cache, code, str(e.value))
        after = (gpu.environment_state(pair[0]), gpu.environment_state(pair[1]), gpu.device_ptr(pair[0]),
                 gpu.device_ptr(pair[1]))
        assert after == before
        _check(gpu, pair, m, "after the errors")
    finally:
        for t in (other, buf, wrapped, banded):
            gpu.destroy_texture(t)

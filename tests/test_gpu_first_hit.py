"""The bounce-0 shade's keep mode on the device (DESIGN.md "Static view, part 4"; int uniform reuse_static on the
path-tracing passes): on a standing view a draw leaves the miss pixels alone, stores no emission or albedo texel and
does not visit all-miss tiles, and `color`, `emission`, `albedo` and the modulated frame of every frame equal, bit for
bit, those of a renderer whose path-tracing passes have the uniform 0.

The shapes are tests/test_gpu_static_background.py's: one quad in a corner of the frame over the environment, at
256 x 256 and at 200 x 136 (partial tiles at the right and bottom edges); the quad's edge gives tiles that mix hit and
miss pixels. One and four frames in flight."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFF, FULL, KEEP = 0, 1, 2
(R_NONE, R_UNIFORM, R_ENV, R_STATS, R_SPP, R_BATCH, R_MEGAKERNEL, R_TILES, R_ROWS, R_DEEP, R_UNFOLDED, R_DEPTH0,
 R_ACCUMULATE, R_STAGE, R_COLOUR, R_EMISSION, R_ALBEDO) = range(17)
SIZES = [(256, 256), (200, 136)]


def _quad_scene(x0, y0, x1, y1, colour=(0.7, 0.5, 0.3)):
    from ptsvgf.scene import POINT_LIGHTS, Scene, SceneBuilder, env_map, hdr_cache, material, transform

    b = SceneBuilder()
    pos = np.array([[x0, y0, 0.0], [x1, y0, 0.0], [x1, y1, 0.0], [x0, y1, 0.0]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    b.add_mesh(pos, idx, material(baseColor=colour), transform(), True, 0)
    b.build(8)
    tri, node, raster = b.encode()
    hdr = env_map(128, 64)
    return Scene("quad", tri, node, raster, POINT_LIGHTS.copy(), hdr, hdr_cache(hdr), b.counts())


@pytest.fixture(scope="module")
def corner():
    return _quad_scene(-1.7, 1.0, -1.1, 1.6)   # top-left of the default view


@pytest.fixture(scope="module")
def other_corner():
    return _quad_scene(1.1, -1.4, 1.7, -0.8)   # the same two triangles, bottom-right


@pytest.fixture(scope="module")
def recoloured():
    return _quad_scene(-1.7, 1.0, -1.1, 1.6, colour=(0.2, 0.6, 0.9))


def _make(scene, w, h, on, k=1, **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, w, h, mode="fast", aspect_corrected=True, run_taa=False, run_output=False, frames_in_flight=k,
                 **kw)
    if not on:
        for p, _ in r.pt_slots:
            p.set_uniform_int("reuse_static", 0)
    return r


def _textures(r):
    t = dict(modulate=r.modulate_color)
    for s, (_, (c, e, a)) in enumerate(r.pt_slots):
        t[f"color{s}"], t[f"emission{s}"], t[f"albedo{s}"] = c, e, a
    return t


def _sync(r):
    import torch

    r.flush()
    torch.cuda.synchronize()


def _run(gl, scene, w, h, on, steps, k=1, **kw):
    """steps: per frame None or a callable(renderer, gl) applied before the frame. Returns per frame the planes and, of
    the slot that drew it, (mode, reason, kept, busy, tiles)."""
    r = _make(scene, w, h, on, k, **kw)
    frames, info = [], []
    try:
        for f, st in enumerate(steps):
            if st is not None:
                _sync(r)
                st(r, gl)
            r.frame()
            _sync(r)
            frames.append({key: gl.readback(t).view(np.uint32).copy() for key, t in _textures(r).items()})
            p = r.pt_slots[f % len(r.pt_slots)][0]
            info.append(p.first_hit_last() + p.first_hit_busy())
    finally:
        r.close()
    return frames, info


def _assert_equal(on, off):
    assert len(on) == len(off)
    for f, (a, b) in enumerate(zip(on, off)):
        for key in a:
            bad = np.argwhere(np.any(a[key] != b[key], axis=-1))
            assert len(bad) == 0, (f, key, len(bad), bad[:5].tolist())


def _assert_keeps(i):
    mode, reason, kept, busy, tiles = i
    assert (mode, reason) == (KEEP, R_NONE) and kept > 0 and 0 < busy < tiles, i


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("k", [1, 4])
def test_ten_standing_frames(gpu, corner, w, h, k):
    on, i_on = _run(gpu, corner, w, h, True, [None] * 10, k)
    off, i_off = _run(gpu, corner, w, h, False, [None] * 10, k)
    for f, i in enumerate(i_on):
        print(f, i)
    _assert_equal(on, off)
    for f in range(10):
        assert i_off[f][:3] == (OFF, R_UNIFORM, 0), (f, i_off[f])
        if f < k:  # the slot's first draw runs the primary stage
            assert i_on[f][:3] == (FULL, R_STAGE, 0), (f, i_on[f])
        else:
            _assert_keeps(i_on[f])
            assert i_on[f][2] == f // k
    # the frames are not copies of each other: the hit pixels' colour follows the frame counter
    assert not np.array_equal(on[9][f"color{9 % k}"], on[9 - k][f"color{9 % k}"])
    hit = np.any(off[9]["albedo0"][..., :3] != 0, axis=-1)
    assert hit.any() and not hit.all()
    # the quad covers few tiles: the list is short, and holds at least the tiles the quad's pixels lie in
    tiles_hit = len({(y // 16, x // 16) for y, x in np.argwhere(hit)})
    assert i_on[9][3] == tiles_hit


@pytest.mark.parametrize("name,reason", [("color0", R_COLOUR), ("emission0", R_EMISSION), ("albedo0", R_ALBEDO)])
def test_poison_through_the_library_costs_one_full_draw(gpu, corner, name, reason):
    w, h = 200, 136
    junk = np.full((h, w, 4), np.nan, np.float32)

    def spoil(r, gl):
        gl.upload_rgba(_textures(r)[name], junk)

    steps = [None] * 3 + [spoil] + [None] * 2
    on, i_on = _run(gpu, corner, w, h, True, steps)
    off, _ = _run(gpu, corner, w, h, False, steps)
    _assert_equal(on, off)
    _assert_keeps(i_on[2])
    assert i_on[3][:2] == (FULL, reason), i_on[3]
    _assert_keeps(i_on[4])
    assert not np.isnan(on[3][name].view(np.float32)).any()


def test_poison_the_library_cannot_see_shows_what_a_kept_draw_writes(gpu, corner):
    """The attachments are torch tensors wrapped as textures, so a fill from torch is a write the library cannot see
    (the caller's statement reuse_static = 1 is then false, on purpose). After it a kept draw restores exactly the
    pixels it must write: the colour of the hit pixels. Every other texel keeps the poison, which a full draw would
    have overwritten: the skip is real."""
    import torch

    from ptsvgf import gl

    w, h = 200, 136
    held = {}

    def factory(tw, th):
        t = torch.zeros((th, tw, 4), dtype=torch.float32, device="cuda")
        handle = gl.wrap_device_texture(t.data_ptr(), tw, th)
        held[handle] = t
        return handle

    want, _ = _run(gpu, corner, w, h, False, [None] * 4)
    r = _make(corner, w, h, True, tex_factory=factory)
    try:
        p, (c, e, a) = r.pt_slots[0]
        assert p.first_hit_last()[0] == OFF
        p.set_uniform_int("reuse_static", 1)  # (a renderer that does not own its planes leaves it 0)
        for _ in range(3):
            r.frame()
        _sync(r)
        _assert_keeps(p.first_hit_last() + p.first_hit_busy())
        for t in (c, e, a):
            held[t].fill_(float("nan"))
        torch.cuda.synchronize()
        r.frame()
        _sync(r)
        _assert_keeps(p.first_hit_last() + p.first_hit_busy())
        got = {k: held[t].cpu().numpy() for k, t in (("color", c), ("emission", e), ("albedo", a))}
    finally:
        r.close()
    hit = np.any(want[3]["albedo0"][..., :3] != 0, axis=-1)
    assert hit.any() and not hit.all()
    assert np.array_equal(got["color"].view(np.uint32)[hit], want[3]["color0"][hit])
    assert np.isnan(got["color"][~hit]).all()
    assert np.isnan(got["emission"]).all() and np.isnan(got["albedo"]).all()


def _orbit(r, gl):
    r.camera.orbit(3.0, 1.0)


def _new_environment(r, gl):
    from ptsvgf.scene import env_map

    gl.upload_rgb32f(r.hdrMap, np.ascontiguousarray(env_map(128, 64)[::-1] * np.float32(0.5)))


def _clamp(r, gl):
    r.cfg.clamp_threshold = 0.25  # a uniform on the miss path: the environment is brighter than this


def _to(scene):
    return lambda r, gl: r.rebuild_bvh(tri_enc=scene.tri_enc, raster=scene.raster, leaf_n=8, ploc_radius=16)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("change,reason", [(_orbit, R_STAGE), (_new_environment, R_COLOUR), (_clamp, R_COLOUR),
                                           ("material", R_STAGE)],
                         ids=["camera", "environment", "uniform", "material"])
def test_static_change_static(gpu, corner, recoloured, w, h, change, reason):
    first = None
    if change == "material":  # both scenes as device builds, so that the edit changes the materials alone
        first, change = _to(corner), _to(recoloured)
    steps = [first] + [None] * 3 + [change] + [None] * 3
    on, i_on = _run(gpu, corner, w, h, True, steps)
    off, _ = _run(gpu, corner, w, h, False, steps)
    _assert_equal(on, off)
    assert i_on[0][0] == FULL
    for f in (1, 2, 3, 5, 6, 7):
        _assert_keeps(i_on[f])
    assert i_on[4][:2] == (FULL, reason), i_on[4]
    assert any(not np.array_equal(on[3][k], on[4][k]) for k in ("color0", "albedo0"))


@pytest.mark.parametrize("w,h", SIZES)
def test_geometry_moves_into_an_all_miss_tile_and_back(gpu, corner, other_corner, w, h):
    steps = [_to(corner)] + [None] * 3 + [_to(other_corner)] + [None] * 3 + [_to(corner)] + [None] * 3
    on, i_on = _run(gpu, corner, w, h, True, steps)
    off, _ = _run(gpu, corner, w, h, False, steps)
    _assert_equal(on, off)
    for f in (0, 4, 8):
        assert i_on[f][:2] == (FULL, R_STAGE), (f, i_on[f])
        assert i_on[f][3] == -1  # the list of the stage before is gone
    for f in (1, 2, 3, 5, 6, 7, 9, 10, 11):
        _assert_keeps(i_on[f])
    surf = [np.any(on[f]["albedo0"][..., :3] != 0, axis=-1) for f in (3, 7, 11)]
    assert surf[0].any() and surf[1].any() and not (surf[0] & surf[1]).any() and np.array_equal(surf[0], surf[2])
    for f, s in zip((3, 7, 11), surf):  # the list follows the geometry
        assert i_on[f][3] == len({(y // 16, x // 16) for y, x in np.argwhere(s)}), f


def test_bypasses_draw_in_mode_off(gpu, corner, scene_cornell):
    import torch

    from ptsvgf.renderer import parameter_config
    from test_gpu_deep import chain_bvh

    w, h = 256, 256

    def last(r, frames=4):
        for _ in range(frames):
            r.frame()
        _sync(r)
        return [p.first_hit_last()[:2] for p, _ in r.pt_slots]

    def uniform(name, v):
        def prepare(r):
            for p, _ in r.pt_slots:
                p.set_uniform_int(name, v)
        return prepare

    def rows(r):
        for p, _ in r.pt_slots:
            p.set_rows(0, h - 16)

    cost = torch.zeros(h, dtype=torch.int32, device="cuda")

    def row_cost(r):
        for p, _ in r.pt_slots:
            p.set_row_cost(cost.data_ptr())

    def depth0(r):
        r.cfg.max_tracing_depth = 0

    acc = parameter_config()
    acc.accumulate_color = True
    cases = [(dict(spp=2), 1, None, R_SPP), (dict(trace_batch=2), 4, None, R_BATCH),
             ({}, 1, uniform("pt_kernel", 1), R_MEGAKERNEL), ({}, 1, uniform("tile_stride", 2), R_TILES),
             ({}, 1, rows, R_ROWS), ({}, 1, uniform("shade_fold", 0), R_UNFOLDED), ({}, 1, depth0, R_DEPTH0),
             ({}, 1, row_cost, R_STATS), (dict(config=acc), 1, None, R_ACCUMULATE),
             ({}, 1, uniform("reuse_static", 0), R_UNIFORM)]
    for kw, k, prepare, reason in cases:
        r = _make(corner, w, h, True, k, **kw)
        try:
            if prepare:
                prepare(r)
            got = last(r, 6)
            # (an accumulating renderer keeps a second slot for lastFrame: a pass that has not drawn reports (0, 0))
            assert got[0] == (OFF, reason) and all(g in ((OFF, reason), (0, 0)) for g in got), (reason, got)
            assert all(p.first_hit_last()[2] == 0 for p, _ in r.pt_slots), reason
        finally:
            r.close()
    # trace statistics: bound for one frame of a standing view that keeps before and after
    r = _make(corner, w, h, True)
    try:
        assert last(r) == [(KEEP, R_NONE)]
        r.trace_stats()
        assert r.pt_slots[0][0].first_hit_last()[:2] == (OFF, R_STATS)
        # the counted draw ran the stage and stamped the colour, and left no first-hit record
        assert last(r, 1) == [(FULL, R_EMISSION)]
        assert last(r, 1) == [(KEEP, R_NONE)]
    finally:
        r.close()
    # a band (pt_set_band): the standing pass drawn once more with a band of the frame's rows set
    r = _make(corner, w, h, True)
    try:
        assert last(r) == [(KEEP, R_NONE)]
        p = r.pt_slots[0][0]
        gpu.set_band(w, h, 16, 64, 0, h)
        try:
            p.draw()
            _sync(r)
            assert p.first_hit_last()[:2] == (OFF, R_ROWS)
        finally:
            gpu.set_band(w, h, 0, h, 0, h)
    finally:
        r.close()
    # a reference tree deeper than the LDS stack
    tri = scene_cornell.tri_enc[np.random.default_rng(7).permutation(scene_cornell.ntris)]
    deep = dataclasses.replace(scene_cornell, name="cornell_chain", tri_enc=tri, node_enc=chain_bvh(tri))
    r = _make(deep, 64, 48, True)
    try:
        assert last(r, 3) == [(OFF, R_DEEP)]
    finally:
        r.close()

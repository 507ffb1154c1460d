"""The bounce-0 point-light verdict cache (pass uniform point_cache, DESIGN.md "Static view, part 2"): from a standing
view, whether light i is occluded from a pixel's first hit does not change, so once a shadow ray has brought the verdict
back, later frames store it instead of queueing the ray. Every sequence is drawn twice, with point_cache 1 and 0 (the
primary-hit cache on in both), and the path tracer's planes must agree bit for bit frame by frame. The counters of
pt_debug_point_cache_counts and the plane itself (pt_debug_point_cache_read) must show the cache serving verdicts
where the sequence says and nowhere else, and a plane with its verdicts flipped must change the picture: so neither a
cache that never engages, nor one that never invalidates, nor one whose contents do not matter passes. 160 x 96."""
import numpy as np
import pytest

from test_gpu_skin import plant  # noqa: F401  (fixture: the small scene's plant on a chain of bones, two bends)

pytestmark = pytest.mark.gpu

W, H = 160, 96
PLANES = ("color", "emission", "albedo")
SCENES = ["scene_small", "scene_bench", "scene_cornell", "scene_nan"]
OFF, RESET, USE = 0, 1, 2


def _renderer(scene, on, depth=2, uniforms=None, **kw):
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    cfg = parameter_config()
    cfg.max_tracing_depth = depth
    r = Renderer(scene, W, H, cfg, mode="fast", aspect_corrected=True, run_taa=False, run_output=False, **kw)
    r.cache_on = on
    for p, _ in r.pt_slots:
        for name, v in (uniforms or {}).items():
            p.set_uniform_int(name, v)
        p.set_uniform_int("point_cache", 1 if on else 0)
    return r


def _last_pass(r):
    return r.pt_slots[(r.frame_index - 1) % len(r.pt_slots)][0]


def _run(gl, scene, steps, on, setup=None, plane=False, **kw):
    """steps: per frame None or a callable(r) run before the frame. Returns per frame: the planes, and a dict with
    the drawing pass's served / queued verdicts, its mode, and (plane=True) its verdict words after the frame."""
    from ptsvgf._lib import PtError

    megakernel = (kw.get("uniforms") or {}).get("pt_kernel", 0) == 1
    r = _renderer(scene, on, **kw)
    r.npix = W * H  # pixels of the rows the path tracer draws (_rows changes it)
    if setup:
        setup(r)
    frames, info = [], []
    for act in steps:
        if act:
            act(r)
        r.frame()
        pl = r.planes()
        frames.append({k: gl.readback(pl[k]) for k in PLANES})
        p = _last_pass(r)
        if megakernel:  # a pass that only ever drew with the megakernel has no wavefront state: the counts say so
            with pytest.raises(PtError) as e:
                p.point_cache_counts()
            assert e.value.code == -9  # PT_ERR_STATE (include/ptsvgf.h)
            served, queued = 0, 0
        else:
            served, queued = p.point_cache_counts()
        mode, valid = p.point_cache_mode()
        d = dict(served=served, queued=queued, mode=mode, valid=valid)
        if plane and mode != OFF:
            d["words"] = p.point_cache_read(r.npix)
        info.append(d)
    r.close()
    return frames, info


def _same(a, b, tag):
    assert len(a) == len(b)
    for f, (fa, fb) in enumerate(zip(a, b)):
        for k in PLANES:
            bad = np.argwhere(np.any(fa[k].view(np.uint32) != fb[k].view(np.uint32), axis=-1))
            assert len(bad) == 0, (tag, f, k, len(bad), bad[:5].tolist())


def _both(gl, scene, steps, tag, **kw):
    on, ion = _run(gl, scene, steps, True, **kw)
    off, ioff = _run(gl, scene, steps, False, **{k: v for k, v in kw.items() if k != "plane"})
    _same(on, off, tag)
    for f, (a, b) in enumerate(zip(ion, ioff)):
        print(tag, "frame", f, "on", {k: a[k] for k in ("served", "queued", "mode")}, "off queued", b["queued"])
        assert b["served"] == 0 and b["mode"] == OFF, (tag, f, b)
        assert a["served"] + a["queued"] == b["queued"], (tag, f, a, b)  # every verdict is served or queued
    return on, off, ion, ioff


def _known(words):
    return words & np.uint16(0xF)


# ------------------------------------------------------------------ static ---
@pytest.mark.parametrize("scene_name", SCENES)
def test_static_frames_serve_more_and_more(gpu, scene_name, request):
    n = 12
    on, _, ion, _ = _both(gpu, request.getfixturevalue(scene_name), [None] * n, scene_name, plane=True)
    assert [i["mode"] for i in ion] == [OFF, RESET] + [USE] * (n - 2)
    assert ion[0]["served"] == 0 and ion[1]["served"] == 0
    assert ion[1]["queued"] > 0
    assert all(i["served"] > 0 for i in ion[2:]), [i["served"] for i in ion]
    assert ion[-1]["queued"] < ion[1]["queued"]
    prev = None
    for f in range(1, n):
        w = ion[f]["words"]
        assert not (w & np.uint16(0x700)).any(), f  # every queued ray's verdict came back: nothing is left pending
        assert not (w & np.uint16(0xF800)).any(), f
        assert not ((w >> 4) & 0xF & ~_known(w)).any(), f  # an occluded bit only under a known bit
        if prev is not None:
            assert not (_known(prev) & ~_known(w)).any(), f  # the known bits only grow
        prev = w
    assert (np.unpackbits(_known(ion[1]["words"]).astype(np.uint8)).reshape(-1, 8).sum(1) <= 1).all()  # the reset frame
    assert _known(ion[-1]["words"]).astype(np.int64).sum() > _known(ion[1]["words"]).astype(np.int64).sum()
    for f in range(1, n):  # the frames are not copies of each other: the counter moved on
        assert not np.array_equal(on[f]["color"], on[f - 1]["color"]), f


def test_flipped_verdicts_change_the_picture(gpu, scene_small):
    """After 6 static frames every known verdict's occluded bit is flipped in the plane: the next frame must differ
    from the switch-off run's, or the equality the other tests assert would prove nothing."""
    def flip(r):
        if not r.cache_on:
            return
        p = _last_pass(r)
        w = p.point_cache_read(W * H)
        assert _known(w).any()
        p.point_cache_write(w ^ (_known(w) << np.uint16(4)))

    steps = [None] * 6 + [flip]
    on, ion = _run(gpu, scene_small, steps, True)
    off, _ = _run(gpu, scene_small, steps, False)
    _same(on[:6], off[:6], "before the flip")
    assert ion[6]["mode"] == USE and ion[6]["served"] > 0
    assert not np.array_equal(on[6]["color"], off[6]["color"])
    for k in ("emission", "albedo"):
        assert np.array_equal(on[6][k], off[6][k])


# ------------------------------------------------------------ invalidation ---
def _eye_move(r):
    r.camera.cam_position = (r.camera.cam_position + np.array([0.03, 0.01, -0.02], np.float32)).astype(np.float32)


def _rotate(r):
    from ptsvgf.camera import look_at

    r.camera.cam_view_mat = look_at(r.camera.cam_position, [0.1, -0.05, 0.0], [0, 1, 0])


def _uni(name, v):
    def act(r):
        for p, _ in r.pt_slots:
            p.set_uniform_int(name, v)
    return act


def _rows(y0, y1):
    def act(r):
        for p, _ in r.pt_slots:
            p.set_rows(y0, y1)
        r.npix = W * (y1 - y0)
    return act


def _bits_set(words):
    return np.unpackbits(_known(words).astype(np.uint8)).reshape(-1, 8).sum(1)


def _check_words(ion, first, tag):
    """The plane from frame `first` on, whose first frame that touches it must be a reset: that frame leaves at most
    one known light per pixel (the one whose ray it queued), and f frames later a pixel knows at most f + 1: no bit
    from before the reset survives into a use frame. Nothing is ever left pending, an occluded bit stands only under
    a known bit, and the known bits only grow."""
    prev, age = None, 0
    for f in range(first, len(ion)):
        if ion[f]["mode"] == OFF:
            assert prev is None, (tag, f)
            continue
        assert ion[f]["mode"] == (RESET if prev is None else USE), (tag, f)
        w = ion[f]["words"]
        assert not (w & np.uint16(0xFF00)).any(), (tag, f)
        assert not ((w >> 4) & 0xF & ~_known(w)).any(), (tag, f)
        age += 1
        assert (_bits_set(w) <= age).all(), (tag, f, int(_bits_set(w).max()))
        if prev is not None:
            assert not (_known(prev) & ~_known(w)).any(), (tag, f)
        prev = w
    assert prev is not None and _known(prev).any(), tag


def _poisoned(act):
    """`act`, after every word of the plane is overwritten with "all four lights known and occluded": a reset that
    failed to clear a word would serve these, and the frames would differ from the switch-off run's."""
    def both(r):
        if r.cache_on:
            _last_pass(r).point_cache_write(np.full(r.npix, 0xFF, np.uint16))
        return act(r)
    return both


def _move_light(r):
    """The pointLights buffer uploaded again (a new texture buffer) with one light moved."""
    lights = np.array(r.scene.lights, np.float32, copy=True)
    lights[1, :3] += np.float32(0.5)
    from ptsvgf import gl

    r.pointLightBuffer = gl.texture_buffer(lights)
    r._owned.append(r.pointLightBuffer)


def _check_invalidation(gpu, scene, act, tag, expect_after, **kw):
    """Three static frames, the change, three more. expect_after: the modes of the four frames from the change on."""
    steps = [None] * 3 + [_poisoned(act)] + [None] * 3
    on, _, ion, _ = _both(gpu, scene, steps, tag, plane=True, **kw)
    assert [i["mode"] for i in ion[:3]] == [OFF, RESET, USE], tag
    _check_words(ion[:3], 0, tag)
    _check_words(ion, 3, tag)
    assert ion[2]["served"] > 0
    modes = [i["mode"] for i in ion[3:]]
    assert modes == expect_after, (tag, modes)
    for i in ion[3:]:
        if i["mode"] != USE:
            assert i["served"] == 0, (tag, i)
    return on, ion


@pytest.mark.parametrize("change", [_eye_move, _rotate], ids=["eye", "rotation"])
def test_camera_change(gpu, scene_small, change):
    _check_invalidation(gpu, scene_small, change, change.__name__, [OFF, RESET, USE, USE])


def _dynamic(r, scene, plant):
    r.rebuild_bvh(raster=scene.raster, leaf_n=8, ploc_radius=16)
    r.set_skin(*plant["skin"])


@pytest.mark.parametrize("kind", ["refit", "pose", "skin", "rebuild"])
def test_geometry_change(gpu, scene_small, plant, kind):  # noqa: F811
    from ptsvgf.scene import transform

    s = scene_small
    change = {
        "refit": lambda r: r.refit_bvh(plant["tris"][0], raster=plant["lists"][0], prev_raster=s.raster),
        "pose": lambda r: r.pose_objects({2: transform(rot=(0, 5, 0), trans=(0, 0.05, 0))}),
        "skin": lambda r: r.skin_objects(plant["bends"][1]),
        "rebuild": lambda r: r.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16) and None,
    }[kind]
    _check_invalidation(gpu, s, change, kind, [OFF, RESET, USE, USE], setup=lambda r: _dynamic(r, s, plant))


def test_light_moved(gpu, scene_small):
    """The first hit is what it was (the stage is reused), the verdicts are not: the plane is reset at once."""
    _check_invalidation(gpu, scene_small, _move_light, "light moved", [RESET, USE, USE, USE])


def test_fewer_lights(gpu, scene_small):
    _check_invalidation(gpu, scene_small, _uni("pointLightSize", 2), "pointLightSize 4 -> 2", [RESET, USE, USE, USE])


def test_other_rows(gpu, scene_small):
    """Another row range reallocates the wavefront state (and the plane with it)."""
    steps = [None] * 3 + [_rows(24, 70)] + [None] * 2
    _, _, ion, _ = _both(gpu, scene_small, steps, "rows", plane=True)
    assert [i["mode"] for i in ion] == [OFF, RESET, USE, OFF, RESET, USE]
    _check_words(ion[:3], 0, "rows")
    _check_words(ion, 3, "rows")
    assert ion[3]["served"] == 0 and ion[4]["served"] == 0 and ion[5]["served"] > 0


def test_shadow_tree_off(gpu, scene_small):
    """shadow_tree 1 -> 0: the shadow rays walk the reference tree; the trees bound are part of the primary key."""
    _check_invalidation(gpu, scene_small, _uni("shadow_tree", 0), "shadow_tree", [OFF, RESET, USE, USE])


def test_point_bins_switched_between_static_frames(gpu, scene_small):
    """Who decides a point-light ray (the lights' triangle bins or the walk) is part of the cache's key: the switch
    resets the plane, so a verdict always comes from the launches of its own setting. (One frame at a time the renderer
    sets point_bins = 0: the sequence starts with it set.)"""
    _check_invalidation(gpu, scene_small, _uni("point_bins", 0), "point_bins", [RESET, USE, USE, USE],
                        uniforms={"point_bins": 1})


def _depth(d):
    def act(r):
        r.cfg.max_tracing_depth = d
    return act


def test_depth_zero_between_static_frames(gpu, scene_small):
    """max_tracing_depth 2 -> 0 -> 2 from a standing view. A draw of no bounce launches no shade, so it cannot reset
    the plane and must not count as the draw that did: it is bypassed, and the first draw with a bounce again resets.
    The plane is poisoned before the depth-0 frames: served as verdicts, those words would change the picture."""
    steps = [None] * 3 + [_poisoned(_depth(0)), None, _depth(2), None, None]
    _, _, ion, _ = _both(gpu, scene_small, steps, "depth 0", plane=True)
    assert [i["mode"] for i in ion] == [OFF, RESET, USE, OFF, OFF, RESET, USE, USE]
    assert not ion[3]["valid"] and not ion[4]["valid"]
    assert ion[5]["served"] == 0 and ion[6]["served"] > 0
    _check_words(ion, 3, "depth 0")


# ---------------------------------------------------------- configurations ---
CONFIGS = {
    "depth1": dict(depth=1), "depth2": dict(depth=2), "depth3": dict(depth=3),
    "fold1": dict(uniforms={"shade_fold": 1}),
    "fork0": dict(uniforms={"trace_fork": 0}), "fork1": dict(uniforms={"trace_fork": 1}),
    "bins0": dict(uniforms={"point_bins": 0}), "bins1": dict(uniforms={"point_bins": 1}),
    "refill0": dict(uniforms={"trace_refill": 0}), "refill100": dict(uniforms={"trace_refill": 100}),
    "tiles": dict(uniforms={"tile_stride": 2, "tile_offset": 1}),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_configurations(gpu, scene_cornell, name):
    _, _, ion, _ = _both(gpu, scene_cornell, [None] * 5, name, **CONFIGS[name])
    assert [i["mode"] for i in ion] == [OFF, RESET, USE, USE, USE], name
    assert all(i["served"] > 0 for i in ion[2:]), name


def test_frames_in_flight(gpu, scene_small):
    """K = 3 slots: each slot has its own plane, stage frame and reset frame."""
    _, _, ion, _ = _both(gpu, scene_small, [None] * 12, "K=3", frames_in_flight=3)
    assert [i["mode"] for i in ion] == [OFF] * 3 + [RESET] * 3 + [USE] * 6
    assert all(i["served"] > 0 for i in ion[6:])


# ------------------------------------------------------- what bypasses it ---
BYPASS = {
    "spp2": dict(spp=2),
    "batch": dict(frames_in_flight=2, trace_batch=2),
    "megakernel": dict(uniforms={"pt_kernel": 1}),
    "no_lights": dict(uniforms={"pointLightSize": 0}),
    "five_lights": dict(uniforms={"pointLightSize": 5}),
    # the unfolded shade (shade_fold = 0, kept for A/B) has no cache code: it spilled with it
    "unfolded": dict(uniforms={"shade_fold": 0}),
}


@pytest.mark.parametrize("name", list(BYPASS))
def test_bypasses(gpu, scene_small, name):
    on, ion = _run(gpu, scene_small, [None] * 5, True, **BYPASS[name])
    off, _ = _run(gpu, scene_small, [None] * 5, False, **BYPASS[name])
    _same(on, off, name)
    assert all(i["served"] == 0 and i["mode"] == OFF and not i["valid"] for i in ion), (name, ion)


def test_statistics_bound_bypass(gpu, scene_small):
    """Trace statistics bound: the counters of the point-light rays must stay what they are, so nothing is served."""
    import torch

    buf = torch.zeros(16, dtype=torch.int64, device="cuda")

    def bind(r):
        for p, _ in r.pt_slots:
            p.set_trace_stats(buf.data_ptr(), buf.numel())

    on, ion = _run(gpu, scene_small, [None] * 4, True, setup=bind)
    off, _ = _run(gpu, scene_small, [None] * 4, False, setup=bind)
    _same(on, off, "stats")
    assert all(i["served"] == 0 and i["mode"] == OFF for i in ion), ion

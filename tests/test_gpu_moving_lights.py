"""Moving point lights (pt_lights_update, Renderer.set_lights; DESIGN.md "Moving point lights"): a light updated in
place between frames, with frames in flight, gives bit for bit the frames of fresh renderers built on the lights in
force at each frame; only the moved light's triangle bins are set aside and rebuilt, and only its verdicts are
forgotten."""
import dataclasses

import numpy as np
import pytest

from test_gpu_primary_tri import PLANES, _same

pytestmark = pytest.mark.gpu

W, H = 160, 96
NF = 6  # frames of the scenario: 0 1 | move | 2 | move + colour | 3 4 5


def _light_sets(scene):
    """The lights in force at frames 0-1, 2 and 3-5: light 1 moves twice, light 3 changes colour with the second
    move. The moved positions stay within 0.3 of the default ones, which lie clear of both scenes' geometry."""
    l0 = scene.lights.copy()
    l1 = l0.copy()
    l1[1, :3] = np.float32([-0.3, 0.9, 0.4])
    l2 = l1.copy()
    l2[1, :3] = np.float32([-0.2, 0.85, 0.6])
    l2[3, 3:] = np.float32([2.0, 9.0, 5.0])
    return l0, l1, l2


def _own(scene, lights=None):
    """A scene object of the test's own (set_lights keeps scene.lights in step: the session's fixture stays as is)."""
    return dataclasses.replace(scene, lights=(scene.lights if lights is None else lights).copy())


def _renderer(scene, **kw):
    from ptsvgf.renderer import Renderer

    return Renderer(scene, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False, **kw)


def _read(gl, r, f=None):
    if f is None:
        return {k: gl.readback(r.planes()[k]) for k in PLANES}
    _, (color, emission, albedo) = r.pt_slots[f % len(r.pt_slots)]
    return dict(zip(PLANES, (gl.readback(color), gl.readback(emission), gl.readback(albedo))))


@pytest.fixture(scope="module")
def fresh(gpu, request):
    """Per scene: frame f of a fresh renderer on the lights in force at f, every cache and the bins off."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        scene = request.getfixturevalue(name)
        sets = _light_sets(scene)
        force = [0, 0, 1, 2, 2, 2]
        frames = [None] * NF
        for si, lights in enumerate(sets):
            last = max(f for f in range(NF) if force[f] == si)
            r = _renderer(_own(scene, lights))
            for p, _ in r.pt_slots:
                for u in ("point_bins", "primary_cache", "point_cache"):
                    p.set_uniform_int(u, 0)
            for f in range(last + 1):
                r.frame()
                if force[f] == si:
                    frames[f] = _read(gpu, r)
            r.close()
        cache[name] = frames
        return frames

    return get


def _scenario(gl, scene, settle, read_each):
    """The scenario on one renderer with three frames in flight; read_each: every frame is read back as it is drawn
    (which waits for the device); else nothing waits until the end, and the three slots' last frames are read."""
    _, l1, l2 = _light_sets(scene)
    r = _renderer(_own(scene), frames_in_flight=3, light_settle=settle)
    out = []
    for f in range(NF):
        if f == 2:
            r.set_lights(l1[1:2], first=1)
        if f == 3:
            r.set_lights(l2[1:4], first=1)  # light 1 moves, 2 is rewritten as it is, 3 changes colour only
        r.frame()
        if read_each:
            out.append(_read(gl, r))
    if not read_each:
        r.flush()
        gl.sync()
        out = [_read(gl, r, f) for f in range(NF - 3, NF)]
    assert np.array_equal(r.scene.lights, l2)
    state = gl.lights_state(r.pointLightBuffer)
    r.close()
    return out, state


@pytest.mark.parametrize("settle", [0, 2])
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_equal_to_fresh_renderers(gpu, fresh, scene_name, settle, request):
    scene = request.getfixturevalue(scene_name)
    want = fresh(scene_name)
    got, state = _scenario(gpu, scene, settle, read_each=True)
    _same(got, want, f"{scene_name}/settle{settle}/read each frame")
    # light 1 moved at both updates (versions 2 and 3), light 2's rewrite and light 3's colour moved no stamp
    assert state["version"] == 3 and state["pos_stamps"] == [0, 3, 0, 0], state
    got, _ = _scenario(gpu, scene, settle, read_each=False)
    _same(got, want[NF - 3:], f"{scene_name}/settle{settle}/in flight")


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_who_decided_the_rays(gpu, scene_name, request):
    """light_settle = 2: the moved light walks (off == 2) while the others stay binned; two standing draws later its
    bins are back, around the new position."""
    scene = request.getfixturevalue(scene_name)
    _, l1, _ = _light_sets(scene)
    r = _renderer(_own(scene), frames_in_flight=3, light_settle=2)
    for _ in range(2):
        r.frame()
    r.set_lights(l1[1:2], first=1)
    st = r.trace_stats()  # the frame after the move
    per = gpu.point_bins_info(r.trianglesTextureBuffer, r.nodesTextureBuffer)["per_light"]
    print(scene_name, "after the move", st, [q["off"] for q in per])
    assert [q["off"] for q in per] == [0, 2, 0, 0], per
    assert st["shadow_point_binned"] > 0 and st["shadow_point_fallback"] > 0, st
    assert st["shadow_point_binned"] + st["shadow_point_fallback"] == st["shadow_point_rays"], st
    r.frame()
    st = r.trace_stats()  # the second standing draw after it
    per = gpu.point_bins_info(r.trianglesTextureBuffer, r.nodesTextureBuffer)["per_light"]
    print(scene_name, "settled", st, [q["off"] for q in per])
    assert [q["off"] for q in per] == [0, 0, 0, 0], per
    assert per[1]["pos"] == l1[1, :3].tolist(), per
    assert [q["pos"] for q in per] == l1[:, :3].tolist(), per
    assert st["shadow_point_rays"] > 0
    assert st["shadow_point_binned"] >= 0.9 * st["shadow_point_rays"], st
    r.close()


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_rebuilt_lists_equal_a_fresh_build(gpu, scene_name, request):
    """After one light's rebuild every light's headers and entries are bit for bit those of a full build on the same
    lights."""
    scene = request.getfixturevalue(scene_name)
    _, l1, _ = _light_sets(scene)

    def lists(r):
        tt, nt = r.trianglesTextureBuffer, r.nodesTextureBuffer
        return gpu.point_bins_info(tt, nt), [gpu.point_bins_read(tt, nt, l) for l in range(4)]

    r = _renderer(_own(scene), frames_in_flight=3, light_settle=0)
    r.frame()
    info0, before = lists(r)
    r.set_lights(l1[1:2], first=1)
    r.frame()
    info1, got = lists(r)
    r.close()
    f = _renderer(_own(scene, l1), frames_in_flight=3)
    f.frame()
    info2, want = lists(f)
    f.close()
    assert info1["bytes"] == info2["bytes"] and info1["cap"] == info2["cap"]
    for l in range(4):
        a, b = info1["per_light"][l], info2["per_light"][l]
        assert a == b, (l, a, b)
        assert a["off"] == 0 and a["entries"] > 0
        assert np.array_equal(got[l][0], want[l][0]), (l, "headers")
        assert got[l][1].shape == want[l][1].shape == (a["entries"], 2)
        assert np.array_equal(got[l][1], want[l][1]), (l, "entries")
        if l != 1:  # the lights that stood kept their sections
            assert info0["per_light"][l] == a
            assert np.array_equal(before[l][0], got[l][0]) and np.array_equal(before[l][1], got[l][1])
    assert info0["per_light"][1]["pos"] != info1["per_light"][1]["pos"]
    assert not np.array_equal(before[1][0], got[1][0])  # (the test would pass on lists that never changed)


def test_verdict_cache_forgets_one_light(gpu, scene_small):
    """One frame at a time the renderer turns the bins off and the verdict cache still runs: after light 2 moves, the
    next draw forgets light 2 alone."""
    l0 = scene_small.lights.copy()
    moved = l0[2:3].copy()
    moved[0, :3] = np.float32([-0.3, 0.9, 0.6])
    recoloured = l0[3:4].copy()
    recoloured[0, 3:] = np.float32([2.0, 9.0, 5.0])

    def run(cache_on):
        r = _renderer(_own(scene_small), frames_in_flight=1)
        pt = r.pt_slots[0][0]
        if not cache_on:
            pt.set_uniform_int("point_cache", 0)
        notes, frames = [], []
        for f in range(9):
            if f == 6:
                r.set_lights(moved, first=2)
            if f == 8:
                r.set_lights(recoloured, first=3)
            r.frame()
            if f >= 5:
                frames.append(_read(gpu, r))
                if cache_on:
                    served, queued = pt.point_cache_counts()
                    notes.append(dict(f=f, mode=pt.point_cache_mode(), forgot=pt.point_cache_forgotten(),
                                      served=served, queued=queued, words=pt.point_cache_read(W * H)))
        r.close()
        return frames, notes

    want, _ = run(False)
    got, notes = run(True)
    for n in notes:
        print({k: v for k, v in n.items() if k != "words"})
    _same(got, want, "verdict cache")
    before, after, stood, colour = notes  # frames 5, 6 (after the move), 7, 8 (after the colour change)
    assert before["mode"] == (2, True) and before["forgot"] == 0
    assert after["mode"] == (2, True) and after["forgot"] == 1 << 2
    assert after["served"] > 0  # the other lights' verdicts still came from the cache
    # every word lost light 2's verdict at the top of the draw, so the words that know it now are this draw's own
    # rays: the pixels that picked light 2 and hit a surface
    picked = int(np.count_nonzero(after["words"] & 0b0100))
    surface = int(np.count_nonzero(before["words"] & 0b1111))
    print("picked light 2:", picked, "of", surface, "pixels with a verdict")
    assert picked > 0 and after["queued"] >= picked
    # the other lights' bits are what they were, but for the verdicts this draw added
    known = before["words"] & np.uint16(0b1011)
    assert np.array_equal(after["words"] & known, known)
    assert np.array_equal((after["words"] >> 4) & known, (before["words"] >> 4) & known)
    assert stood["forgot"] == 0 and stood["mode"] == (2, True)
    # a colour-only update forgets nothing and queues no more rays than the draw before it
    assert colour["mode"] == (2, True) and colour["forgot"] == 0
    assert colour["queued"] <= stood["queued"]


def test_no_update_control(gpu, scene_small):
    """A renderer that never calls set_lights: the bins' report and the cache behave as before."""
    r = _renderer(_own(scene_small), frames_in_flight=3)
    for _ in range(4):
        r.frame()
    r.flush()
    per = gpu.point_bins_info(r.trianglesTextureBuffer, r.nodesTextureBuffer)["per_light"]
    assert [q["off"] for q in per] == [0, 0, 0, 0], per
    assert [q["pos"] for q in per] == scene_small.lights[:, :3].tolist()
    assert all(set(q) == {"off", "entries", "list_bytes", "catch_all", "pos", "magnitude", "large"} for q in per), per
    assert [p.point_cache_forgotten() for p, _ in r.pt_slots] == [0, 0, 0]
    assert gpu.lights_state(r.pointLightBuffer) == {"version": 1, "pos_stamps": [0, 0, 0, 0], "device_versions": 1}
    r.close()


def test_updates_reuse_their_device_versions(gpu, scene_small):
    """After the first few updates an update allocates nothing: a version no draw reads any more is taken again."""
    r = _renderer(_own(scene_small), frames_in_flight=3, light_settle=2)
    rec = scene_small.lights[0:1].copy()

    def step(i):
        rec[0, 0] = np.float32(0.5 + 0.01 * i)
        r.set_lights(rec, first=0)
        r.frame()

    for i in range(4):  # nothing waits: the draws in flight hold their versions
        step(i)
    r.flush()
    gpu.sync()
    n0 = gpu.lights_state(r.pointLightBuffer)["device_versions"]
    for i in range(4, 10):
        step(i)
        r.flush()
        gpu.sync()
    state = gpu.lights_state(r.pointLightBuffer)
    assert state["device_versions"] == n0 <= 6, (n0, state)
    assert state["version"] == 11 and state["pos_stamps"] == [11, 0, 0, 0], state
    r.close()


def test_argument_errors(gpu, scene_small):
    from ptsvgf._lib import PtError

    buf = gpu.texture_buffer(scene_small.lights)
    tex = gpu.getTextureRGB32F(4, 4)
    one = scene_small.lights[:1]
    try:
        with pytest.raises(PtError) as e:
            gpu.lights_update(tex, 0, one)
        assert e.value.code == -1  # PT_ERR_INVALID_HANDLE: not a texture buffer
        with pytest.raises(PtError) as e:
            gpu.lights_update(987654, 0, one)
        assert e.value.code == -1
        for first, lights in ((4, one), (3, scene_small.lights[:2]), (5, one)):
            with pytest.raises(PtError) as e:
                gpu.lights_update(buf, first, lights)
            assert e.value.code == -6, first  # PT_ERR_ARG: outside the buffer
        assert gpu.lights_state(buf)["version"] == 1  # nothing was written
        gpu.lights_update(buf, 3, one)
        assert np.array_equal(gpu.buffer_readback(buf).reshape(-1, 6),
                              np.concatenate([scene_small.lights[:3], one]))
    finally:
        gpu.destroy_texture(buf)
        gpu.destroy_texture(tex)


# ------------------------------------------------------- large cell boxes ---
@pytest.mark.parametrize("scene_name,R,large", [("scene_cornell", 128, True), ("scene_small", 4, False)],
                         ids=["cornell-R128", "small-R4"])
def test_large_boxes_binned_by_a_wave(gpu, scene_name, R, large, request):
    """A (triangle, face) box of more than 64 cells is binned by a wave (pb_bin_large): the Cornell box's walls at
    R = 128 for every light; never at R = 4, where a face has 16 cells. Same planes as the walk either way."""
    from test_gpu_point_bins import _check_stats, _pt
    from test_gpu_primary_tri import MOVES

    scene = request.getfixturevalue(scene_name)
    u = {"point_bins_r": R}
    want, st0 = _pt(gpu, scene, W, H, 0, MOVES[:2], uniforms=u)
    got, st1 = _pt(gpu, scene, W, H, 1, MOVES[:2], uniforms=u)
    _same(got, want, f"{scene_name}/R{R}")
    _check_stats(st1, st0, f"{scene_name}/R{R}")
    assert st1["shadow_point_binned"] > 0, st1
    info = st1["bins_info"]
    assert info["R"] == R
    per = info["per_light"]
    print(scene_name, R, [(q["off"], q["large"], q["entries"]) for q in per])
    assert [q["off"] for q in per] == [0, 0, 0, 0], per
    if large:
        assert all(q["large"] > 0 for q in per), per
    else:
        assert all(q["large"] == 0 for q in per), per

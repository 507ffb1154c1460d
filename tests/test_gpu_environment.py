"""Environment edits in place (pt_environment_update, Renderer.set_environment; DESIGN.md "Environment edits"): the
map changed between frames, with frames in flight, gives bit for bit the frames of fresh renderers constructed on
(X, hdr_cache(X)) for the map X in force at each frame; nothing that does not read the environment is rebuilt or
forgotten, and the device versions stay bounded."""
import dataclasses

import numpy as np
import pytest

from test_gpu_primary_tri import PLANES, _same

pytestmark = pytest.mark.gpu

W, H = 160, 96
NF = 6  # frames of the scenario: 0 1 | A | 2 | B | 3 4 5
FORCE = [0, 0, 1, 2, 2, 2]


def _maps(scene):
    """The scene's own map, A (turned a third, tinted and brightened) and B (a small sun on a dim sky)."""
    m0 = np.array(scene.hdr, np.float32, copy=True)
    h, w, _ = m0.shape
    a = np.ascontiguousarray(np.roll(m0, w // 3, axis=1) * np.array([1.6, 1.0, 0.5], np.float32))
    b = np.ascontiguousarray(m0[::-1] * np.float32(0.25))
    b[(2 * h) // 3:(2 * h) // 3 + 3, w // 5:w // 5 + 4] = np.array([900.0, 700.0, 400.0], np.float32)
    return m0, a, b


def _own(scene, hdr=None):
    """A scene object of the test's own (set_environment keeps scene.hdr in step: the fixture stays as it is)."""
    from ptsvgf.scene import hdr_cache

    if hdr is None:
        return dataclasses.replace(scene, hdr=scene.hdr.copy(), cache=scene.cache.copy())
    return dataclasses.replace(scene, hdr=hdr.copy(), cache=hdr_cache(hdr))


def _renderer(scene, merge=1, **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False, **kw)
    for p, _ in r.pt_slots:
        p.set_uniform_int("hdr_merge", merge)
    return r


def _all_off(r):
    for p, _ in r.pt_slots:
        for u in ("point_bins", "primary_cache", "point_cache", "reuse_static"):
            p.set_uniform_int(u, 0)


def _read(gl, r, f=None):
    if f is None:
        return {k: gl.readback(r.planes()[k]) for k in PLANES}
    _, (color, emission, albedo) = r.pt_slots[f % len(r.pt_slots)]
    return dict(zip(PLANES, (gl.readback(color), gl.readback(emission), gl.readback(albedo))))


@pytest.fixture(scope="module")
def fresh(gpu, request):
    """Per scene, sample count and hdr_merge: frame f of a fresh renderer, every cache and the bins off, constructed on
    (X, hdr_cache(X)) for the map X in force at f."""
    cache = {}

    def get(name, spp, merge):
        key = (name, spp, merge)
        if key in cache:
            return cache[key]
        scene = request.getfixturevalue(name)
        frames = [None] * NF
        for si, m in enumerate(_maps(scene)):
            last = max(f for f in range(NF) if FORCE[f] == si)
            r = _renderer(_own(scene, m), merge=merge, spp=spp)
            _all_off(r)
            for f in range(last + 1):
                r.frame()
                if FORCE[f] == si:
                    frames[f] = _read(gpu, r)
            r.close()
        cache[key] = frames
        return frames

    return get


def _scenario(gl, scene, spp, merge, read_each, device=False):
    """The scenario on one renderer with three frames in flight; read_each: every frame is read back as it is drawn
    (which waits for the device); else nothing waits until the end, and the three slots' last frames are read."""
    _, a, b = _maps(scene)
    if device:
        import torch

        a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    r = _renderer(_own(scene), merge=merge, frames_in_flight=3, spp=spp)
    out = []
    for f in range(NF):
        if f == 2:
            r.set_environment(a)
        if f == 3:
            r.set_environment(b)
        r.frame()
        if read_each:
            out.append(_read(gl, r))
    if not read_each:
        r.flush()
        gl.sync()
        out = [_read(gl, r, f) for f in range(NF - 3, NF)]
    state = gl.environment_state(r.hdrMap)
    hdr = None if device else r.scene.hdr
    assert r.scene.cache is None
    r.close()
    return out, state, hdr


@pytest.mark.parametrize("merge", [1, 0])
@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_equal_to_fresh_renderers(gpu, fresh, scene_name, spp, merge, request):
    scene = request.getfixturevalue(scene_name)
    want = fresh(scene_name, spp, merge)
    # the edits are visible at all: the yardstick's frames differ across them
    assert not np.array_equal(want[1]["color"], want[2]["color"])
    assert not np.array_equal(want[2]["color"], want[3]["color"])
    tag = f"{scene_name}/spp{spp}/merge{merge}"
    got, state, hdr = _scenario(gpu, scene, spp, merge, read_each=True)
    _same(got, want, tag + "/read each frame")
    assert state["version"] == 4, state  # the creation's 1, the constructor's upload, two updates
    assert np.array_equal(hdr.view(np.uint32), _maps(scene)[2].view(np.uint32))
    assert np.array_equal(scene.hdr.view(np.uint32), _maps(scene)[0].view(np.uint32))  # the fixture stands
    got, _, _ = _scenario(gpu, scene, spp, merge, read_each=False, device=(spp == 2))
    _same(got, want[NF - 3:], tag + "/in flight")


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_nothing_else_is_invalidated(gpu, scene_name, request):
    """A standing view, three slots: after an update the trees, the bins, the verdicts, the primary hit and the
    G-buffer stand."""
    scene = request.getfixturevalue(scene_name)
    _, a, _ = _maps(scene)
    r = _renderer(_own(scene), frames_in_flight=3)
    tt, nt = r.trianglesTextureBuffer, r.nodesTextureBuffer

    def bins():
        info = gpu.point_bins_info(tt, nt)
        return info["bytes"], info["per_light"]

    def slots(what):
        return [what(p) for p, _ in r.pt_slots]

    for _ in range(6):
        r.frame()
    r.flush()
    gpu.sync()
    bins0 = bins()
    vers0 = [gpu.lights_state(t)["version"] for t in (tt, nt)]  # (Texture::version of any texture buffer)
    stage0 = slots(lambda p: p.stage_counts())
    gbuf0 = [p.stage_counts() for p in r.init_pass]
    env0 = gpu.environment_state(r.hdrMap)["version"], gpu.environment_state(r.hdrCache)["version"]
    r.set_environment(a)
    assert (gpu.environment_state(r.hdrMap)["version"], gpu.environment_state(r.hdrCache)["version"]) == \
        (env0[0] + 1, env0[1] + 1)
    for f in range(6):
        r.frame()
        r.flush()
        gpu.sync()
        p = r.pt_slots[f % 3][0]
        assert p.point_cache_forgotten() == 0, f
        assert p.point_cache_mode() == (2, True), f
    # the primary stage did not run again, nor a G-buffer draw; the bins are the same lists
    stage1 = slots(lambda p: p.stage_counts())
    assert [s[0] for s in stage1] == [s[0] for s in stage0], (stage0, stage1)
    assert [s[1] for s in stage1] == [s[1] + 2 for s in stage0], (stage0, stage1)
    gbuf1 = [p.stage_counts() for p in r.init_pass]
    assert [g[0] for g in gbuf1] == [g[0] for g in gbuf0], (gbuf0, gbuf1)
    assert bins() == bins0
    assert [gpu.lights_state(t)["version"] for t in (tt, nt)] == vers0
    # and the frames are the new environment's
    want = _renderer(_own(scene, a))
    _all_off(want)
    for _ in range(12):
        want.frame()
    _same([_read(gpu, r)], [_read(gpu, want)], f"{scene_name}/standing")
    want.close()
    r.close()


def test_no_allocation_in_steady_state(gpu, scene_small):
    """Forty updates over forty frames with frames in flight: at most frames_in_flight + 2 device versions (one per
    slot's queued reader, the current one, the textures' own set aside), staging slots no more, none added late."""
    k = 3
    r = _renderer(_own(scene_small), frames_in_flight=k)
    m0 = _maps(scene_small)[0]
    r.frame()
    st = gpu.environment_state(r.hdrMap)
    assert st["device_versions"] == 1 and st["staging_slots"] == 0, st
    counts = []
    for i in range(40):
        r.set_environment(np.roll(m0, 5 * (i + 1), axis=1))
        r.frame()
        # the first half waits once the three slots are full: every queued draw holds the version it was issued with;
        # the second half waits every frame, so each update finds a version nothing reads
        if i >= 20 or i % k == k - 1:
            r.flush()
            gpu.sync()
        counts.append(gpu.environment_state(r.hdrMap))
    print(counts)
    assert all(c["device_versions"] <= k + 2 for c in counts), counts
    assert all(c["staging_slots"] <= k + 1 for c in counts), counts
    assert len({c["device_versions"] for c in counts[10:]}) == 1, counts
    assert len({c["staging_slots"] for c in counts[10:]}) == 1, counts
    assert counts[-1]["version"] == 42  # the creation's 1, the constructor's upload, forty updates
    r.close()

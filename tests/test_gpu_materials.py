"""Material edits in place (pt_materials_update, Renderer.set_materials; DESIGN.md "Material edits"): an object's
material changed between frames, with frames in flight, gives bit for bit the frames of fresh renderers built on
tests/materials_ref.py's buffer for the materials in force at each frame; nothing that reads geometry alone is rebuilt
or forgotten, and on a standing view each slot pays one full first-hit draw."""
import dataclasses

import numpy as np
import pytest

from materials_ref import materials_ref
from test_gpu_primary_tri import PLANES, _same

pytestmark = pytest.mark.gpu

W, H = 160, 96
NF = 6  # frames of the scenario: 0 1 | A | 2 | A again, B emissive | 3 4 5
FORCE = [0, 0, 1, 2, 2, 2]
FH_FULL, FH_KEEP = 1, 2
FH_R_NONE, FH_R_EMISSION, FH_R_ALBEDO = 0, 15, 16
AB = {"scene_small": (1, 2), "scene_cornell": (1, 0), "textured": (1, 0)}  # the objects A and B of each scene


def _mat(**kw):
    from ptsvgf.scene import material

    return material(**kw)


def _edits(name):
    """The edits before frames 2 and 3, as {object: material18}."""
    a, b = AB[name]
    return ({a: _mat(baseColor=(0.15, 0.35, 0.9), roughness=0.15, metallic=0.2)},
            {a: _mat(baseColor=(0.9, 0.2, 0.25), roughness=0.7, specular=0.2, clearcoat=0.5),
             b: _mat(baseColor=(0.6, 0.6, 0.5), emissive=(1.5, 1.0, 0.5), roughness=0.5)})


def _patched(tri, edit):
    for o, m in edit.items():
        tri = materials_ref(tri, o, m[None])
    return tri


def _own(scene, tri=None):
    """A scene object of the test's own (set_materials keeps scene.tri_enc in step: the fixture stays as it is)."""
    return dataclasses.replace(scene, tri_enc=(scene.tri_enc if tri is None else tri).copy())


def _renderer(scene, **kw):
    from ptsvgf.renderer import Renderer

    return Renderer(scene, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False, **kw)


def _all_off(r):
    for p, _ in r.pt_slots:
        for u in ("point_bins", "primary_cache", "point_cache", "reuse_static"):
            p.set_uniform_int(u, 0)


def _read(gl, r, f=None):
    if f is None:
        return {k: gl.readback(r.planes()[k]) for k in PLANES}
    _, (color, emission, albedo) = r.pt_slots[f % len(r.pt_slots)]
    return dict(zip(PLANES, (gl.readback(color), gl.readback(emission), gl.readback(albedo))))


def _scene_of(request, name):
    if name == "textured":
        from ptsvgf.scene import build_scene

        return build_scene("textured", hdr_size=(128, 64))
    return request.getfixturevalue(name)


@pytest.fixture(scope="module")
def fresh(gpu, request):
    """Per scene and sample count: frame f of a fresh renderer, every cache and the bins off, built on materials_ref's
    buffer for the materials in force at f."""
    cache = {}

    def get(name, spp):
        if (name, spp) in cache:
            return cache[name, spp]
        scene = _scene_of(request, name)
        e1, e2 = _edits(name)
        t1 = _patched(scene.tri_enc, e1)
        sets = (scene.tri_enc, t1, _patched(t1, e2))
        frames = [None] * NF
        for si, tri in enumerate(sets):
            last = max(f for f in range(NF) if FORCE[f] == si)
            r = _renderer(_own(scene, tri), spp=spp)
            _all_off(r)
            for f in range(last + 1):
                r.frame()
                if FORCE[f] == si:
                    frames[f] = _read(gpu, r)
            r.close()
        cache[name, spp] = (frames, sets)
        return cache[name, spp]

    return get


def _scenario(gl, scene, name, spp, read_each):
    """The scenario on one renderer with three frames in flight; read_each: every frame is read back as it is drawn
    (which waits for the device); else nothing waits until the end, and the three slots' last frames are read."""
    e1, e2 = _edits(name)
    r = _renderer(_own(scene), frames_in_flight=3, spp=spp)
    out = []
    for f in range(NF):
        if f == 2:
            r.set_materials(e1)
        if f == 3:
            r.set_materials(e2)
        r.frame()
        if read_each:
            out.append(_read(gl, r))
    if not read_each:
        r.flush()
        gl.sync()
        out = [_read(gl, r, f) for f in range(NF - 3, NF)]
    tri = r.scene.tri_enc
    texels = gl.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    state = gl.materials_state(r.trianglesTextureBuffer, r.nodesTextureBuffer)
    r.close()
    return out, tri, texels, state


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_equal_to_fresh_renderers(gpu, fresh, scene_name, spp, request):
    scene = request.getfixturevalue(scene_name)
    want, sets = fresh(scene_name, spp)
    # the edits are visible at all: the yardstick's frames differ across them
    assert not np.array_equal(want[1]["albedo"], want[2]["albedo"])
    assert not np.array_equal(want[2]["emission"], want[3]["emission"])
    got, tri, texels, state = _scenario(gpu, scene, scene_name, spp, read_each=True)
    _same(got, want, f"{scene_name}/spp{spp}/read each frame")
    # the renderer's rows, the device texels and the host mirror's decode all hold the last materials
    assert np.array_equal(tri.view(np.uint32), sets[2].view(np.uint32))
    assert np.array_equal(texels.view(np.uint32), sets[2].view(np.uint32))
    assert np.array_equal(scene.tri_enc.view(np.uint32), sets[0].view(np.uint32))
    a, b = AB[scene_name]
    calls = 1 + (1 if abs(a - b) == 1 else 2)  # contiguous objects go in one call
    assert state["shade_version"] == calls, state
    got, _, _, _ = _scenario(gpu, scene, scene_name, spp, read_each=False)
    _same(got, want[NF - 3:], f"{scene_name}/spp{spp}/in flight")


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_nothing_else_is_invalidated(gpu, scene_name, request):
    """A standing view, three slots: after an update the trees, the bins, the verdicts, the primary hit and the
    G-buffer stand; each slot's next draw is a full first-hit draw, the one after keeps again."""
    scene = request.getfixturevalue(scene_name)
    e1, _ = _edits(scene_name)
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
    assert [q["off"] for q in bins0[1]] == [0, 0, 0, 0]
    stage0 = slots(lambda p: p.stage_counts())
    gbuf0 = [p.stage_counts() for p in r.init_pass]
    assert all(m == (FH_KEEP, FH_R_NONE) for m in slots(lambda p: p.first_hit_last()[:2]))
    kept0 = slots(lambda p: p.first_hit_last()[2])
    r.set_materials(e1)
    modes = []
    for f in range(6):
        r.frame()
        r.flush()
        gpu.sync()
        p = r.pt_slots[f % 3][0]
        modes.append(p.first_hit_last()[:2])
        assert p.point_cache_forgotten() == 0, f
        assert p.point_cache_mode() == (2, True), f
    print(scene_name, modes)
    for f in range(3):
        assert modes[f][0] == FH_FULL and modes[f][1] in (FH_R_EMISSION, FH_R_ALBEDO), (f, modes)
        assert modes[3 + f] == (FH_KEEP, FH_R_NONE), (f, modes)
    assert slots(lambda p: p.first_hit_last()[2]) == [k + 1 for k in kept0]
    # the primary stage did not run again, nor a G-buffer draw; the bins are the same lists
    stage1 = slots(lambda p: p.stage_counts())
    assert [s[0] for s in stage1] == [s[0] for s in stage0], (stage0, stage1)
    assert [s[1] for s in stage1] == [s[1] + 2 for s in stage0], (stage0, stage1)
    gbuf1 = [p.stage_counts() for p in r.init_pass]
    assert [g[0] for g in gbuf1] == [g[0] for g in gbuf0], (gbuf0, gbuf1)
    assert bins() == bins0
    assert [gpu.lights_state(t)["version"] for t in (tt, nt)] == vers0
    assert gpu.materials_state(tt, nt)["shade_version"] == 1
    r.close()


def test_versions_of_the_buffers_stand(gpu, scene_small):
    """The triangle buffer's version does not advance: a GPU-built pair can still be refitted after an update (the
    refit's check compares the versions the build left), and the update shows in the refitted texels."""
    scene = _own(scene_small)
    e1, _ = _edits("scene_small")
    r = _renderer(scene, frames_in_flight=3)
    r.rebuild_bvh(raster=scene.raster)
    for _ in range(3):
        r.frame()
    r.set_materials(e1)
    r.frame()
    r.pose_objects({1: np.eye(4, dtype=np.float32)})  # PT_ERR_STATE had a version moved
    r.frame()
    texels = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    want = _patched(scene_small.tri_enc, e1)
    key = lambda t: t[np.lexsort(t.view(np.uint32).T[::-1])]  # the build reorders the rows
    assert np.array_equal(key(texels).view(np.uint32), key(want).view(np.uint32))
    r.close()


def _pose_mats():
    from ptsvgf.scene import transform

    return (transform(rot=(0, 25, 0), trans=(0.1, 0.05, 0.0)), transform(rot=(10, -30, 5), trans=(-0.1, 0.1, 0.1)))


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell"])
def test_gpu_built_and_posed_scenes(gpu, scene_name, request):
    scene = request.getfixturevalue(scene_name)
    a, _ = AB[scene_name]
    e1, e2 = _edits(scene_name)
    m0, m1 = _pose_mats()

    def run(tri, edit):
        r = _renderer(_own(scene, tri), frames_in_flight=3)
        if edit is None:
            _all_off(r)
        r.rebuild_bvh(raster=scene.raster)
        r.pose_objects({a: m0})
        out = []
        r.frame()
        if edit is not None:
            r.set_materials(edit)  # the pose exists: its rest list is patched with the texels
        r.frame()
        out.append(_read(gpu, r))  # the posed texels, patched where they lie
        r.pose_objects({a: m1})
        r.frame()
        out.append(_read(gpu, r))  # posed again from the patched rest list
        if edit is not None:
            # without the pose handle: the texels show the edit until the next pose copies the rest list's over them
            gpu.materials_update(r.trianglesTextureBuffer, a, e2[a][None])
            rows = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
            assert np.array_equal(rows[rows[:, 42] == a][:, 18:36], np.tile(e2[a], (int((rows[:, 42] == a).sum()), 1)))
        r.pose_objects({a: m1})
        r.frame()
        out.append(_read(gpu, r))
        r.close()
        return out

    want = run(_patched(scene.tri_enc, e1), None)
    got = run(scene.tri_enc, e1)
    _same(got, want, f"{scene_name}/posed")


def test_skinned_scene(gpu, scene_small):
    """The small scene's plant (object 2) on a chain of four bones: an edit between two bends shows in the skinned
    texels at once and in the next bend, which skins the patched rest list."""
    from ptsvgf import skin

    s = scene_small
    tp, rp = skin.corner_positions(s.tri_enc), skin.corner_positions_raster(s.raster)
    tmask, rmask = np.repeat(s.tri_enc[:, 42] == 2.0, 3), np.repeat(s.raster_obj == 2, 3)
    lo, hi = tp[tmask].min(axis=0), tp[tmask].max(axis=0)
    base = np.array([(lo[0] + hi[0]) / 2, lo[1], (lo[2] + hi[2]) / 2])
    tip = np.array([base[0], hi[1], base[2]])
    tb, tw = skin.chain_weights(tp, base, tip, 4, tmask)
    rb, rw = skin.chain_weights(rp, base, tip, 4, rmask)
    bends = [skin.chain_bones(base, tip, 4, deg, (0, 0, 1)) for deg in (6.0, 12.0)]
    edit = {2: _mat(baseColor=(0.8, 0.3, 0.6), roughness=0.3, sheen=0.6), 1: _mat(baseColor=(0.2, 0.3, 0.8))}

    def run(tri, e):
        r = _renderer(_own(s, tri), frames_in_flight=3)
        if e is None:
            _all_off(r)
        r.rebuild_bvh(raster=s.raster)
        r.set_skin(tb, tw, rb, rw)
        r.skin_objects(bends[0])
        r.frame()
        if e is not None:
            r.set_materials(e)
        r.frame()
        out = [_read(gpu, r)]
        r.skin_objects(bends[1])
        r.frame()
        out.append(_read(gpu, r))
        r.close()
        return out

    want = run(_patched(s.tri_enc, edit), None)
    plain = run(s.tri_enc, None)
    assert not np.array_equal(want[1]["albedo"], plain[1]["albedo"])
    _same(run(s.tri_enc, edit), want, "skinned")


def test_texture_array_materials(gpu, request):
    """An object switched from constants to layer-selecting (negative) baseColor / metallic / roughness and back."""
    scene = _scene_of(request, "textured")
    table = 0  # `half`: constant baseColor and roughness
    tex = _mat(baseColor=(-1.0, -1.0, -1.0), metallic=-1.0, roughness=-1.0, specular=0.5)
    const = _mat(baseColor=(0.3, 0.5, 0.7), metallic=0.1, roughness=0.45)
    t1 = materials_ref(scene.tri_enc, table, tex[None])
    t2 = materials_ref(t1, table, const[None])
    want = []
    for tri, f in ((t1, 2), (t2, 3)):
        r = _renderer(_own(scene, tri))
        _all_off(r)
        for _ in range(f + 1):
            r.frame()
        want.append(_read(gpu, r))
        r.close()
    r = _renderer(_own(scene), frames_in_flight=3)
    got = []
    for f in range(4):
        if f == 2:
            r.set_materials({table: tex})
        if f == 3:
            r.set_materials({table: const})
        r.frame()
        if f >= 2:
            got.append(_read(gpu, r))
    r.close()
    assert not np.array_equal(want[0]["albedo"], want[1]["albedo"])
    _same(got, want, "textured")


def test_no_allocation_in_steady_state(gpu, scene_small):
    """Twelve updates with frames in flight: at most frames_in_flight + 2 device versions of the shading records (one
    per slot's queued reader, the current one, the decode's set aside), and none added over the last six."""
    k = 3
    r = _renderer(_own(scene_small), frames_in_flight=k)
    tt, nt = r.trianglesTextureBuffer, r.nodesTextureBuffer
    r.frame()
    st = gpu.materials_state(tt, nt)
    assert st["shade_version"] == 0 and st["device_versions"] == 1, st
    counts = []
    for i in range(12):
        r.set_materials({1: _mat(baseColor=(0.1 + 0.07 * i, 0.5, 0.3), roughness=0.3)})
        r.frame()
        # the first six wait once the three slots are full: every queued draw holds the version it was issued with;
        # the last six wait every frame, so each update finds a version nothing reads
        if i >= 6 or i % k == k - 1:
            r.flush()
            gpu.sync()
        counts.append(gpu.materials_state(tt, nt))
    print(counts)
    assert all(c["device_versions"] <= k + 2 for c in counts), counts
    assert len({c["device_versions"] for c in counts[5:]}) == 1, counts
    assert len({c["staging_slots"] for c in counts[5:]}) == 1, counts
    assert counts[-1]["shade_version"] == 12
    r.close()


def test_argument_errors(gpu, scene_small):
    from ptsvgf._lib import PtError

    tri = scene_small.tri_enc[:64]
    buf = gpu.texture_buffer(tri)
    ragged = gpu.texture_buffer(np.zeros(48, np.float32))  # whole texels, no whole record
    tex = gpu.getTextureRGB32F(4, 4)
    other = gpu.texture_buffer(scene_small.tri_enc[:32])
    pose = gpu.pose_create(other)
    one = _mat(baseColor=(0.2, 0.3, 0.4))[None]
    try:
        for handle, kw, code in ((tex, {}, -1), (987654, {}, -1), (buf, {"pose": 987654}, -1), (ragged, {}, -6),
                                 (buf, {"pose": pose}, -6)):
            with pytest.raises(PtError) as e:
                gpu.materials_update(handle, 0, one, **kw)
            assert e.value.code == code, (handle, kw)
        assert np.array_equal(gpu.buffer_readback(buf).reshape(-1, 45).view(np.uint32), tri.view(np.uint32))
        # a buffer no draw has decoded is no error: texels and mirror are patched
        o = int(tri[0, 42])
        gpu.materials_update(buf, o, one)
        assert np.array_equal(gpu.buffer_readback(buf).reshape(-1, 45).view(np.uint32),
                              materials_ref(tri, o, one).view(np.uint32))
    finally:
        gpu.pose_destroy(pose)
        for h in (buf, ragged, tex, other):
            gpu.destroy_texture(h)

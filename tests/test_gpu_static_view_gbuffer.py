"""G-buffer draw elision (rasterize-pass uniform reuse_static, DESIGN.md "Static view"): with the caller's statement
that nothing outside the library writes the pass's attachments, a draw whose inputs and outputs are as the pass's last
completed draw left them launches nothing. Every sequence is rendered twice, with the renderer's default (reuse_static
= 1 on its own G-buffer sets) and with both static-view switches off, and the four attachments, both compact planes and
the a-trous output of the frame drawn over them (which reads the tile flags) must agree bit for bit frame by frame; the
counters of pt_debug_stage_counts must show a draw exactly where the sequence forces one. The serial fast driver
alternates two sets: frame f draws set f % 2. 160 x 96."""
import numpy as np
import pytest

from test_gpu_skin import plant  # noqa: F401  (fixture: the small scene's plant on a chain of bones, two bends)

pytestmark = pytest.mark.gpu

W, H = 160, 96
GBUF = ("world", "normal_depth", "velocity", "fwidth")
AUX = ("world", "fwidth")


def _renderer(scene, reuse, init_uniforms=None, bound_plane=True, **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False, **kw)
    r.static_view_on = reuse
    r.bound_plane = bound_plane  # the draws also write the primary rays' compact bound plane (the driver's default: not)
    for p in r.init_pass:
        for name, v in (init_uniforms or {}).items():
            p.set_uniform_int(name, v)
        if not reuse:
            p.set_uniform_int("reuse_static", 0)
    if not reuse:
        for p, _ in r.pt_slots:
            p.set_uniform_int("primary_cache", 0)
    return r


def _counts(r):
    c = [p.stage_counts() for p in r.init_pass]
    return sum(a for a, _ in c), sum(b for _, b in c)


def _run(gl, scene, steps, reuse, setup=None, **kw):
    r = _renderer(scene, reuse, **kw)
    if setup:
        setup(r)
    frames, drawn = [], []
    for act in steps:
        if act:
            act(r)
        before = _counts(r)
        r.frame()
        pl = r.planes()
        fr = {k: gl.readback(pl[k]) for k in GBUF + ("atrous",)}
        for k in AUX:
            fr["aux_" + k] = gl.readback_aux(pl[k])
        frames.append(fr)
        after = _counts(r)
        drawn.append((after[0] - before[0], after[1] - before[1]))
    r.close()
    return frames, drawn


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(gl, scene, steps, draws, tag, **kw):
    """draws[f] = 1 where frame f's G-buffer draw must launch with reuse on, 0 where it must be elided."""
    on, d_on = _run(gl, scene, steps, True, **kw)
    off, d_off = _run(gl, scene, steps, False, **kw)
    print(tag, "draws with reuse on:", [a for a, _ in d_on])
    assert d_on == [(s, 1 - s) for s in draws], (tag, d_on)
    assert d_off == [(1, 0)] * len(steps), (tag, d_off)
    for f, (a, b) in enumerate(zip(on, off)):
        for k in a:
            assert (a[k] is None) == (b[k] is None), (tag, f, k)
            if a[k] is not None:
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (tag, f, k)
        assert (a["aux_world"] is not None) == kw.get("bound_plane", True) and a["aux_fwidth"] is not None, (tag, f)
    return on


def _vel(frames):
    """v(f, g): frames f and g hold the same motion plane."""
    return lambda f, g: bool(np.array_equal(_bits(frames[f]["velocity"]), _bits(frames[g]["velocity"])))


# ------------------------------------------------------------------ static ---
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell", "scene_nan", "scene_bench"])
def test_static_frames_draw_each_set_once(gpu, scene_name, request):
    """pre_viewproj starts at projection * view, so a set's first draw already is the static one."""
    on = _check(gpu, request.getfixturevalue(scene_name), [None] * 5, [1, 1, 0, 0, 0], scene_name)
    assert np.any(on[0]["normal_depth"][..., 3] != 1.0)  # (a surface, not background alone)


def _band(stage):
    return (24, 70)


@pytest.mark.parametrize("kw", [dict(init_uniforms={"gbuffer_mode": 0}),
                                dict(gbuffer_rows=(24, 70), stage_rows=_band),
                                dict(bound_plane=False)], ids=["ray cast", "band", "no bound plane"])
def test_ray_cast_mode_a_band_of_rows_and_no_bound_plane(gpu, scene_small, kw):
    """(The band: the SVGF stages draw the G-buffer's rows, not a multiple of the tile. An a-trous draw over other rows
    derives the tile flags again for its own, and the set's next draw then launches: the flags are part of the key.)"""
    _check(gpu, scene_small, [None] * 4, [1, 1, 0, 0], str(sorted(kw)), **kw)


# ------------------------------------------------------------ forced draws ---
def test_camera_move(gpu, scene_small):
    """The move's frame carries the old pre_viewproj (motion), the next one draws the other set from the new view,
    and the moved set is drawn once more with pre_viewproj = projection * view before both rest."""
    on = _check(gpu, scene_small, [None, None, None, lambda r: r.camera.orbit(3.0, 1.5), None, None, None, None],
                [1, 1, 0, 1, 1, 1, 0, 0], "move")
    v = _vel(on)
    assert not v(3, 4) and v(4, 5) and v(5, 6) and v(0, 2)  # motion on the move's frame alone


def _dynamic(r, scene, plant):
    r.rebuild_bvh(raster=scene.raster, leaf_n=8, ploc_radius=16)
    r.set_skin(*plant["skin"])


@pytest.mark.parametrize("kind", ["rebuild_prev", "refit", "pose", "pose_still", "skin"])
def test_geometry_change(gpu, scene_small, plant, kind):  # noqa: F811
    """A change with motion records: the frame of the change draws with them, the other set draws the new triangles,
    and the first set is drawn again without the records (object_motion is pending for one frame only). Without
    records (pose_still) each set draws the new triangles once."""
    from ptsvgf.scene import transform

    s = scene_small
    change = {
        "rebuild_prev": lambda r: r.rebuild_bvh(tri_enc=plant["tris"][0], raster=plant["lists"][0], leaf_n=8,
                                                ploc_radius=16, prev_raster=s.raster),
        "refit": lambda r: r.refit_bvh(plant["tris"][0], raster=plant["lists"][0], prev_raster=s.raster),
        "pose": lambda r: r.pose_objects({2: transform(rot=(0, 5, 0), trans=(0, 0.05, 0))}),
        "pose_still": lambda r: r.pose_objects({2: transform(rot=(0, 5, 0), trans=(0, 0.05, 0))}, motion=False),
        "skin": lambda r: r.skin_objects(plant["bends"][1]),
    }[kind]
    still = kind == "pose_still"
    on = _check(gpu, s, [None, None, None, change, None, None, None], [1, 1, 0, 1, 1, 0 if still else 1, 0], kind,
                setup=lambda r: _dynamic(r, s, plant))
    v = _vel(on)
    assert v(3, 4) == still and v(4, 5) and v(5, 6)  # the records move the change's frame alone
    assert not np.array_equal(_bits(on[2]["world"]), _bits(on[3]["world"]))


def test_upload_into_an_attachment(gpu, scene_small):
    """pt_texture_upload_rgba into the motion plane of the set frame 3 would have left alone."""
    def upload(r):
        gpu.upload_rgba(r.gbuf[3 % len(r.gbuf)]["velocity"], np.full((H, W, 4), 0.25, np.float32))

    on = _check(gpu, scene_small, [None, None, None, upload, None, None], [1, 1, 0, 1, 0, 0], "upload")
    assert _vel(on)(2, 3)  # (the draw wrote over the upload)


def test_another_pass_draws_into_an_attachment(gpu, scene_small):
    """A second rasterize pass (its own triangles, identity matrices) over the same four attachments."""
    from ptsvgf.gl import Rasterize_RenderPass

    made = []

    def other(r):
        g = r.gbuf[3 % len(r.gbuf)]
        q = Rasterize_RenderPass(r.init_pass[0].program, W, H)
        q.colorAttachments += [g["world"], g["normal_depth"], g["velocity"], g["fwidth"]]
        q.bindData(scene_small.raster)
        q.draw()
        made.append(q)

    _check(gpu, scene_small, [None, None, None, other, None, None], [1, 1, 0, 1, 0, 0], "second pass")
    for q in made:
        q.destroy()


def test_motion_bound_always_draws(gpu, scene_small):
    import torch

    bound = torch.zeros(1, dtype=torch.int32, device="cuda")

    def bind(r):
        for p in r.init_pass:
            p.set_motion_bound(bound.data_ptr())

    _check(gpu, scene_small, [None, None, None, bind, None, None], [1, 1, 0, 1, 1, 1], "motion bound")
    torch.cuda.synchronize()
    assert int(bound.item()) == 0  # (static frames: the largest |motion.y| is 0)


def test_switch_off_in_the_middle(gpu, scene_small):
    def off(r):
        for p in r.init_pass:
            p.set_uniform_int("reuse_static", 0)

    def on(r):
        for p in r.init_pass:
            p.set_uniform_int("reuse_static", 1 if r.static_view_on else 0)  # (not in the switch-off run)

    _check(gpu, scene_small, [None, None, None, off, None, on, None], [1, 1, 0, 1, 1, 0, 0], "reuse_static uniform")


def test_elided_draw_is_timed(gpu, scene_small):
    """Under profiling an elided draw still is the pass's draw: pt_pass_last_ms answers, with next to nothing."""
    from ptsvgf.renderer import Renderer

    gpu.set_profiling(True)
    try:
        r = Renderer(scene_small, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False)
        for _ in range(3):
            r.frame()
        assert r.init_pass[0].stage_counts() == (1, 1)
        assert 0.0 <= r.init_pass[0].last_ms() < 0.5
        r.close()
    finally:
        gpu.set_profiling(False)

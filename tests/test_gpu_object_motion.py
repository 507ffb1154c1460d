"""Object motion vectors (pt_raster_pass_set_prev_vertices, Renderer.rebuild_bvh(prev_raster=...)): the G-buffer
kernels against the float64 restatement (tests/object_motion_ref.py) at the project's G-buffer bar, the cases that
must not change a bit, and SVGF history following an object that moved."""

import numpy as np
import pytest

import object_motion_ref as R

pytestmark = pytest.mark.gpu

GBUF = ("world", "normal_depth", "velocity", "fwidth")
BAR = 1e-5  # the G-buffer bar of tests/test_gpu_fullsize.py, absolute, uv units (linear depth for motion.z)
CLEAR = np.array([0.2, 0.3, 0.3, 1.0], np.float32)
D = np.array([0.02, 0.03, -0.01], np.float32)  # the rigid translation of test 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _renderer(scene, W, H, gbuffer_mode=1, **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, W, H, mode="fast", run_taa=False, run_output=False, **kw)
    for p in r.init_pass:
        p.set_uniform_int("gbuffer_mode", gbuffer_mode)
    return r


def _gbuf(gpu, r):
    got = r.planes()
    return {k: gpu.readback(got[k]) for k in GBUF}


def _viewproj(r):
    from ptsvgf.camera import mat_mul

    return mat_mul(r.camera.cam_proj_mat, r.camera.cam_view_mat)


def _shift_raster(raster, d, tris=slice(None)):
    v = raster.reshape(-1, 3, 6).copy()
    v[tris, :, :3] += np.asarray(d, np.float32)
    return v.reshape(-1)


def _shift_tri_enc(tri_enc, d, sel=slice(None)):
    t = tri_enc.copy()
    t[sel, :9] += np.tile(np.asarray(d, np.float32), 3)
    return t


# ---- the rigidly translated scene_small, rendered once per G-buffer mode and shared (tests 2 and 4) ----
_translated = {}


def _translated_frames(gpu, scene, mode):
    if mode not in _translated:
        raster = _shift_raster(scene.raster, D)
        prev = _shift_raster(raster, -D)  # prev_raster = raster - d, in float32
        tri = _shift_tri_enc(scene.tri_enc, D)
        r = _renderer(scene, 160, 96, mode)
        r.rebuild_bvh(tri_enc=tri, raster=raster, leaf_n=8, ploc_radius=16)
        r.frame()
        plain = _gbuf(gpu, r)
        PV = np.array(r.pre_viewproj, np.float32)
        r.rebuild_bvh(tri_enc=tri, raster=raster, leaf_n=8, ploc_radius=16, prev_raster=prev)
        r.frame()
        moved = _gbuf(gpu, r)
        M = _viewproj(r)
        r.close()
        for d in (plain, moved):
            for a in d.values():
                a.setflags(write=False)
        _translated[mode] = dict(raster=raster, prev=prev, tri=tri, plain=plain, moved=moved, M=M, PV=PV)
    return _translated[mode]


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_stationary_is_bit_identical(gpu, scene_small, gbuffer_mode):
    """Records of a list equal to the bound one (no triangle flagged moved), and object_motion = 0 over a really
    different list: the four planes are those of a rebuild without prev_raster, bit for bit."""
    raster = scene_small.raster
    r = _renderer(scene_small, 160, 96, gbuffer_mode)
    r.rebuild_bvh(raster=raster, leaf_n=8, ploc_radius=16)
    r.frame()
    want = _gbuf(gpu, r)
    r.rebuild_bvh(raster=raster, leaf_n=8, ploc_radius=16, prev_raster=raster.copy())
    r.frame()
    same_list = _gbuf(gpu, r)
    r.object_motion = False
    r.rebuild_bvh(raster=raster, leaf_n=8, ploc_radius=16, prev_raster=_shift_raster(raster, (0.05, -0.04, 0.03)))
    r.frame()
    switched_off = _gbuf(gpu, r)
    r.close()
    for k in GBUF:
        assert np.array_equal(_bits(same_list[k]), _bits(want[k])), k
        assert np.array_equal(_bits(switched_off[k]), _bits(want[k])), k
    assert 0.05 < float(np.mean(want["normal_depth"][..., 3] != 1.0)) < 0.95


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_rigid_translation_matches_the_restatement(gpu, scene_small, gbuffer_mode):
    """Every vertex moved by d, static camera: velocity.xyz of every surface pixel against the restatement at the
    readback world position with displacement -d, at the G-buffer bar (1e-5 absolute); background keeps the clear
    colour; the other planes are those of the plain bind."""
    t = _translated_frames(gpu, scene_small, gbuffer_mode)
    got = t["moved"]
    surf = got["normal_depth"][..., 3] != 1.0
    assert 0.05 < float(np.mean(surf)) < 0.95
    want = R.motion_from_displacement(got["world"][surf][:, :3], -D.astype(np.float64), t["M"], t["PV"])
    err = np.abs(got["velocity"][surf][:, :3].astype(np.float64) - want)
    print(f"rigid translation (gbuffer_mode {gbuffer_mode}): max |velocity - restatement| = {err.max(axis=0)}, "
          f"max |velocity| = {np.abs(want).max(axis=0)}, {int(surf.sum())} surface pixels")
    assert np.abs(want[:, :2]).max() > 1e-3 and np.abs(want[:, 2]).max() > 1e-3  # the motion is there to be measured
    assert err.max() <= BAR
    assert np.all(got["velocity"][surf][:, 3] == 1.0)
    assert np.array_equal(_bits(got["velocity"][~surf]), _bits(np.broadcast_to(CLEAR, got["velocity"][~surf].shape)))
    for k in ("world", "normal_depth", "fwidth"):
        assert np.array_equal(_bits(got[k]), _bits(t["plain"][k])), k
    # the plain bind's velocity is the camera's alone: none, with a static camera
    assert np.abs(t["plain"]["velocity"][surf][:, :3]).max() < 1e-6


# ---- two quads facing the camera: a large back one, a smaller front one (raster order = emission order) ----
def _view_basis(W, H):
    from ptsvgf.camera import Camera

    cam = Camera(W, H)
    cam.update()
    eye = np.asarray(cam.cam_position, np.float64)
    f = np.asarray(cam.look_at_point, np.float64) - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, [0.0, 1.0, 0.0])
    s /= np.linalg.norm(s)
    return eye, f, s, np.cross(s, f)


BACK_DIST, FRONT_DIST = 3.0, 1.5


def _quad(eye, f, s, u, dist, hw, hh):
    c = eye + f * dist
    return np.array([c - s * hw - u * hh, c + s * hw - u * hh, c + s * hw + u * hh, c - s * hw + u * hh], np.float32)


def _two_quads(W, H):
    """Scene, and the view basis it was built in. Triangles 0, 1: the back quad; 2, 3: the front quad, vertices
    (0, 1, 2) and (0, 2, 3) of its corners; both quads perpendicular to the view axis, counter-clockwise."""
    from ptsvgf.scene import POINT_LIGHTS, Scene, SceneBuilder, env_map, hdr_cache, material, transform

    eye, f, s, u = _view_basis(W, H)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    b = SceneBuilder()
    b.add_mesh(_quad(eye, f, s, u, BACK_DIST, 2.0, 1.5), idx, material(baseColor=(0.6, 0.6, 0.6)), transform(), False, 0)
    b.add_mesh(_quad(eye, f, s, u, FRONT_DIST, 0.5, 0.4), idx, material(baseColor=(0.8, 0.3, 0.2)), transform(), False, 1)
    b.build(8)
    tri, node, raster = b.encode()
    hdr = env_map(128, 64)
    sc = Scene("two_quads", tri, node, raster, POINT_LIGHTS.copy(), hdr, hdr_cache(hdr), b.counts())
    assert sc.raster.size == 4 * 18
    return sc, (eye, f, s, u)


def _front_mask(world, eye, f):
    """Pixels of the front quad, from the world plane: nearer along the view axis than half way to the back quad."""
    depth = (world[..., :3].astype(np.float64) - eye) @ f
    surface = np.any(world[..., :3] != CLEAR[:3], axis=-1)  # the background holds the clear colour
    return surface & (depth < 0.5 * (BACK_DIST + FRONT_DIST))


def _erode(mask, r):
    """Pixels whose (2r + 1)^2 neighbourhood lies in the mask: at least r pixels from its silhouette."""
    H, W = mask.shape
    pad = np.zeros((H + 2 * r, W + 2 * r), bool)
    pad[r:r + H, r:r + W] = mask
    out = np.ones_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out &= pad[dy:dy + H, dx:dx + W]
    return out


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_per_vertex_motion_blends_over_the_triangle(gpu, gbuffer_mode):
    """One corner of the front quad moved (the corner both of its triangles share): every front-quad pixel against
    the restatement, which solves the pixel's barycentrics in float64 in the triangle that holds it; the back quad
    and the background are the unmoved frame's bits."""
    W, H = 96, 64
    sc, (eye, f, s, u) = _two_quads(W, H)
    prev = sc.raster.copy()
    cur = sc.raster.reshape(-1, 3, 6).copy()
    step = (0.12 * s + 0.07 * u - 0.15 * f).astype(np.float32)
    cur[2, 2, :3] += step  # corner 2, in triangle (0, 1, 2) ...
    cur[3, 1, :3] += step  # ... and in triangle (0, 2, 3)
    cur = cur.reshape(-1)
    r = _renderer(sc, W, H, gbuffer_mode)
    r.rebuild_bvh(raster=cur, leaf_n=8, ploc_radius=0)
    r.frame()
    plain = _gbuf(gpu, r)
    PV = np.array(r.pre_viewproj, np.float32)
    r.rebuild_bvh(raster=cur, leaf_n=8, ploc_radius=0, prev_raster=prev)
    r.frame()
    got = _gbuf(gpu, r)
    M = _viewproj(r)
    r.close()
    for k in ("world", "normal_depth", "fwidth"):
        assert np.array_equal(_bits(got[k]), _bits(plain[k])), k
    tris_c = cur.reshape(-1, 3, 6)[2:4, :, :3].astype(np.float64)
    tris_p = prev.reshape(-1, 3, 6)[2:4, :, :3].astype(np.float64)
    # the front quad's pixels: on the plane of one of its two (now folded) triangles, inside it
    P = got["world"][..., :3].astype(np.float64)
    score = []
    for k in range(2):
        uu, vv = R.barycentrics(P, tris_c[k])
        w0 = 1.0 - uu - vv
        on = tris_c[k, 0] * w0[..., None] + tris_c[k, 1] * uu[..., None] + tris_c[k, 2] * vv[..., None]
        score.append(np.linalg.norm(on - P, axis=-1) + np.maximum(0.0, -np.minimum(np.minimum(uu, vv), w0)))
    score = np.stack(score)
    which = np.argmin(score, axis=0)
    front = (got["world"][..., 3] == 1.0) & (got["normal_depth"][..., 3] != 1.0) & (score.min(axis=0) < 1e-4)
    assert front.sum() > 150 and (which[front] == 0).any() and (which[front] == 1).any()
    Pf, wf = P[front], which[front]
    want = R.motion(Pf, tris_c[wf], tris_p[wf], M, PV)
    other = R.motion(Pf, tris_c[1 - wf], tris_p[1 - wf], M, PV)
    diag = np.abs(score[0] - score[1])[front] < 1e-6  # on the shared diagonal either triangle gives the same value
    assert not diag.any() or np.abs(want[diag] - other[diag]).max() < 1e-6
    err = np.abs(got["velocity"][front][:, :3].astype(np.float64) - want)
    print(f"per-vertex motion (gbuffer_mode {gbuffer_mode}): max |velocity - restatement| = {err.max(axis=0)}, "
          f"max |velocity| = {np.abs(want).max(axis=0)}, {int(front.sum())} front-quad pixels")
    assert np.abs(want[:, :2]).max() > 1e-2 and np.abs(want[:, 2]).max() > 1e-2
    assert err.max() <= BAR
    # everything that is not the front quad: the back quad (and the background), bit for bit the unmoved frame
    back = ~front
    assert (got["normal_depth"][..., 3][back] != 1.0).sum() > 500
    assert np.array_equal(_bits(got["velocity"][back]), _bits(plain["velocity"][back]))


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_sharing_passes_and_frames_in_flight(gpu, scene_small, gbuffer_mode):
    """Two frames in flight (three G-buffer sets, sets 1 and 2 sharing set 0's triangles): the moved frame lands on
    a sharing pass and its velocity plane is test 2's; the frame after it is a stationary frame's."""
    t = _translated_frames(gpu, scene_small, gbuffer_mode)
    r = _renderer(scene_small, 160, 96, gbuffer_mode, frames_in_flight=2)
    r.frame()
    r.rebuild_bvh(tri_enc=t["tri"], raster=t["raster"], leaf_n=8, ploc_radius=16, prev_raster=t["prev"])
    assert len(r.init_pass) == 3 and r.frame_index % 3 == 1
    r.frame()
    assert r.planes()["velocity"] == r.gbuf[1]["velocity"]  # set 1's pass shares init_pass[0]'s triangles
    moved = _gbuf(gpu, r)
    r.frame()
    assert r.planes()["velocity"] == r.gbuf[2]["velocity"]
    after = _gbuf(gpu, r)
    r.close()
    for k in GBUF:
        assert np.array_equal(_bits(moved[k]), _bits(t["moved"][k])), k
        assert np.array_equal(_bits(after[k]), _bits(t["plain"][k])), k


def test_host_bound_pass_takes_the_records(gpu, scene_small):
    """The call on a pass bound on the host (pt_raster_pass_bind: another tree, another leaf order, the same original
    indices): the moved frame's planes are the device-bound renderer's, bit for bit."""
    import dataclasses

    import torch

    t = _translated_frames(gpu, scene_small, 1)
    r = _renderer(dataclasses.replace(scene_small, raster=t["raster"], tri_enc=t["tri"]), 160, 96)
    cur, prev = torch.from_numpy(t["raster"]).cuda(), torch.from_numpy(t["prev"]).cuda()
    torch.cuda.synchronize()
    r.init_pass[0].set_prev_vertices(prev.data_ptr(), cur.data_ptr(), cur.numel())
    r.frame()
    assert r.planes()["velocity"] == r.gbuf[0]["velocity"]
    got = _gbuf(gpu, r)
    r.close()
    for k in GBUF:
        assert np.array_equal(_bits(got[k]), _bits(t["moved"][k])), k


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_motion_bound_holds_the_value_written(gpu, scene_small, gbuffer_mode):
    """pt_pass_set_motion_bound with the plant lifted in y: the device word is, as float bits, the largest
    |velocity.y| over the readback's surface pixels."""
    import torch

    n_plant = int(np.sum(scene_small.tri_enc[:, 42] == 2.0))
    assert 0 < n_plant < scene_small.ntris
    plant = slice(scene_small.raster.size // 18 - n_plant, None)  # the last object emitted
    lift = (0.0, 0.05, 0.0)
    raster = _shift_raster(scene_small.raster, lift, plant)
    tri = _shift_tri_enc(scene_small.tri_enc, lift, scene_small.tri_enc[:, 42] == 2.0)
    r = _renderer(scene_small, 160, 96, gbuffer_mode)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    for p in r.init_pass:
        p.set_motion_bound(word.data_ptr())
    r.rebuild_bvh(tri_enc=tri, raster=raster, leaf_n=8, ploc_radius=16, prev_raster=scene_small.raster)
    r.frame()
    got = _gbuf(gpu, r)
    torch.cuda.synchronize()
    bound = int(word.item()) & 0xFFFFFFFF
    for p in r.init_pass:
        p.set_motion_bound(0)
    r.close()
    surf = got["normal_depth"][..., 3] != 1.0
    vy = np.abs(got["velocity"][..., 1][surf])
    assert vy.max() > 1e-2  # the plant's lift, seen from the static camera
    assert bound == int(_bits(np.array([vy.max()], np.float32))[0])


# ---- history follows the object ----
def _history_after_move(gpu, sc, basis, W, H, move, object_motion):
    """Three frames, then the front quad moved by `move` and one more frame: (front mask before, front mask after,
    history length plane after)."""
    eye, f = basis[0], basis[1]
    r = _renderer(sc, W, H)
    r.object_motion = object_motion
    for _ in range(3):
        r.frame()
    before = _front_mask(gpu.readback(r.planes()["world"]), eye, f)
    assert np.all(gpu.readback(r.planes()["reproj_moments"])[..., 2][before] == 3.0)
    r.rebuild_bvh(tri_enc=_shift_tri_enc(sc.tri_enc, move, sc.tri_enc[:, 42] == 1.0),
                  raster=_shift_raster(sc.raster, move, slice(2, 4)), leaf_n=8, ploc_radius=0, prev_raster=True)
    r.frame()
    pl = r.planes()
    after = _front_mask(gpu.readback(pl["world"]), eye, f)
    hist = gpu.readback(pl["reproj_moments"])[..., 2].copy()
    r.close()
    return before, after, hist


def test_history_follows_a_sideways_move(gpu):
    """The front quad moves about 6 pixels parallel to the image plane. With prev_raster every interior pixel (at
    least 2 pixels from the quad's silhouette) keeps its history (length 4); with object_motion = 0 the interior of
    the newly covered strip (pixels of the strip at least 2 pixels from the strip's silhouette, so that no history
    tap, which reaches one pixel, meets the quad's old pixels) restarts at 1."""
    W, H = 160, 96
    sc, basis = _two_quads(W, H)
    s = basis[2]
    pixel = 2.0 * FRONT_DIST / H  # fov 90: the frame is 2 * distance high
    move = (6.3 * pixel * s).astype(np.float32)
    res = {}
    for on in (True, False):
        before, after, hist = _history_after_move(gpu, sc, basis, W, H, move, on)
        interior = _erode(after, 2)
        assert interior.sum() >= 0.5 * after.sum() and after.sum() > 500
        strip = _erode(after & ~before, 2)
        assert strip.sum() >= 20
        res[on] = (interior, strip, hist)
    interior, strip, hist = res[True]
    assert np.all(hist[interior] == 4.0)
    interior, strip, hist = res[False]
    assert np.all(hist[strip] == 1.0)


def test_history_follows_a_move_in_depth(gpu):
    """The front quad approaches the camera by three times the depth change the reprojection test rejects at zero
    depth fwidth (|dz| / (fwidth + 0.01) > depth_threshold). With prev_raster the interior keeps its history (4);
    with object_motion = 0 every interior pixel restarts at 1."""
    from ptsvgf.camera import parameter_config

    W, H = 160, 96
    sc, basis = _two_quads(W, H)
    f = basis[1]
    step = 3.0 * 1e-2 * float(parameter_config().reproj_depth_threshold)
    assert abs(step - 0.3) < 1e-12
    move = (-step * f).astype(np.float32)
    for on in (True, False):
        before, after, hist = _history_after_move(gpu, sc, basis, W, H, move, on)
        interior = _erode(after, 2)
        assert interior.sum() >= 0.5 * after.sum() and after.sum() > before.sum() > 500
        assert np.all(hist[interior] == (4.0 if on else 1.0)), on


def test_errors_leave_the_pass_drawable(gpu, scene_small):
    """A wrong size, a sharing pass, an unbound pass and a non-raster pass: PT_ERR_ARG each, and the passes draw what
    they drew before; NULL for the previous list drops the records."""
    import ctypes as C

    import torch

    from ptsvgf._lib import PtError, pt
    from ptsvgf.gl import Rasterize_RenderPass, getShaderProgram, getTextureRGB32F

    W, H = 96, 64
    r = _renderer(scene_small, W, H)
    r.rebuild_bvh(raster=scene_small.raster, leaf_n=8, ploc_radius=16)  # init_pass[1] now shares init_pass[0]
    want = []
    for _ in range(2):
        r.frame()
        want.append(_gbuf(gpu, r))
    cur = torch.from_numpy(scene_small.raster).cuda()
    prev = torch.from_numpy(_shift_raster(scene_small.raster, (0.05, 0.0, 0.0))).cuda()
    torch.cuda.synchronize()
    n = cur.numel()
    unbound = Rasterize_RenderPass(getShaderProgram("shaders/rasterize_frag.frag", "shaders/rasterize_vert.vert"), W, H)
    tex = [getTextureRGB32F(W, H) for _ in range(4)]
    unbound.colorAttachments += tex
    for p, size in ((r.init_pass[0], n - 18), (r.init_pass[0], n + 18), (r.init_pass[1], n), (unbound, n)):
        with pytest.raises(PtError) as e:
            p.set_prev_vertices(prev.data_ptr(), cur.data_ptr(), size)
        assert e.value.code == -6
    rc = pt().pt_raster_pass_set_prev_vertices(r.pt_pass._handle(), C.c_void_p(prev.data_ptr()),
                                               C.c_void_p(cur.data_ptr()), n)
    assert rc == -6
    for k in range(2):
        r.frame()
        got = _gbuf(gpu, r)
        for key in GBUF:
            assert np.array_equal(_bits(got[key]), _bits(want[k][key])), (k, key)
    # records bound by hand draw motion (object_motion defaults to 1); NULL drops them
    r.init_pass[0].set_prev_vertices(prev.data_ptr(), cur.data_ptr(), n)
    r.frame()
    got = _gbuf(gpu, r)
    surf = got["normal_depth"][..., 3] != 1.0
    assert np.abs(got["velocity"][surf][:, 0]).max() > 1e-2
    r.init_pass[0].set_prev_vertices(None, None, 0)
    r.frame()
    got = _gbuf(gpu, r)
    for key in GBUF:
        assert np.array_equal(_bits(got[key]), _bits(want[1][key])), key
    unbound.bindData(scene_small.raster)  # the refused pass binds and draws as any other
    unbound.set_uniform_mat4("view", r.camera.cam_view_mat)
    unbound.set_uniform_mat4("projection", r.camera.cam_proj_mat)
    unbound.set_uniform_mat4("pre_viewproj", _viewproj(r))
    unbound.draw()
    assert np.array_equal(_bits(gpu.readback(tex[1])), _bits(want[0]["normal_depth"]))
    unbound.destroy()
    for h in tex:
        gpu.destroy_texture(h)
    r.close()

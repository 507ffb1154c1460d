"""Point-light shadow rays by the lights' triangle bins (pass uniform point_bins = 1: kernels_pointbins.hip's build,
kernels_wf_trace.hip wf_shadow_point_bins) against the tree walk (point_bins = 0, which test_gpu_parity.py and
test_gpu_fullsize.py pin to the oracle): the same verdict for the same ray, so the path tracer's planes must be
bit-identical over every pixel, and the counters that do not say which path decided a ray must be equal."""
import dataclasses

import numpy as np
import pytest

from test_gpu_lbvh_trees import _moved
from test_gpu_primary_tri import MOVES, PLANES, _same

pytestmark = pytest.mark.gpu

W, H = 160, 96
KEEP = ("shadow_rays", "shadow_point_rays", "shadow_occluded")


def _pt(gl, scene, w, h, bins, moves, depth=2, nlights=None, rows=None, stats=True, uniforms=None, prepare=None,
        **kw):
    """Frames of `moves` with point_bins = bins; (planes per frame, trace counters of one more frame)."""
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    cfg = parameter_config()
    cfg.max_tracing_depth = depth
    r = Renderer(scene, w, h, cfg, mode="fast", aspect_corrected=w != h, run_taa=False, run_output=False,
                 gbuffer_rows=rows, **kw)
    if prepare:
        prepare(r)
    for p, _ in r.pt_slots:
        p.set_uniform_int("point_bins", bins)
        if nlights is not None:
            p.set_uniform_int("pointLightSize", nlights)
        for name, v in (uniforms or {}).items():
            p.set_uniform_int(name, v)
        if rows is not None:
            p.set_rows(*rows)
    out = []
    for mv in moves:
        if mv:
            r.camera.orbit(*mv)
        r.frame()
        out.append({k: gl.readback(r.planes()[k]) for k in PLANES})
    st = r.trace_stats() if stats else None
    if stats and bins:
        try:
            st["bins_info"] = gl.point_bins_info(r.trianglesTextureBuffer, r.nodesTextureBuffer)
        except Exception:  # no bins were built (the path is off for this configuration)
            st["bins_info"] = None
    r.close()
    return out, st


def _check_stats(on, off, tag, binned_share=None, active=True):
    print(tag, "bins", on, "walk", off)
    for k in KEEP:
        assert on[k] == off[k], (tag, k, on[k], off[k])
    if active:  # every point-light ray was either decided by the bins or handed to the walk
        assert on["shadow_point_binned"] + on["shadow_point_fallback"] == on["shadow_point_rays"], (tag, on)
    else:
        assert on["shadow_point_binned"] == 0 and on["shadow_point_fallback"] == 0, (tag, on)
    assert off["shadow_point_binned"] == 0 and off["shadow_point_fallback"] == 0, (tag, off)
    if binned_share is not None:
        assert on["shadow_point_rays"] > 0
        assert on["shadow_point_binned"] >= binned_share * on["shadow_point_rays"], (tag, on)


@pytest.fixture(scope="module")
def walks(gpu, request):
    """The walk's frames (point_bins 0, MOVES) of a scene fixture at 160 x 96 per depth, rendered once per module."""
    cache = {}

    def get(name, depth=2):
        if (name, depth) not in cache:
            cache[name, depth] = _pt(gpu, request.getfixturevalue(name), W, H, 0, MOVES, depth=depth)
        return cache[name, depth]

    return get


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell", "scene_nan"])
def test_bins_equal_walk(gpu, walks, scene_name, depth, request):
    """The four default lights lie clear of all geometry: at least 0.9 of the point-light rays must be decided by the
    bins (a path that silently turned itself off would pass the comparison)."""
    scene = request.getfixturevalue(scene_name)
    want, st0 = walks(scene_name, depth)
    got, st1 = _pt(gpu, scene, W, H, 1, MOVES, depth=depth)
    _same(got, want, f"{scene_name}/depth{depth}")
    _check_stats(st1, st0, f"{scene_name}/depth{depth}", binned_share=0.9)


def test_dense_cells_bench_scene(gpu, scene_bench):
    """30 k triangles: the plant's cells hold long lists. Two camera states."""
    want, st0 = _pt(gpu, scene_bench, W, H, 0, MOVES[:2])
    got, st1 = _pt(gpu, scene_bench, W, H, 1, MOVES[:2])
    _same(got, want, "dense")
    _check_stats(st1, st0, "dense", binned_share=0.9)


# ------------------------------------------------------------------ edge scene ---
EW, EH = 96, 64
FLOOR_Y = -0.8
EDGE_LIGHTS = np.array([
    [0.5, 0.6, 0.5, 10, 10, 10],      # inside the box of the leaf holding the large slanted triangle
    [-1.0, 0.304, -0.35, 8, 4, 4],    # 0.004 above the small horizontal triangle: its catch-all list
    [2.0, 0.2, 0.5, 0, 3, 4],         # in the plane x = 2 of the side quad, 1.5 beyond its edge: grazing rays
    [0.3, 0.2, 0.1, 12, 3, 4],        # 1.0 above the floor: the floor spans its -y face, that face's four edges
], np.float32)                        # (offsets (+-1, -1, dz), (dx, -1, +-1)) and corners (+-1, -1, +-1)


def _edge_scene():
    """Built for the initial camera (eye about (0, 0.35, 1.97), looking at the origin, 90 degrees): a floor and a back
    wall as receivers; the large slanted triangle of test_gpu_primary_tri.py (its leaf's box holds light 0); a small
    horizontal triangle just under light 1; a quad in the plane x = 2 that holds light 2; over the floor, below light
    3: a triangle straddling the -y and +x faces of its cube map, one triangle present twice, a zero-area triangle,
    and a sheet seen from the floor only from its back."""
    from ptsvgf.scene import Scene, SceneBuilder, env_map, hdr_cache, material, transform

    b = SceneBuilder()
    tri = np.array([[0, 1, 2]], np.int32)
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    back = quad[:, ::-1]

    def add(pos, idx, colour, obj):
        b.add_mesh(np.asarray(pos, np.float32), idx, material(baseColor=colour), transform(), False, obj)

    y = FLOOR_Y
    add([[-4, y, 3], [4, y, 3], [4, y, -2], [-4, y, -2]], quad, (0.7, 0.7, 0.7), 0)            # floor, facing +y
    add([[-4, -4, -2], [4, -4, -2], [4, 4, -2], [-4, 4, -2]], quad, (0.6, 0.7, 0.8), 1)        # wall, facing +z
    add([[-1.5, -0.8, -1.0], [1.0, -0.8, -1.0], [-0.3, 1.0, 4.0]], tri, (0.2, 0.8, 0.3), 2)    # large, slanted
    add([[-1.2, 0.3, -0.5], [-0.8, 0.3, -0.5], [-1.0, 0.3, -0.1]], tri, (0.9, 0.2, 0.2), 3)    # under light 1
    add([[2.0, -0.8, -2.0], [2.0, 0.5, -2.0], [2.0, 0.5, -1.0], [2.0, -0.8, -1.0]], quad, (0.9, 0.8, 0.2), 4)
    # below light 3 (0.3, 0.2, 0.1): across the edge between its -y and +x faces (directions (1, -1, *))
    add([[0.6, -0.3, -0.1], [1.1, -0.1, 0.1], [0.7, -0.5, 0.3]], tri, (0.8, 0.3, 0.8), 5)
    add([[-0.2, -0.4, 0.3], [0.1, -0.4, 0.3], [-0.05, -0.4, 0.6]], np.array([[0, 1, 2], [0, 1, 2]], np.int32),
        (0.2, 0.3, 0.9), 6)                                                                   # twice
    add([[0.2, -0.5, -0.4], [0.5, -0.5, -0.4], [0.35, -0.5, -0.4]], tri, (0.5, 0.5, 0.5), 7)  # zero area
    add([[-0.6, -0.5, -0.6], [-0.2, -0.5, -0.6], [-0.2, -0.5, -0.2], [-0.6, -0.5, -0.2]], back, (0.3, 0.9, 0.9), 8)
    b.build(8)
    tri_enc, node, raster = b.encode()
    hdr = env_map(128, 64)
    return Scene("point_bins_edges", tri_enc, node, raster, EDGE_LIGHTS.copy(), hdr, hdr_cache(hdr), b.counts())


def test_edge_scene(gpu):
    scene = _edge_scene()
    # the construction holds what it says
    leaves = scene.node_enc[1:][scene.node_enc[1:, 3] > 0]  # (node 0 is the reference's dummy)
    L0 = EDGE_LIGHTS[0, :3]
    assert any(np.all(L0 >= lf[6:9]) and np.all(L0 <= lf[9:12]) for lf in leaves)
    assert abs(EDGE_LIGHTS[1, 1] - 0.3) < 0.01 and EDGE_LIGHTS[2, 0] == 2.0 and EDGE_LIGHTS[3, 1] - FLOOR_Y == 1.0
    moves = [None, (0.5, 0.25), (-1.0, -0.5)]
    for depth in (1, 2):
        want, st0 = _pt(gpu, scene, EW, EH, 0, moves, depth=depth)
        got, st1 = _pt(gpu, scene, EW, EH, 1, moves, depth=depth)
        _same(got, want, f"edges/depth{depth}")
        _check_stats(st1, st0, f"edges/depth{depth}")
        assert st1["shadow_point_binned"] > 0, st1
        # what the build made of the four lights: all usable; light 1's neighbour (and only a triangle that near or
        # through a light) in its catch-all list; the others' lists hold the scene
        per = st1["bins_info"]["per_light"]
        assert [q["off"] for q in per] == [0, 0, 0, 0], per
        assert per[1]["catch_all"] >= 1 and per[3]["catch_all"] == 0, per
        assert all(q["entries"] > q["catch_all"] for q in per), per
        assert [q["pos"] for q in per] == EDGE_LIGHTS[:, :3].tolist(), per


# -------------------------------------------------------------- configurations ---
@pytest.mark.parametrize("nlights", [1, 2, 4])
def test_light_counts(gpu, scene_small, nlights):
    sc = dataclasses.replace(scene_small, lights=scene_small.lights[:nlights].copy())
    want, st0 = _pt(gpu, sc, W, H, 0, MOVES[:2])
    got, st1 = _pt(gpu, sc, W, H, 1, MOVES[:2])
    _same(got, want, f"lights{nlights}")
    _check_stats(st1, st0, f"lights{nlights}", binned_share=0.9)


def test_light_without_usable_bins_is_walked(gpu, scene_small):
    """A non-finite light position: that light gets no bins and its list stays with the shadow walk; the other
    lights' rays are binned."""
    lights = scene_small.lights.copy()
    lights[1, 0] = np.inf
    sc = dataclasses.replace(scene_small, lights=lights)
    want, st0 = _pt(gpu, sc, W, H, 0, MOVES[:2])
    got, st1 = _pt(gpu, sc, W, H, 1, MOVES[:2])
    _same(got, want, "non-finite light")
    _check_stats(st1, st0, "non-finite light")
    per = st1["bins_info"]["per_light"]
    assert [q["off"] for q in per] == [0, 1, 0, 0], per
    assert 0.5 * st1["shadow_point_rays"] < st1["shadow_point_binned"] < st1["shadow_point_rays"], st1
    assert st1["shadow_point_fallback"] > 0.1 * st1["shadow_point_rays"], st1


def test_off_beyond_four_lights_and_beyond_the_buffer(gpu, scene_small):
    """pointLightSize 5 (more than kPointBins) and pointLightSize above the lights in the buffer: the rays walk."""
    five = np.concatenate([scene_small.lights, scene_small.lights[:1] + np.float32(0.1)])
    cases = {"five": (dataclasses.replace(scene_small, lights=five), None),
             "past-buffer": (dataclasses.replace(scene_small, lights=scene_small.lights[:2].copy()), 3)}
    for tag, (sc, nlights) in cases.items():
        want, st0 = _pt(gpu, sc, W, H, 0, MOVES[:2], nlights=nlights)
        got, st1 = _pt(gpu, sc, W, H, 1, MOVES[:2], nlights=nlights)
        _same(got, want, tag)
        _check_stats(st1, st0, tag, active=False)
        assert st1["shadow_point_rays"] > 0, (tag, st1)


def test_frames_in_flight_batched(gpu, walks, scene_small):
    want, _ = walks("scene_small")
    got, st = _pt(gpu, scene_small, W, H, 1, MOVES, frames_in_flight=3, trace_batch=2)
    _same(got, want, "frames in flight")
    assert st["shadow_point_binned"] >= 0.9 * st["shadow_point_rays"] > 0, st


def test_band_rows(gpu, scene_small):
    rows = (21, 70)
    want, _ = _pt(gpu, scene_small, W, H, 0, MOVES, rows=rows, stats=False)
    got, _ = _pt(gpu, scene_small, W, H, 1, MOVES, rows=rows, stats=False)
    _same(got, want, "band", rows)


def test_tile_subsets(gpu, scene_small):
    """tile_stride 2: each subset's pixels, the others untouched."""
    ntx = (W + 15) // 16
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    owner = (ty * ntx + tx) % 2
    for off in (0, 1):
        u = {"tile_stride": 2, "tile_offset": off}
        want, st0 = _pt(gpu, scene_small, W, H, 0, MOVES[:2], uniforms=u)
        got, st1 = _pt(gpu, scene_small, W, H, 1, MOVES[:2], uniforms=u)
        _check_stats(st1, st0, f"subset{off}", binned_share=0.9)
        for fa, fb in zip(got, want):
            for k in PLANES:
                assert np.array_equal(fa[k][owner == off].view(np.uint32), fb[k][owner == off].view(np.uint32)), (off, k)


@pytest.mark.parametrize("uniforms", [{"trace_refill": 0}, {"trace_fork": 1}, {"trace_fork": 0}],
                         ids=["no-refill", "fork", "no-fork"])
def test_launch_branches(gpu, walks, scene_small, uniforms):
    """The one-ray-per-lane branch of the launch, and the shadow walk on the side stream and on the draw's."""
    want, st0 = walks("scene_small")
    got, st1 = _pt(gpu, scene_small, W, H, 1, MOVES, uniforms=uniforms)
    _same(got, want, str(uniforms))
    _check_stats(st1, st0, str(uniforms), binned_share=0.9)


# ---------------------------------------------------------------- invalidation ---
def test_new_lights_between_frames(gpu, scene_small):
    """New light positions bound between two frames of one renderer with frames in flight: the frames after them
    equal a fresh renderer's on the new lights."""
    from ptsvgf import gl
    from ptsvgf.renderer import Renderer

    lights2 = scene_small.lights.copy()
    lights2[:, :3] += np.float32([0.2, 0.15, -0.1])
    sc2 = dataclasses.replace(scene_small, lights=lights2)
    r = Renderer(scene_small, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False,
                 frames_in_flight=2)
    for _ in range(2):
        r.frame()
    old = r.pointLightBuffer
    r.pointLightBuffer = gl.texture_buffer(lights2)
    r._owned.append(r.pointLightBuffer)
    r._owned.remove(old)
    got = []
    for _ in range(2):
        r.frame()
        got.append({k: gpu.readback(r.planes()[k]) for k in PLANES})
    st = r.trace_stats()
    r.close()
    gl.destroy_texture(old)
    assert st["shadow_point_binned"] >= 0.9 * st["shadow_point_rays"] > 0, st
    fresh = Renderer(sc2, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False)
    for p, _ in fresh.pt_slots:
        p.set_uniform_int("point_bins", 0)
    want = []
    for i in range(4):
        fresh.frame()
        if i >= 2:
            want.append({k: gpu.readback(fresh.planes()[k]) for k in PLANES})
    fresh.close()
    _same(got, want, "new lights")


def test_rebuilt_and_rebound_scenes(gpu, scene_small):
    """rebuild_bvh with moved geometry, then with fewer triangles: the bins follow the scene."""
    def scenario(bins):
        def prepare(r):
            r.rebuild_bvh(leaf_n=8, ploc_radius=16)
        out, stats = [], []
        from ptsvgf.renderer import Renderer

        r = Renderer(scene_small, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False,
                     frames_in_flight=2)
        for p, _ in r.pt_slots:
            p.set_uniform_int("point_bins", bins)
        prepare(r)
        r.frame()
        for tri in (_moved(scene_small, 0.05), scene_small.tri_enc[:scene_small.tri_enc.shape[0] // 2]):
            r.rebuild_bvh(tri_enc=tri, leaf_n=8, ploc_radius=16)
            r.frame()
            out.append({k: gpu.readback(r.planes()[k]) for k in PLANES})
            stats.append(r.trace_stats())
        r.close()
        return out, stats

    want, st0 = scenario(0)
    got, st1 = scenario(1)
    _same(got, want, "rebuilt")
    for a, b in zip(st1, st0):
        _check_stats(a, b, "rebuilt", binned_share=0.9)


def test_rebind_scene_of_another_triangle_count(gpu, scene_small, scene_cornell):
    """Other triangle and node textures (another scene, another triangle count) bound to a live renderer's passes
    with frames in flight: a second device scene with its own bins; the old textures are destroyed while the
    renderer goes on, which tears the first scene's bins down."""
    from ptsvgf import gl
    from ptsvgf.renderer import Renderer

    def scenario(bins):
        r = Renderer(scene_small, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False,
                     frames_in_flight=3)
        for p, _ in r.pt_slots:
            p.set_uniform_int("point_bins", bins)
        for _ in range(3):
            r.frame()
        old = (r.trianglesTextureBuffer, r.nodesTextureBuffer)
        r.trianglesTextureBuffer = gl.texture_buffer(scene_cornell.tri_enc)
        r.nodesTextureBuffer = gl.texture_buffer(scene_cornell.node_enc)
        for h in old:
            r._owned.remove(h)
        r._owned += [r.trianglesTextureBuffer, r.nodesTextureBuffer]
        out = []
        for i in range(3):
            r.frame()
            if i == 0:
                for h in old:
                    gl.destroy_texture(h)
            out.append({k: gpu.readback(r.planes()[k]) for k in PLANES})
        st = r.trace_stats()
        info = gl.point_bins_info(r.trianglesTextureBuffer, r.nodesTextureBuffer) if bins else None
        r.close()
        return out, st, info

    assert scene_cornell.ntris != scene_small.ntris
    want, st0, _ = scenario(0)
    got, st1, info = scenario(1)
    _same(got, want, "rebound")
    _check_stats(st1, st0, "rebound", binned_share=0.9)
    assert [q["off"] for q in info["per_light"]] == [0, 0, 0, 0], info


def test_counter_count(gpu):
    from ptsvgf._lib import pt
    from ptsvgf.renderer import Renderer

    assert pt().pt_trace_stats_total() == len(Renderer.STAT_KEYS) + len(Renderer.STAT_KEYS_POINT_BINS) == 16

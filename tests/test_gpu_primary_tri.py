"""Primary rays by tile-binned triangles (primary_raster = 2: kernels_wf_primary.hip pr_tri_setup / wf_primary_tri)
against the per-pixel walk (primary_raster = 0, wf_primary, which test_gpu_parity.py and test_gpu_fullsize.py pin
to the oracle): the same closest hit of the same ray, so the path tracer's planes must be bit-identical over
every pixel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANES = ("color", "emission", "albedo")
MOVES = [None, (1.0, 0.75), (-1.5, -1.0), (20.0, 10.0)]  # test_gpu_raster.py's camera states


def _pt(gl, scene, W, H, raster, moves, cap=0, tree=1, rows=None, stats=True, **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, W, H, mode="fast", aspect_corrected=W != H, run_taa=False, run_output=False,
                 gbuffer_rows=rows, **kw)
    for p, _ in r.pt_slots:
        p.set_uniform_int("primary_raster", raster)
        p.set_uniform_int("raster_pair_cap", cap)
        p.set_uniform_int("closest_tree", tree)
        if rows is not None:
            p.set_rows(*rows)
    out = []
    for mv in moves:
        if mv:
            r.camera.orbit(*mv)
        r.frame()
        out.append({k: gl.readback(r.planes()[k]) for k in PLANES})
    st = r.trace_stats() if stats else None
    r.close()
    return out, st


def _same(a, b, tag, rows=None):
    assert len(a) == len(b)
    for f, (fa, fb) in enumerate(zip(a, b)):
        for k in PLANES:
            x, y = fa[k], fb[k]
            if rows is not None:
                x, y = x[rows[0]:rows[1]], y[rows[0]:rows[1]]
            bad = np.argwhere(np.any(x.view(np.uint32) != y.view(np.uint32), axis=-1))
            assert len(bad) == 0, (tag, f, k, len(bad), bad[:5].tolist())


@pytest.fixture(scope="module")
def walks(gpu, request):
    """The walk's frames (primary_raster 0, MOVES) of a scene fixture at 160 x 96, rendered once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _pt(gpu, request.getfixturevalue(name), 160, 96, 0, MOVES)
        return cache[name]

    return get


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell", "scene_nan"])
def test_triangle_raster_equals_walk(gpu, walks, scene_name, request):
    """Through camera moves; flagged pixels go to wf_primary_coop with the SAH tree on and to wf_primary's fix-up
    without it; with a pair list of 4 entries every pixel takes the overflow path."""
    scene = request.getfixturevalue(scene_name)
    W, H = 160, 96
    want, st0 = walks(scene_name)
    got, st2 = _pt(gpu, scene, W, H, 2, MOVES)
    print(scene_name, "walk", st0, "triangles", st2)
    _same(got, want, scene_name)
    assert st2["primary_rays"] == st0["primary_rays"] == W * H, (st0, st2)
    no_tree, _ = _pt(gpu, scene, W, H, 2, MOVES, tree=0, stats=False)
    _same(no_tree, want, scene_name + "/no-tree")
    over, _ = _pt(gpu, scene, W, H, 2, MOVES, cap=4, stats=False)
    _same(over, want, scene_name + "/overflow")


def test_dense_tiles_bench_scene(gpu, scene_bench):
    """30 k triangles in 60 tiles: many 224-triangle chunks per tile, the large triangles binned by whole blocks."""
    W, H = 160, 96
    want, _ = _pt(gpu, scene_bench, W, H, 0, MOVES[:2], stats=False)
    got, st = _pt(gpu, scene_bench, W, H, 2, MOVES[:2])
    print("bench scene", st)
    _same(got, want, "dense")
    assert st["primary_rays"] == W * H


def test_band_rows(gpu, scene_small):
    """A band of rows (boxes clipped to the band, tiles counted from its first row, a ragged last tile row)."""
    W, H, rows = 160, 96, (21, 70)
    want, _ = _pt(gpu, scene_small, W, H, 0, MOVES, rows=rows, stats=False)
    got, _ = _pt(gpu, scene_small, W, H, 2, MOVES, rows=rows, stats=False)
    _same(got, want, "band", rows)


def test_tile_subsets(gpu, walks, scene_small):
    """tile_stride 2: each subset rasterises its own tiles from bins that cover the band; offsets 0 and 1 of one frame
    compose the full frame."""
    from ptsvgf.renderer import Renderer

    gl = gpu
    W, H = 160, 96
    want = walks("scene_small")[0][0]  # the first frame
    r = Renderer(scene_small, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False)
    pt = r.pass_path_tracing
    pt.set_uniform_int("primary_raster", 2)
    pt.set_uniform_int("tile_stride", 2)
    pt.set_uniform_int("tile_offset", 0)
    r.frame()
    ntx = (W + 15) // 16
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    owner = (ty * ntx + tx) % 2
    got = gl.readback(r.planes()["color"])
    assert np.array_equal(got[owner == 0].view(np.uint32), want["color"][owner == 0].view(np.uint32))
    assert not got[owner != 0].any()  # zero-initialised planes, untouched
    r.camera.frameCounter -= 1        # the same frame again, the other subset
    pt.set_uniform_int("tile_offset", 1)
    r._path_trace()
    r.camera.frameCounter += 1
    _same([{k: gl.readback(r.planes()[k]) for k in PLANES}], [want], "subsets")
    r.close()


def test_frames_in_flight(gpu, walks, scene_small):
    """Four frames in flight, their path tracers drawn in batches of two, give the serial walk's frames."""
    want, _ = walks("scene_small")
    got, _ = _pt(gpu, scene_small, 160, 96, 2, MOVES, stats=False, frames_in_flight=4, trace_batch=2)
    _same(got, want, "frames in flight")


# ------------------------------------------------------------------ edge scene ---
EW, EH = 96, 64
GRAZE_PIXEL = (30, 40)


def _primary_ray(cam, x, y):
    """Eye and direction of pixel (x, y)'s primary ray (wf_common.h primary_dir, aspect-corrected)."""
    from ptsvgf.camera import rigid_inverse

    m = rigid_inverse(cam.cam_view_mat).astype(np.float64)
    px = ((2 * x + 1) / cam.width - 1.0) * (cam.width / cam.height)
    py = (2 * y + 1) / cam.height - 1.0
    d = m[0:3] * px + m[4:7] * py - m[8:11]
    return np.asarray(cam.cam_position, np.float64), d / np.linalg.norm(d)


def _edge_scene():
    """Built for the initial camera (eye about (0, 0.35, 1.97), looking at the origin, 90 degrees):
    a front-facing wall at z = -2; a triangle whose plane passes 4.5e-4 from the eye along GRAZE_PIXEL's ray
    (|N.d| = 2e-4 .. 4.5e-4 over its hits); a large triangle from in front of the camera to behind it, passing under
    the eye, whose box holds the eye; one triangle present twice; a quad beside the wall seen only from its back; a
    back-facing sheet in front of the wall."""
    from ptsvgf.camera import Camera
    from ptsvgf.scene import POINT_LIGHTS, Scene, SceneBuilder, env_map, hdr_cache, material, transform

    S, d0 = _primary_ray(Camera(EW, EH), *GRAZE_PIXEL)
    up = np.array([0.0, 1.0, 0.0])
    n0 = np.cross(d0, up)
    n0 /= np.linalg.norm(n0)               # horizontal, perpendicular to the ray
    N = n0 + 3.0e-4 * d0
    N /= np.linalg.norm(N)
    along = d0 - np.dot(d0, N) * N
    along /= np.linalg.norm(along)         # in the plane, nearly along the ray
    u = np.cross(N, along)                 # in the plane, across the ray (nearly vertical on screen)
    C = S + 1.5 * d0
    graze = np.array([C - 0.5 * along - 0.3 * u, C - 0.5 * along + 0.3 * u, C + 0.6 * along])

    b = SceneBuilder()
    tri = np.array([[0, 1, 2]], np.int32)
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    back = quad[:, ::-1]

    def add(pos, idx, colour, obj):
        b.add_mesh(np.asarray(pos, np.float32), idx, material(baseColor=colour), transform(), False, obj)

    add([[-4, -4, -2], [4, -4, -2], [4, 4, -2], [-4, 4, -2]], quad, (0.7, 0.7, 0.7), 0)       # wall, facing +z
    add(graze, tri, (0.9, 0.2, 0.2), 1)
    add([[-1.5, -0.8, -1.0], [1.0, -0.8, -1.0], [-0.3, 1.0, 4.0]], tri, (0.2, 0.8, 0.3), 2)   # passes under the eye
    add([[0.5, 0.5, -1.0], [1.0, 0.5, -1.0], [0.75, 1.0, -1.0]], np.array([[0, 1, 2], [0, 1, 2]], np.int32),
        (0.2, 0.3, 0.9), 3)                                                                   # twice: exact ties
    add([[4.5, 0.0, -2.0], [5.5, 0.0, -2.0], [5.5, 1.0, -2.0], [4.5, 1.0, -2.0]], back, (0.9, 0.8, 0.2), 4)
    add([[-1.2, 0.6, -1.0], [-0.6, 0.6, -1.0], [-0.6, 1.0, -1.0], [-1.2, 1.0, -1.0]], back, (0.8, 0.3, 0.8), 5)
    b.build(8)
    tri_enc, node, raster = b.encode()
    hdr = env_map(128, 64)
    return Scene("primary_tri_edges", tri_enc, node, raster, POINT_LIGHTS.copy(), hdr, hdr_cache(hdr),
                 b.counts()), graze, (S, N)


def test_edge_scene(gpu):
    from ptsvgf.camera import Camera

    gl = gpu
    scene, graze, (S, N) = _edge_scene()
    # the construction holds what it says: |N.d| of the rays meeting the grazing triangle, the eye in a leaf's box
    nd = [abs(np.dot(N, (v - S) / np.linalg.norm(v - S))) for v in graze]
    assert all(1.0e-5 < v < 1.0e-3 for v in nd), nd
    leaves = scene.node_enc[1:][scene.node_enc[1:, 3] > 0]  # (node 0 is the reference's dummy)
    assert any(np.all(S >= lf[6:9]) and np.all(S <= lf[9:12]) for lf in leaves)
    moves = [None, (0.5, 0.25), (-1.0, -0.5)]  # small steps: every item stays on screen
    want, st0 = _pt(gl, scene, EW, EH, 0, moves)
    got, st2 = _pt(gl, scene, EW, EH, 2, moves)
    print("edge scene: walk", st0, "triangles", st2)
    _same(got, want, "edges")
    assert st2["primary_rays"] == EW * EH
    assert st2["tie_rewalks"] >= 1, st2  # the doubled triangle's pixels went to the walk
    # the grazing triangle is on screen: GRAZE_PIXEL shows it, the pixels left and right of it the wall behind
    gx, gy = GRAZE_PIXEL
    row = want[0]["albedo"][gy]
    assert np.array_equal(row[gx - 3], row[gx + 3]) and not np.array_equal(row[gx], row[gx - 3]), row[gx - 3:gx + 4]
    no_tree, _ = _pt(gl, scene, EW, EH, 2, moves, tree=0, stats=False)
    _same(no_tree, want, "edges/no-tree")

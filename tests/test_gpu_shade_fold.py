"""Paths that end in place (uniform shade_fold = 1: no wf_finalize, no wf_finish between two shades, the shade
specialised on first / last bounce; kernels_wf_shade.hip) against the separate launches (shade_fold = 0), and the
primary rasterisers' compact bound plane (written by the G-buffer draw; uniform bound_plane = 1) against their
two-plane read (bound_plane = 0): the same statements in the same order, so the path tracer's planes must be
bit-identical over every pixel and every frame."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLANES = ("color", "emission", "albedo")
MOVES = [None, (1.0, 0.75), (-1.5, -1.0), (20.0, 10.0)]  # test_gpu_primary_tri.py's camera states
W, H = 160, 96


def _pt(gl, scene, fold, moves=MOVES, depth=2, rows=None, bound=1, accumulate=False, refill=None, each=None,
        uniforms=None, plane=True, **kw):
    """The path tracer's planes of every frame of `moves`; each(renderer, frame's planes) may add to a frame's dict."""
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    cfg = parameter_config()
    cfg.max_tracing_depth = depth
    cfg.accumulate_color = accumulate
    r = Renderer(scene, W, H, cfg, mode="fast", aspect_corrected=True, run_taa=False, run_output=False,
                 gbuffer_rows=rows, **kw)
    r.bound_plane = plane  # the G-buffer draws write the compact bound plane (off by default)
    for p, _ in r.pt_slots:
        p.set_uniform_int("shade_fold", fold)
        p.set_uniform_int("bound_plane", bound)
        if refill is not None:
            p.set_uniform_int("trace_refill", refill)
        for name, v in (uniforms or {}).items():
            p.set_uniform_int(name, v)
        if rows is not None:
            p.set_rows(*rows)
    out = []
    for mv in moves:
        if mv:
            r.camera.orbit(*mv)
        r.frame()
        fr = {k: gl.readback(r.planes()[k]) for k in PLANES}
        if each:
            each(r, fr)
        out.append(fr)
    return r, out


def _frames(gl, scene, fold, **kw):
    r, out = _pt(gl, scene, fold, **kw)
    r.close()
    return out


def _same(a, b, tag, rows=None):
    assert len(a) == len(b)
    for f, (fa, fb) in enumerate(zip(a, b)):
        for k in PLANES:
            x, y = fa[k], fb[k]
            if rows is not None:
                x, y = x[rows[0]:rows[1]], y[rows[0]:rows[1]]
            bad = np.argwhere(np.any(x.view(np.uint32) != y.view(np.uint32), axis=-1))
            assert len(bad) == 0, (tag, f, k, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("depth", [1, 2, 3])
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell", "scene_nan"])
def test_fold_equals_separate_launches(gpu, scene_name, depth, request):
    """Depth 1: the first bounce is the last; depth 3: a folded finish between two list-driven shades."""
    scene = request.getfixturevalue(scene_name)
    want = _frames(gpu, scene, 0, depth=depth)
    got = _frames(gpu, scene, 1, depth=depth)
    _same(got, want, (scene_name, depth))
    assert any(f["color"][..., :3].any() for f in want)  # something was rendered


def test_bench_scene(gpu, scene_bench):
    _same(_frames(gpu, scene_bench, 1, moves=MOVES[:2]), _frames(gpu, scene_bench, 0, moves=MOVES[:2]), "bench")


def test_accumulate(gpu, scene_small):
    """accumulate_color: every end point mixes its pixel with lastFrame's (a still camera: a move restarts the
    frame counter, and the first frame's weight is 1)."""
    mv = [None, None, None]
    want = _frames(gpu, scene_small, 0, moves=mv, accumulate=True)
    got = _frames(gpu, scene_small, 1, moves=mv, accumulate=True)
    _same(got, want, "accumulate")
    plain = _frames(gpu, scene_small, 1, moves=mv[:2])
    assert not np.array_equal(plain[1]["color"], got[1]["color"])  # the mix did happen


def test_band_rows(gpu, scene_small):
    rows = (21, 70)
    _same(_frames(gpu, scene_small, 1, rows=rows), _frames(gpu, scene_small, 0, rows=rows), "band", rows)


def test_tile_subsets(gpu, scene_small):
    """Stride 3, offsets 0 and 2: the subset's pixels equal the full frame's, every other pixel keeps its contents."""
    from ptsvgf.renderer import Renderer

    gl = gpu
    want = _frames(gl, scene_small, 0, moves=MOVES[:1])[0]
    ntx = (W + 15) // 16
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    owner = (ty * ntx + tx) % 3
    for fold in (1, 0):
        r = Renderer(scene_small, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False)
        pt = r.pass_path_tracing
        pt.set_uniform_int("shade_fold", fold)
        pt.set_uniform_int("tile_stride", 3)
        pt.set_uniform_int("tile_offset", 0)
        r.frame()
        got = {k: gl.readback(r.planes()[k]) for k in PLANES}
        for k in PLANES:
            assert np.array_equal(got[k][owner == 0].view(np.uint32), want[k][owner == 0].view(np.uint32)), (fold, k)
            assert not got[k][owner != 0].any(), (fold, k)  # zero-initialised planes, untouched
        r.camera.frameCounter -= 1  # the same frame again, another subset
        pt.set_uniform_int("tile_offset", 2)
        r._path_trace(r.gbuf[0])
        r.camera.frameCounter += 1
        got = {k: gl.readback(r.planes()[k]) for k in PLANES}
        for k in PLANES:
            own = owner != 1
            assert np.array_equal(got[k][own].view(np.uint32), want[k][own].view(np.uint32)), (fold, k)
            assert not got[k][owner == 1].any(), (fold, k)
        r.close()


def test_frames_in_flight_batched(gpu, scene_small):
    kw = dict(frames_in_flight=3, trace_batch=2)
    want = _frames(gpu, scene_small, 0)
    _same(_frames(gpu, scene_small, 0, **kw), want, "K=3 B=2 separate")
    _same(_frames(gpu, scene_small, 1, **kw), want, "K=3 B=2 folded")


def test_trace_fork(gpu, scene_small):
    """One frame at a time the renderer forks the bounce-0 shadow walk to a side stream (trace_fork = 1); folded, the
    join follows that walk directly."""
    r, got = _pt(gpu, scene_small, 1, depth=3)
    assert r.K == 1
    r.close()
    want = _frames(gpu, scene_small, 0, depth=3)
    _same(got, want, "fork")


def test_one_ray_per_lane_kernels(gpu, scene_small):
    _same(_frames(gpu, scene_small, 1, refill=0), _frames(gpu, scene_small, 0, refill=0), "trace_refill=0")
    _same(_frames(gpu, scene_small, 1, refill=0), _frames(gpu, scene_small, 0), "trace_refill=0 vs refill")


# ----------------------------------------------------------------- bound plane ---
def _host_bound(world, nd, eye):
    """raster_bound's statements (kernels_wf_primary.hip) in float32 on the read-back texels."""
    f = np.float32
    e = np.asarray(eye, f)
    with np.errstate(all="ignore"):
        d = world[..., :3] - e
        dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=f)
        b = dist * f(1.001) + f(1.0e-3)
    b = np.where(dist == dist, b, f(np.inf))
    return np.where(nd[..., 3] != f(1.0), b, f(np.inf)).astype(f)


def _ulps(a, b):
    """Distance in units in the last place of two arrays of non-negative float32 (inf included)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_nan"])
def test_bound_plane_values(gpu, scene_name, request):
    gl = gpu
    scene = request.getfixturevalue(scene_name)
    seen = []

    def each(r, fr):
        pl = r.planes()
        plane = gl.readback_aux(pl["world"])
        assert plane is not None, "the G-buffer draw wrote no bound plane"
        world, nd = gl.readback(pl["world"]), gl.readback(pl["normal_depth"])
        want = _host_bound(world, nd, r.camera.cam_position)
        bg = nd[..., 3] == np.float32(1.0)
        assert np.all(np.isposinf(plane[bg])) and not np.any(np.isnan(plane))
        u = _ulps(plane, want)
        print(scene_name, "frame", len(seen), "surface", int((~bg).sum()), "max ulp", int(u.max()),
              "inf", int(np.isposinf(plane).sum()))
        assert u.max() <= 1, (int(u.max()), np.argwhere(u > 1)[:5].tolist())
        assert np.array_equal(np.isposinf(plane), np.isposinf(want))
        seen.append(int((~bg).sum()))

    r, _ = _pt(gl, scene, 1, each=each)
    r.close()
    assert len(seen) == len(MOVES) and all(n > 0 for n in seen), seen
    if scene_name == "scene_small":
        assert all(n < W * H for n in seen), seen  # background pixels too


@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell", "scene_nan"])
def test_bound_plane_equals_two_plane_read(gpu, scene_name, request):
    scene = request.getfixturevalue(scene_name)
    want = _frames(gpu, scene, 1, bound=0)
    _same(_frames(gpu, scene, 1, bound=1), want, scene_name)
    r, none = _pt(gpu, scene, 1, plane=False)  # the default: the G-buffer draws write no plane
    assert gpu.readback_aux(r.planes()["world"]) is None
    r.close()
    _same(none, want, scene_name + "/no plane")
    _same(_frames(gpu, scene, 1, bound=1, rows=(21, 70)), _frames(gpu, scene, 1, bound=0, rows=(21, 70)),
          scene_name + "/band", (21, 70))


def test_bound_plane_primary_counters(gpu, scene_small):
    """The plane holds the float the two-plane read forms (the same statements on the same texels and eye), so the
    primary rasteriser prunes identically. Equal in both modes: the rays, the pixels that found nothing under their
    bound and were retried unbounded (they depend on the bound alone) and the tie re-walks. The visit count is not a
    function of the bound alone: a tile's triangle list is filled by atomics, in an order that differs from run to
    run (bins_scatter: "slot order within a tile is arbitrary"), and how many triangles a pixel skips as beyond its
    best hit so far depends on that order. Measured on MI355X, three runs of one frame per mode: 443 510 / 443 511 /
    443 642 visits with the plane, 443 533 / 443 603 / 443 744 with the two planes: the modes differ by no more than
    two runs of one mode (0.03 %). Without a bound (primary_bound = 0) the frame below takes 597 500 visits against
    490 342. So the visits are held to lie at least 20 times nearer to the two-plane read's than the unbounded
    rasteriser's do: a plane that pruned nothing, or pruned differently, would not."""
    st = {}
    for name, bound, uni in (("plane", 1, {}), ("two planes", 0, {}), ("no bound", 0, {"primary_bound": 0})):
        r, _ = _pt(gpu, scene_small, 1, moves=MOVES[:2], bound=bound, uniforms=uni)
        st[name] = r.trace_stats()
        r.close()
        print(name, st[name])
    a, b, c = st["plane"], st["two planes"], st["no bound"]
    for k in ("primary_rays", "primary_retries", "tie_rewalks"):
        assert a[k] == b[k], (k, st)
    assert a["primary_rays"] == W * H and a["primary_visits"] > 0
    assert c["primary_retries"] == 0 and c["primary_visits"] > b["primary_visits"], st
    for k in ("primary_visits", "primary_slots"):
        assert 20 * abs(a[k] - b[k]) < abs(c[k] - b[k]), (k, st)

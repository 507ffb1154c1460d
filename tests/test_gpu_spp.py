"""Several samples per pixel in one path-tracing draw (int uniform spp = N, Renderer(spp=N): kernels_wavefront.hip
launch_wavefront's sample draw, kernels_spp.hip wf_spp_resolve) against its definition (tests/spp_ref.py, over the CPU
oracle), against N one-sample draws of the GPU itself, and through every switch and draw geometry that must keep the
bits. 160 x 96, the camera states of test_gpu_shade_fold.py and one still frame after them (a move restarts the frame
counter, so only a still frame has F > 0); comparisons on uint32 views."""
import numpy as np
import pytest

import oracle_ref as O
from spp_ref import fold_mean, spp_ref
from test_gpu_shade_fold import MOVES, PLANES, H, W, _same

pytestmark = pytest.mark.gpu

STILL = MOVES + [None]  # F = 0, 0, 0, 0, 1
SENTINEL = np.float32(-7.25)
_oracles = {}


def _oracle(name, scene):
    if name not in _oracles:
        _oracles[name] = O.OracleScene(scene)
    return _oracles[name]


def _renderer(scene, depth=2, rows=None, accumulate=False, uniforms=None, prepare=None, mode="fast", **kw):
    from ptsvgf.camera import parameter_config
    from ptsvgf.renderer import Renderer

    cfg = parameter_config()
    cfg.max_tracing_depth = depth
    cfg.accumulate_color = accumulate
    r = Renderer(scene, W, H, cfg, mode=mode, aspect_corrected=True, run_taa=False, run_output=False,
                 gbuffer_rows=rows, **kw)
    if prepare:
        prepare(r)
    for p, _ in r.pt_slots:
        for name, v in (uniforms or {}).items():
            p.set_uniform_int(name, v)
        if rows is not None:
            p.set_rows(*rows)
    return r


def _run(gl, scene, moves=STILL, counter=None, keep=False, extra=(), **kw):
    """The path tracer's planes of every frame of `moves`, with the frame's counter F, eye and cameraRotate;
    counter(F) replaces the frameCounter uniform of the frame whose own counter is F."""
    r = _renderer(scene, **kw)
    out = []
    for mv in moves:
        if mv:
            r.camera.orbit(*mv)
        r.camera.update()  # (a move restarts the counter here)
        F = int(r.camera.frameCounter)
        if counter is not None:
            r.camera.frameCounter = counter(F)
        r.frame()
        if counter is not None:
            r.camera.frameCounter = F + 1
        pl = r.planes()
        fr = {k: gl.readback(pl[k]) for k in PLANES + tuple(extra)}
        fr.update(F=F, eye=np.array(r.camera.cam_position, np.float32), rot=np.array(r.cameraRotate, np.float32))
        out.append(fr)
    if keep:
        return r, out
    r.close()
    return out


def _want(name, scene, frames, n, depth=2, rows=None):
    """The definition's planes of the frames a run recorded."""
    from ptsvgf.camera import parameter_config

    cfg = parameter_config()
    os_ = _oracle(name, scene)
    out = []
    for fr in frames:
        c, e, a = spp_ref(os_, W, H, fr["F"], n, fr["eye"], fr["rot"], cfg.clamp_threshold, depth, True, rows=rows,
                          use_normal_map=cfg.use_normal_texture)
        out.append(dict(color=c, emission=e, albedo=a))
    return out


@pytest.fixture(scope="module")
def base(gpu, request):
    """Frames at the renderer's defaults per (scene fixture, spp, depth), rendered once per module."""
    cache = {}

    def get(name, n, depth=2):
        if (name, n, depth) not in cache:
            cache[name, n, depth] = _run(gpu, request.getfixturevalue(name), spp=n, depth=depth)
        return cache[name, n, depth]

    return get


# ------------------------------------------------------------ 1. the definition ---
@pytest.mark.parametrize("n,depth", [(2, 2), (3, 2), (8, 2), (2, 1), (2, 3)])
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell", "scene_nan"])
def test_equals_the_definition(gpu, base, scene_name, n, depth, request):
    """(8, 2) on scene_small is the largest batch; depth 1: the first bounce is the last; depth 3: a folded finish
    between two list-driven shades."""
    scene = request.getfixturevalue(scene_name)
    got = base(scene_name, n, depth)
    assert [f["F"] for f in got] == [0, 0, 0, 0, 1]
    _same(got, _want(scene_name, scene, got, n, depth), (scene_name, n, depth))
    assert all(f["color"][..., :3].any() for f in got)


def test_nan_normal_paths_at_one_sample(gpu, base, scene_nan):
    """One sample per pixel on scene_nan over the same frames: the definition's sample is the reference's main(),
    which ends a path on NdotL <= 0 (:1016, :1098), so a NaN NdotL (NaN vertex normals) goes on and the pixel ends at
    0. The bounce-0 / bounce-1 shade used to test NdotL > 0 and kept what such a path had gathered: 6 and 3 pixels of
    the last two frames differed from the oracle (and from the megakernel, which has the reference's test)."""
    got = base("scene_nan", 1)
    _same(got, _want("scene_nan", scene_nan, got, 1), "scene_nan spp=1")
    mega = _run(gpu, scene_nan, uniforms={"pt_kernel": 1})
    _same(got, mega, "wavefront / megakernel")


# ------------------------------------------------------------ 2. the GPU itself ---
def test_four_samples_equal_four_draws(gpu, base, scene_small):
    """N = 4 is the float32 fold of four one-sample renders with the frameCounter uniform 4F + s: no oracle."""
    got = base("scene_small", 4)
    singles = [_run(gpu, scene_small, spp=1, counter=lambda F, s=s: 4 * F + s) for s in range(4)]
    for f, fr in enumerate(got):
        assert all(x[f]["F"] == fr["F"] for x in singles)
        want = dict(color=fold_mean([x[f]["color"] for x in singles]), emission=singles[0][f]["emission"],
                    albedo=singles[0][f]["albedo"])
        _same([fr], [want], ("fold of four draws", f))
        for x in singles[1:]:  # the shared primary hit: every one-sample draw wrote these bits too
            _same([dict(fr, color=x[f]["color"])], [x[f]], ("first-hit planes", f))
    assert not np.array_equal(got[0]["color"], singles[0][0]["color"])


def test_explicit_one_equals_never_set(gpu, base, scene_small):
    never = _run(gpu, scene_small)
    _same(base("scene_small", 1), never, "spp=1")
    _same(_run(gpu, scene_small, uniforms={"spp": 1}), never, "uniform spp=1")


# ---------------------------------------------------- 3. the primary hit traced once ---
def test_primary_traced_once(gpu, scene_small):
    def stats(n, counter=None):
        r = _renderer(scene_small, spp=n)
        r.frame()  # F = 0
        if counter is not None:
            r.camera.frameCounter = counter(1)
        st = r.trace_stats()  # the frame with F = 1
        r.close()
        return st

    four = stats(4)
    singles = [stats(1, lambda F, s=s: 4 * F + s) for s in range(4)]
    print("spp 4", four, "singles", singles)
    assert four["primary_rays"] == singles[0]["primary_rays"] == W * H
    assert four["bounce_rays"] == sum(s["bounce_rays"] for s in singles) > 0
    assert four["shadow_rays"] == sum(s["shadow_rays"] for s in singles) > 0


# ------------------------------------------------------ 4. switches keep the bits ---
SWITCHES = {
    "shade_fold=0": dict(uniforms={"shade_fold": 0}),
    "shade_fold=1": dict(uniforms={"shade_fold": 1}),
    "trace_refill=0": dict(uniforms={"trace_refill": 0}),
    "trace_refill=0, unfolded": dict(uniforms={"trace_refill": 0, "shade_fold": 0}),
    "trace_fork=1, depth 3": dict(uniforms={"trace_fork": 1}, depth=3),
    "trace_fork=0": dict(uniforms={"trace_fork": 0}),
    "point_bins=1": dict(uniforms={"point_bins": 1}),
    "point_bins=0": dict(uniforms={"point_bins": 0}),
    "primary_raster=0": dict(uniforms={"primary_raster": 0}),
    "primary_raster=1": dict(uniforms={"primary_raster": 1}),
    "primary_raster=2": dict(uniforms={"primary_raster": 2}),
    "closest_tree=0": dict(uniforms={"closest_tree": 0}),
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_switches_keep_the_bits(gpu, base, scene_small, switch):
    """N = 2 on test_gpu_point_bins.py's main scene and lights (scene_small's four)."""
    kw = dict(SWITCHES[switch])
    depth = kw.get("depth", 2)
    got = _run(gpu, scene_small, spp=2, **kw)
    _same(got, base("scene_small", 2, depth), switch)


@pytest.mark.parametrize("wide", [1, 0])
def test_rebuilt_scene(gpu, scene_small, wide):
    """A tree rebuild_bvh built on the device, walked through its 4-wide tree (lbvh_wide = 1) and without it: the
    definition evaluated on the rebuilt buffers."""
    import dataclasses

    def prepare(r):
        r.rebuild_bvh(leaf_n=3, ploc_radius=32)
        r.set_lbvh_wide(bool(wide))

    r, got = _run(gpu, scene_small, spp=2, moves=STILL[:2] + [None], prepare=prepare, keep=True)
    tri = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    r.close()
    rebuilt = dataclasses.replace(scene_small, tri_enc=tri, node_enc=nodes)
    _same(got, _want(("rebuilt", wide), rebuilt, got, 2), ("rebuilt", wide))


# ------------------------------------------------------ 5. geometry of the draw ---
def test_band_rows(gpu, base, scene_small):
    rows = (21, 70)
    got = _run(gpu, scene_small, spp=2, rows=rows)
    _same(got, base("scene_small", 2), "band", rows)
    for fr in got:
        for k in PLANES:  # zero-initialised planes, untouched outside the band
            assert not fr[k][:rows[0]].any() and not fr[k][rows[1]:].any(), k


def test_tile_subsets(gpu, base, scene_small):
    """Stride 3, offsets 0 and 2: the subset's pixels equal the full frame's, every other pixel keeps the sentinel."""
    gl = gpu
    want = base("scene_small", 2)[0]
    ntx = (W + 15) // 16
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    owner = (ty * ntx + tx) % 3
    r = _renderer(scene_small, spp=2)
    pt = r.pass_path_tracing
    pt.set_uniform_int("tile_stride", 3)
    pt.set_uniform_int("tile_offset", 0)
    fill = np.full((H, W, 4), SENTINEL, np.float32)
    for t in r.pt_slots[0][1]:  # colour, emission, albedo of the only slot
        gl.upload_rgba(t, fill)
    r.frame()
    got = {k: gl.readback(r.planes()[k]) for k in PLANES}
    for k in PLANES:
        assert np.array_equal(got[k][owner == 0].view(np.uint32), want[k][owner == 0].view(np.uint32)), k
        assert np.all(got[k][owner != 0] == SENTINEL), k
    r.camera.frameCounter -= 1  # the same frame again, another subset
    pt.set_uniform_int("tile_offset", 2)
    r._path_trace(r.gbuf[0])
    r.camera.frameCounter += 1
    got = {k: gl.readback(r.planes()[k]) for k in PLANES}
    for k in PLANES:
        own = owner != 1
        assert np.array_equal(got[k][own].view(np.uint32), want[k][own].view(np.uint32)), k
        assert np.all(got[k][owner == 1] == SENTINEL), k
    r.close()


def test_frames_in_flight(gpu, base, scene_small):
    """K = 4 (the library's point_bins default and no fork, as the renderer sets them then), also with trace_batch
    asked for: frames are not batched while spp > 1."""
    want = base("scene_small", 2)
    _same(_run(gpu, scene_small, spp=2, frames_in_flight=4), want, "K=4")
    r, got = _run(gpu, scene_small, spp=2, frames_in_flight=4, trace_batch=2, keep=True)
    assert not r._batching()
    r.spp = 1
    assert r._batching() and r.spp == 1
    r.close()
    _same(got, want, "K=4 B=2")


# ------------------------------------------------------------------ 6. accumulate ---
def test_accumulate(gpu, scene_small):
    """Three still frames at N = 2: the definition chained through lastFrame (zero before the first frame)."""
    from ptsvgf.camera import parameter_config

    got = _run(gpu, scene_small, spp=2, moves=[None, None, None], accumulate=True)
    cfg = parameter_config()
    os_ = _oracle("scene_small", scene_small)
    last = np.zeros((H, W, 4), np.float32)
    for f, fr in enumerate(got):
        assert fr["F"] == f
        c, e, a = spp_ref(os_, W, H, f, 2, fr["eye"], fr["rot"], cfg.clamp_threshold, 2, True, accumulate=True,
                          last_frame=last)
        _same([fr], [dict(color=c, emission=e, albedo=a)], ("accumulate", f))
        last = c
    plain = _run(gpu, scene_small, spp=2, moves=[None, None])
    assert not np.array_equal(plain[1]["color"], got[1]["color"])  # the mix did happen


# ----------------------------------------------------------------------- 7. chain ---
def test_svgf_chain(gpu, scene_small):
    out = {}
    for n in (1, 2):
        r, frames = _run(gpu, scene_small, spp=n, moves=[None, None, None], keep=True)
        pl = {k: gpu.readback(v) for k, v in r.planes().items()}
        r.close()
        assert np.isfinite(pl["modulate"]).all()
        # the chain read the resolved colour: the path tracer's colour plane is the one the definition gives
        assert np.array_equal(pl["color"].view(np.uint32), frames[-1]["color"].view(np.uint32))
        out[n] = (pl, frames)
    _same([out[2][1][-1]], _want("scene_small", scene_small, out[2][1][-1:], 2), "chain colour")
    assert not np.array_equal(out[1][0]["modulate"], out[2][0]["modulate"])
    assert not np.array_equal(out[1][0]["reproj_illum"], out[2][0]["reproj_illum"])


def test_reference_driver(gpu, base, scene_small):
    got = _run(gpu, scene_small, spp=2, mode="reference", moves=STILL[:2] + [None])
    _same(got[:2], base("scene_small", 2)[:2], "reference driver")
    _same(got, _want("scene_small", scene_small, got, 2), "reference driver / definition")


# ---------------------------------------------------------------------- 8. errors ---
def _filled(gl, r):
    fill = np.full((H, W, 4), SENTINEL, np.float32)
    for k in PLANES:
        gl.upload_rgba(r.planes()[k], fill)


def _untouched(gl, r, tag):
    gl.sync()
    for k in PLANES:
        assert np.all(gl.readback(r.planes()[k]) == SENTINEL), (tag, k)


@pytest.mark.parametrize("case", ["spp=0", "spp=-1", "spp=9", "megakernel", "batch"])
def test_errors(gpu, base, scene_small, case):
    """Each refused draw returns PT_ERR_ARG and leaves the sentinel in every plane; the same pass then draws."""
    import torch

    from ptsvgf._lib import PtError

    gl = gpu
    r = _renderer(scene_small, frames_in_flight=2 if case == "batch" else 1)
    for _ in r.pt_slots:
        r.frame()  # binds every uniform and sampler of the slots' passes; slot 0 holds the frame F = 0
    torch.cuda.synchronize()
    fill = np.full((H, W, 4), SENTINEL, np.float32)
    for _, outs in r.pt_slots:
        for t in outs:
            gl.upload_rgba(t, fill)
    pt = r.pt_slots[0][0]
    if case.startswith("spp="):
        pt.set_uniform_int("spp", int(case[4:]))
    elif case == "megakernel":
        pt.set_uniform_int("spp", 2)
        pt.set_uniform_int("pt_kernel", 1)
    else:
        r.pt_slots[1][0].set_uniform_int("spp", 2)
    with pytest.raises(PtError) as e:
        if case == "batch":
            gl.draw_batch([p for p, _ in r.pt_slots])
        else:
            pt.draw()
    assert e.value.code == -6, e.value  # PT_ERR_ARG
    torch.cuda.synchronize()
    for _, outs in r.pt_slots:
        for t in outs:
            assert np.all(gl.readback(t) == SENTINEL), case
    pt.set_uniform_int("pt_kernel", 0)
    pt.set_uniform_int("spp", 2)
    pt.draw()
    torch.cuda.synchronize()
    got = {k: gl.readback(t) for k, t in zip(PLANES, r.pt_slots[0][1])}
    r.close()
    _same([got], base("scene_small", 2)[:1], case + ": valid draw after")


def test_python_range(gpu, scene_small):
    for n in (0, -1, 9, 1.5):
        with pytest.raises(ValueError):
            _renderer(scene_small, spp=n)
    r = _renderer(scene_small)
    with pytest.raises(ValueError):
        r.spp = 9
    assert r.spp == 1
    r.close()

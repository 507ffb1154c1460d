"""The material zoo (tests/material_zoo.py) on the GPU: twelve teapots at the corners of the Disney BRDF's parameter
space (black base colour, metallic 1, roughness 0 and 1, subsurface 1, full tints, clearcoatGloss 0 and 1, a black
emitter) through brdf_eval / brdf_pdf / sample_brdf (pt_shading.h), the shade stages (kernels_wf_shade.hip,
kernels_pt.hip), the device-side material decode (kernels_bvh.hip, kernels_materials.hip) and, with albedo 0 and
emission on surface pixels, the SVGF chain (kernels_svgf.hip, kernels_spp.hip, kernels_atrous.hip) against the CPU
oracle, which tests/test_material_zoo.py ties to the float64 restatement of path_tracing.frag:620-669, :753-784 and
:948-968 on this very scene. 96 x 64, aspect-corrected ray; every path-tracer comparison is bitwise."""
import dataclasses

import numpy as np
import pytest

import material_zoo as Z
import oracle_ref as O
from adaptive_ref import adaptive_ref, derive_counts
from materials_ref import materials_ref
from spp_ref import spp_ref
from test_gpu_deep import _check_bits
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

W, H = 96, 64
PT = ("color", "emission", "albedo")
GBUF = ("normal_depth", "velocity", "fwidth", "world")
SVGF = ("reproj_illum", "reproj_moments", "variance", "atrous", "history_illum", "modulate")
ORBIT = (2.0, 0.5)
SEQUENCE = (None, None, None, ORBIT, None, None)  # 3 standing frames, one orbit step, 2 more
f32 = np.float32


@pytest.fixture(scope="module")
def zoo():
    return Z.zoo_edges()


def _cfg(depth=2):
    from ptsvgf.camera import parameter_config

    cfg = parameter_config()
    cfg.max_tracing_depth = depth
    return cfg


@pytest.fixture(scope="module")
def oracle_seq(zoo):
    """The oracle frame loop's frames over SEQUENCE (depth 2), computed once and left as they are."""
    ref = O.OracleFrameLoop(zoo, W, H, run_taa=False)
    out = []
    for mv in SEQUENCE:
        if mv:
            ref.camera.orbit(*mv)
        out.append(ref.frame())
    return out


@pytest.fixture(scope="module")
def oracle_pt(zoo):
    """The oracle path tracer's planes of standing frames 0 .. n-1 per depth."""
    osc = O.OracleScene(zoo)
    eye, rot = Z.camera(W, H)
    cache = {}

    def get(depth, n):
        have = cache.setdefault(depth, [])
        cfg = _cfg(depth)
        while len(have) < n:
            have.append(dict(zip(PT, osc.path_trace(W, H, len(have), eye, rot, cfg.clamp_threshold, depth, True))))
        return have[:n]

    return get


def _renderer(scene, uniforms=None, depth=2, mode="fast", **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, W, H, _cfg(depth), mode=mode, aspect_corrected=True, run_taa=False, run_output=False, **kw)
    for p, _ in r.pt_slots:
        for name, v in (uniforms or {}).items():
            p.set_uniform_int(name, v)
    return r


def _own(scene, tri=None):
    """A scene object of the test's own (set_materials keeps scene.tri_enc in step: the fixture stays as it is)."""
    return dataclasses.replace(scene, tri_enc=(scene.tri_enc if tri is None else tri).copy())


def _pt(gl, r):
    pl = r.planes()
    return {k: gl.readback(pl[k]) for k in PT}


def _standing(gl, r, n):
    out = []
    for _ in range(n):
        r.frame()
        out.append(_pt(gl, r))
    return out


def _check_frames(got, want, tag):
    assert len(got) == len(want)
    for f, (a, b) in enumerate(zip(got, want)):
        _check_bits(a, {k: b[k] for k in PT}, (tag, f))


# ----------------------------------------------------------------------- 1. the frame loop ---
@pytest.mark.parametrize("mode", ["reference", "fast"])
def test_frames_match_oracle(gpu, zoo, oracle_seq, mode):
    """Every pass output over SEQUENCE against the oracle frame loop, test_gpu_parity.test_frames_match_oracle's bars
    (its _cmp: the finite / non-finite agreement, G-buffer within 1e-5, SVGF planes within 1e-3 relative, exact
    a-trous), the path tracer's planes bit for bit."""
    r = _renderer(zoo, mode=mode, atrous_exact=True)
    for f, mv in enumerate(SEQUENCE):
        if mv:
            r.camera.orbit(*mv)
        r.frame()
        want = oracle_seq[f]
        got = {k: gpu.readback(v) for k, v in r.planes().items()}
        _check_bits({k: got[k] for k in PT}, {k: want[k] for k in PT}, (mode, f))
        for key in GBUF:
            _cmp(f"{mode}/f{f}/{key}", got[key], want[key], tol=1e-5)
        for key in SVGF:
            _cmp(f"{mode}/f{f}/{key}", got[key], want[key], rel=True)
    r.close()


@pytest.mark.parametrize("mode", ["reference", "fast"])
def test_production_atrous_within_tolerance(gpu, zoo, oracle_seq, mode):
    """The production a-trous (atrous_exact=False) over SEQUENCE in both drivers: test_fast_atrous_within_tolerance's
    bar on its planes, at every frame. In the fast driver the last iteration's epilogue writes `modulate` itself
    (fuse_modulate), so this is where the kernel production draws with meets albedo-0 and emitting surface pixels, the
    static-background skip and the history reprojected over the orbit step."""
    r = _renderer(zoo, mode=mode, atrous_exact=False)
    for f, mv in enumerate(SEQUENCE):
        if mv:
            r.camera.orbit(*mv)
        r.frame()
        got = {k: gpu.readback(r.planes()[k]) for k in ("atrous", "modulate")}
        for key in got:
            _cmp(f"{mode}/f{f}/{key}", got[key], oracle_seq[f][key], rel=True)
    r.close()


# ------------------------------------------------------------------- 2. kernels and depths ---
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("kernel", [0, 1])
def test_both_kernels_and_depths(gpu, zoo, oracle_pt, kernel, depth):
    """The wavefront stages (pt_kernel 0) and the megakernel (1) at depth 1 .. 4 over frameCounter 0 .. 2; depth 3 and 4
    reach Sobol dimensions 5 and 7 (path_tracing.frag:463-472)."""
    r = _renderer(zoo, {"pt_kernel": kernel}, depth=depth)
    _check_frames(_standing(gpu, r, 3), oracle_pt(depth, 3), (kernel, depth))
    r.close()


# ---------------------------------------------------------------------------- 3. switches ---
SWITCHES = {
    "point_bins=0": ({"point_bins": 0}, {}),
    "shade_fold=0": ({"shade_fold": 0}, {}),
    "primary_cache=0": ({"primary_cache": 0}, {}),
    "point_cache=0": ({"point_cache": 0}, {}),
    "reference trees": ({"closest_tree": 0, "shadow_tree": 0}, {}),
    "defaults, 3 in flight": ({}, {"frames_in_flight": 3}),
    "defaults": ({}, {}),
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_switches_match_oracle(gpu, zoo, oracle_pt, switch):
    """One switch at a time over 4 standing frames (the static-view caches engage from the second frame of a slot on;
    with three slots, frames 0 .. 5)."""
    uniforms, kw = SWITCHES[switch]
    n = 6 if kw else 4
    r = _renderer(zoo, uniforms, **kw)
    _check_frames(_standing(gpu, r, n), oracle_pt(2, n), switch)
    r.close()


# ------------------------------------------------------------------- 4. samples per pixel ---
N = 3
MOVES_SPP = (None, None, ORBIT, None)


def _frame(gl, r, move, keys):
    if move:
        r.camera.orbit(*move)
    r.camera.update()  # (a move restarts the counter here)
    F = int(r.camera.frameCounter)
    r.frame()
    pl = r.planes()
    fr = {k: gl.readback(pl[k]) for k in keys}
    fr.update(F=F, eye=np.array(r.camera.cam_position, f32), rot=np.array(r.cameraRotate, f32))
    return fr


@pytest.fixture(scope="module")
def samples_of(zoo):
    """spp_ref's per-sample colours, emission and albedo of a recorded frame, cached per (camera, F)."""
    osc = O.OracleScene(zoo)
    cache = {}

    def get(fr):
        key = (fr["eye"].tobytes(), fr["rot"].tobytes(), fr["F"])
        if key not in cache:
            cfg = _cfg()
            samples = []
            c, e, a = spp_ref(osc, W, H, fr["F"], N, fr["eye"], fr["rot"], cfg.clamp_threshold, 2, True,
                              use_normal_map=cfg.use_normal_texture, samples=samples)
            cache[key] = (samples, c, e, a)
        return cache[key]

    return get


def test_three_samples_equal_the_definition(gpu, zoo, samples_of):
    """Renderer(spp=3) against tests/spp_ref.py over the oracle: bit for bit, standing frames and a camera step."""
    r = _renderer(zoo, spp=N)
    for f, mv in enumerate(MOVES_SPP):
        fr = _frame(gpu, r, mv, PT)
        _, c, e, a = samples_of(fr)
        _check_bits({k: fr[k] for k in PT}, dict(color=c, emission=e, albedo=a), ("spp", f))
    r.close()


def test_sample_moments_equal_the_definition(gpu, zoo, samples_of, tmp_path_factory):
    """Renderer(spp=3, sample_moments=True): the resolve's plane, the reproject and the variance pass bit for bit
    against tests/sample_moments_ref.cpp on the inputs the GPU had, the passes behind them within the oracle's
    tolerance, called as test_gpu_sample_moments.py's _renderer_loop calls them. spp_demod_lum and the reprojection
    demodulate by max(albedo, 0.001) on the two black teapots here."""
    import sample_moments_ref as SM
    from adaptive_ref import fold_counts
    from test_gpu_sample_moments import KEYS, Chain, _eq

    ref = SM.load(tmp_path_factory.mktemp("sample_moments_ref"))
    r = _renderer(zoo, spp=N, sample_moments=True, atrous_exact=True)
    chain = Chain(ref, r.cfg)
    full = np.full((H, W), 255, np.uint8)
    for f, mv in enumerate(MOVES_SPP):
        fr = _frame(gpu, r, mv, KEYS)
        samples, _, e, a = samples_of(fr)
        _eq(fr["color"], fold_counts(samples, full), ("sm", f, "color"))
        sm = ref.resolve_plane(samples, e, a, None)
        _eq(r.sample_moments(), sm, ("sm", f, "moments"))
        chain.check(fr, sm, ("sm", f))
    r.close()


def test_adaptive_counts_equal_the_definition(gpu, zoo, samples_of):
    """Renderer(spp=3, adaptive=1.0) over standing frames: the counts are the definition's derive of the previous
    statistics, colour and statistics tests/adaptive_ref.py's over the oracle's samples, bit for bit."""
    tau = 1.0
    r = _renderer(zoo, spp=N, adaptive=tau)
    prev = None
    for f in range(4):
        fr = _frame(gpu, r, None, PT + ("normal_depth", "velocity"))
        assert fr["F"] == f
        counts, stats = r.sample_counts(), r.sample_stats()
        if prev is None:
            assert np.all(counts == 255)
        else:
            want = derive_counts(prev, fr["velocity"], fr["normal_depth"], 1.0, tau, N)
            bad = np.argwhere(counts != want)
            assert len(bad) == 0, ("counts", f, len(bad), bad[:5].tolist())
        samples, _, e, a = samples_of(fr)
        color, st = adaptive_ref(samples, counts)
        _check_bits({k: fr[k] for k in PT}, dict(color=color, emission=e, albedo=a), ("adaptive", f))
        assert np.array_equal(stats.view(np.uint32), st.view(np.uint32)), ("stats", f)
        prev = stats
    r.close()


# --------------------------------------------------------------------- 5. the GPU-built tree ---
@pytest.mark.parametrize("lbvh_wide", [1, 0])
def test_render_over_gpu_built_tree_matches_oracle(gpu, zoo, lbvh_wide):
    """rebuild_bvh(leaf_n=8, ploc_radius=16) on the zoo (the shading records are decoded on the device), then frames
    against the oracle on the same buffers, as test_gpu_bvh.test_render_over_gpu_lbvh_matches_oracle compares them;
    through the 4-wide tree and the binary one."""
    from test_gpu_bvh import L

    r = _renderer(zoo, frames_in_flight=2)
    r.rebuild_bvh(leaf_n=8, ploc_radius=16)
    r.set_lbvh_wide(bool(lbvh_wide))
    want_tri, want_nodes = L.lbvh(zoo.tri_enc, 8, 16)
    got_tri = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    got_nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    assert np.array_equal(got_tri.view(np.uint32), want_tri.view(np.uint32))
    assert np.array_equal(got_nodes.view(np.uint32), want_nodes.view(np.uint32))
    osc = O.OracleScene(dataclasses.replace(zoo, tri_enc=want_tri, node_enc=want_nodes))
    eye, rot = Z.camera(W, H)
    want = [dict(zip(PT, osc.path_trace(W, H, f, eye, rot, aspect_corrected=True))) for f in range(3)]
    _check_frames(_standing(gpu, r, 3), want, ("lbvh", lbvh_wide))
    r.close()


# ------------------------------------------------------------------------ 6. material edits ---
def test_material_edits_match_oracle(gpu, zoo):
    """Three frames in flight on a standing view; every teapot starts as `mid`, objects 1 .. 6 take their zoo materials
    after 2 frames, objects 7 .. 12 one frame later; every frame is the oracle's on tests/materials_ref.py's buffer for
    the materials in force, bit for bit (not a fresh renderer's)."""
    mats = {k: Z.zoo_material(k) for k in Z.OBJECTS}
    t0 = materials_ref(zoo.tri_enc, 1, np.tile(mats[12], (12, 1)))
    t1 = materials_ref(t0, 1, np.stack([mats[k] for k in range(1, 7)]))
    t2 = materials_ref(t1, 7, np.stack([mats[k] for k in range(7, 13)]))
    assert np.array_equal(t2.view(np.uint32), zoo.tri_enc.view(np.uint32))  # all edits applied: the zoo itself
    force = [t0, t0, t1, t2, t2, t2]
    oracles = {id(t): O.OracleScene(dataclasses.replace(zoo, tri_enc=t)) for t in (t0, t1, t2)}
    eye, rot = Z.camera(W, H)
    r = _renderer(_own(zoo, t0), frames_in_flight=3)
    for f, tri in enumerate(force):
        if f == 2:
            r.set_materials({k: mats[k] for k in range(1, 7)})
        if f == 3:
            r.set_materials({k: mats[k] for k in range(7, 13)})
        r.frame()
        want = dict(zip(PT, oracles[id(tri)].path_trace(W, H, f, eye, rot, aspect_corrected=True)))
        _check_bits(_pt(gpu, r), want, ("edit", f))
    texels = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    assert np.array_equal(texels.view(np.uint32), zoo.tri_enc.view(np.uint32))
    r.close()


# ---------------------------------------------------------------------- 7. dead parameters ---
@pytest.mark.parametrize("how", ["host bind", "set_materials"])
def test_dead_parameters_change_no_bit(gpu, zoo, oracle_pt, how):
    """anisotropic, IOR and transmission set on every object (tests/test_material_zoo.py: the oracle ignores them):
    the plain zoo's bits, from a scene bound with them and from an edit after the first frame."""
    dead = {k: Z.DEAD for k in range(13)}
    want = oracle_pt(2, 3)
    if how == "host bind":
        scene = Z.zoo_edges(override=dead)
        assert not np.array_equal(scene.tri_enc.view(np.uint32), zoo.tri_enc.view(np.uint32))
        r = _renderer(scene)
        got = _standing(gpu, r, 3)
    else:
        r = _renderer(_own(zoo))
        got = _standing(gpu, r, 1)
        r.set_materials({k: Z.zoo_material(k, override=dead) for k in range(13)})
        got += _standing(gpu, r, 2)
        assert not np.array_equal(r.scene.tri_enc.view(np.uint32), zoo.tri_enc.view(np.uint32))
    _check_frames(got, want, how)
    r.close()

"""SVGF from sample moments on the GPU (pt_pass_set_sample_moments, sampler gSampleMoments, Renderer(spp=N,
sample_moments=True); kernels_spp.hip wf_spp_resolve_adaptive<.., MOMENTS>, kernels_svgf.hip reproject_kernel<SM>
and variance_kernel<SM>) against its definition: tests/sample_moments_ref.cpp over spp_ref.py's per-sample colours of
the CPU oracle and adaptive_ref.py's counts. 40 x 24 frames (partial 16 x 16 tiles; the variance pass's 3-texel apron
crosses block edges), the scenes of test_gpu_spp.py; every comparison of the resolve, the reproject and the variance
pass is bitwise (uint32 views). The reproject and variance passes are checked frame by frame on the inputs the GPU
itself had (its G-buffer, its history), so each frame's verdict stands alone; the a-trous and modulate passes behind
them are held to the oracle within test_gpu_parity.py's tolerance."""
import numpy as np
import pytest

import oracle_ref as O
import sample_moments_ref as SM
from adaptive_ref import derive_counts, effective, fold_counts, stats_counts
from spp_ref import mix_last, spp_ref

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 40, 24
SENTINEL = f32(-7.25)
PT = ("color", "emission", "albedo")
CHAIN = ("reproj_illum", "reproj_moments", "variance")
KEYS = PT + CHAIN + ("normal_depth", "velocity", "fwidth", "history_illum", "modulate")
_oracles = {}
_samples = {}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _eq(got, want, tag):
    idx = np.argwhere(np.any(_bits(got) != _bits(want), axis=-1))
    assert len(idx) == 0, (tag, len(idx), idx[:5].tolist(), got[tuple(idx[0])].tolist(), want[tuple(idx[0])].tolist())


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SM.load(tmp_path_factory.mktemp("sample_moments_ref"))


def _cfg(depth=2, accumulate=False):
    from ptsvgf.camera import parameter_config

    cfg = parameter_config()
    cfg.max_tracing_depth = depth
    cfg.accumulate_color = accumulate
    return cfg


def _renderer(scene, n, accumulate=False, mode="fast", **kw):
    from ptsvgf.renderer import Renderer

    return Renderer(scene, W, H, _cfg(accumulate=accumulate), mode=mode, aspect_corrected=True, atrous_exact=True,
                    run_taa=False, run_output=False, spp=n, **kw)


def _frame(gl, r, move=None):
    """Draw one frame; its planes, counter F, eye and cameraRotate."""
    if move:
        r.camera.orbit(*move)
    r.camera.update()  # (a move restarts the counter here)
    F = int(r.camera.frameCounter)
    r.frame()
    pl = r.planes()
    fr = {k: gl.readback(pl[k]) for k in KEYS}
    fr.update(F=F, eye=np.array(r.camera.cam_position, f32), rot=np.array(r.cameraRotate, f32))
    return fr


def _oracle_samples(name, scene, fr, n):
    """(samples, emission, albedo) of the definition for a recorded frame, cached per (scene, camera, F, n)."""
    key = (name, fr["eye"].tobytes(), fr["rot"].tobytes(), fr["F"], n)
    if key not in _samples:
        if name not in _oracles:
            _oracles[name] = O.OracleScene(scene)
        cfg = _cfg()
        samples = []
        _, e, a = spp_ref(_oracles[name], W, H, fr["F"], n, fr["eye"], fr["rot"], cfg.clamp_threshold, 2, True,
                          use_normal_map=cfg.use_normal_texture, samples=samples)
        _samples[key] = (samples, e, a)
    return _samples[key]


def pattern(N):
    """A count plane holding every value 0 .. N and 255, changing inside every wave."""
    vals = np.array(list(range(N + 1)) + [255], np.uint8)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return vals[(xs + 3 * ys) % len(vals)]


class Bound:
    """A moments texture (and optionally count / statistics planes) bound to every path-tracing pass of a renderer."""

    def __init__(self, gl, r, counts=None, stats=False, moments=True):
        import torch

        self.gl, self.torch, self.r = gl, torch, r
        self.counts = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, np.uint8)).cuda()
        self.stats = torch.full((H, W, 2), float(SENTINEL), dtype=torch.float32, device="cuda") if stats else None
        self.tex = gl.getTextureRGB32F(W, H) if moments else None
        self.fill()
        for p, _ in r.pt_slots:
            p.set_sample_counts(self.counts.data_ptr() if self.counts is not None else 0)
            p.set_sample_stats(self.stats.data_ptr() if self.stats is not None else 0)
            p.set_sample_moments(gl.device_ptr(self.tex) if moments else 0)

    def fill(self):
        if self.tex is not None:
            self.gl.upload_rgba(self.tex, np.full((H, W, 4), SENTINEL, f32))
        self.torch.cuda.synchronize()

    def read(self):
        self.torch.cuda.synchronize()
        return self.gl.readback(self.tex)

    def read_stats(self):
        self.torch.cuda.synchronize()
        return self.stats.cpu().numpy()

    def close(self):
        for p, _ in self.r.pt_slots:
            p.set_sample_counts(0)
            p.set_sample_stats(0)
            p.set_sample_moments(0)
        self.r.close()
        if self.tex is not None:
            self.gl.destroy_texture(self.tex)


# ---------------------------------------------------------- 1. the resolve's plane ---
CASES = [("scene_small", 2), ("scene_small", 3), ("scene_small", 8), ("scene_cornell", 2), ("scene_nan", 3)]


@pytest.mark.parametrize("variant", ["plain", "counts", "accumulate", "counts+accumulate"])
@pytest.mark.parametrize("scene_name,n", CASES)
def test_resolve_plane(gpu, ref, request, scene_name, n, variant):
    """Three still frames (F = 0, 1, 2; with accumulation F > 0 scales r). The colour is the definition's as well."""
    scene = request.getfixturevalue(scene_name)
    counts = pattern(n) if "counts" in variant else None
    acc = "accumulate" in variant
    r = _renderer(scene, n, accumulate=acc)
    b = Bound(gpu, r, counts)
    last = np.zeros((H, W, 4), f32)
    for f in range(3):
        fr = _frame(gpu, r)
        assert fr["F"] == f
        got = b.read()
        samples, e, a = _oracle_samples(scene_name, scene, fr, n)
        tag = (scene_name, n, variant, f)
        _eq(fr["emission"], e, tag + ("emission",))
        _eq(fr["albedo"], a, tag + ("albedo",))
        color = fold_counts(samples, counts if counts is not None else np.full((H, W), 255, np.uint8))
        if acc:
            color = mix_last(last, color, f)
        _eq(fr["color"], color, tag + ("color",))
        last = color
        _eq(got, ref.resolve_plane(samples, e, a, counts, accumulate=acc, F=f), tag + ("moments",))
        if counts is not None:
            miss = fr["normal_depth"][..., 3] == 1.0
            eff = effective(counts, n)
            for k in range(1, n + 1):  # every effective count on a primary hit and on a miss
                assert np.any((eff == k) & ~miss) and np.any((eff == k) & miss), tag + (k,)
            assert set(counts.ravel().tolist()) == set(range(n + 1)) | {255}
        assert np.all(got[..., 3] >= 1.0) and np.any(got[..., 1] > 0.0)
    b.close()


def _sentinel_draw(gl, scene, n, setup):
    r = _renderer(scene, n)
    b = Bound(gl, r, pattern(n))
    setup(r)
    fr = _frame(gl, r)
    got = b.read()
    b.close()
    return fr, got


def test_rows_outside_keep_their_contents(gpu, ref, scene_small):
    rows = (5, 19)

    def setup(r):
        for p, _ in r.pt_slots:
            p.set_rows(*rows)

    n = 3
    fr, got = _sentinel_draw(gpu, scene_small, n, setup)
    samples, e, a = _oracle_samples("scene_small", scene_small, fr, n)
    want = ref.resolve_plane(samples, e, a, pattern(n))
    _eq(got[rows[0]:rows[1]], want[rows[0]:rows[1]], "rows")
    assert np.all(got[:rows[0]] == SENTINEL) and np.all(got[rows[1]:] == SENTINEL)


def test_tiles_outside_the_subset_keep_their_contents(gpu, ref, scene_small):
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    own = (ty * ((W + 15) // 16) + tx) % 2 == 1

    def setup(r):
        r.pass_path_tracing.set_uniform_int("tile_stride", 2)
        r.pass_path_tracing.set_uniform_int("tile_offset", 1)

    n = 3
    fr, got = _sentinel_draw(gpu, scene_small, n, setup)
    samples, e, a = _oracle_samples("scene_small", scene_small, fr, n)
    want = ref.resolve_plane(samples, e, a, pattern(n))
    _eq(got[own], want[own], "subset")
    assert np.all(got[~own] == SENTINEL)


@pytest.mark.parametrize("with_counts", [False, True])
def test_other_outputs_do_not_change(gpu, ref, scene_small, with_counts):
    """With the statistics plane bound as well: colour, emission, albedo and statistics are what they are without
    the moments plane, and all three are the definition's."""
    n = 3
    counts = pattern(n) if with_counts else None
    out = []
    for moments in (False, True):
        r = _renderer(scene_small, n)
        b = Bound(gpu, r, counts, stats=True, moments=moments)
        frames = []
        for f in range(2):
            fr = _frame(gpu, r)
            fr["stats"] = b.read_stats()
            if moments:
                fr["moments"] = b.read()
            frames.append(fr)
        b.close()
        out.append(frames)
    for f, (fa, fb) in enumerate(zip(*out)):
        for k in PT + ("stats",):
            _eq(fa[k], fb[k], (with_counts, f, k))
        samples, e, a = _oracle_samples("scene_small", scene_small, fb, n)
        full = counts if counts is not None else np.full((H, W), 255, np.uint8)
        _eq(fb["stats"], stats_counts(samples, full), ("stats", f))
        _eq(fb["moments"], ref.resolve_plane(samples, e, a, counts), ("moments", f))


def test_plane_is_ignored_at_one_sample(gpu, scene_small):
    r = _renderer(scene_small, 1)
    b = Bound(gpu, r, pattern(2))
    _frame(gpu, r)
    assert np.all(b.read() == SENTINEL)
    b.close()


# ------------------------------------------------- 2. the reproject and variance passes ---
class Chain:
    """The reproject and variance passes of the definition, frame by frame on the inputs the GPU had: this frame's
    G-buffer and path-tracer planes and the history planes of the frame before (zero before the first). `tex` holds
    what the renderer's own illum / moments / variance textures contain, for draws restricted to a row range."""

    def __init__(self, ref, cfg):
        self.ref, self.cfg = ref, cfg
        self.prev = None  # the previous frame's readbacks
        self.prev2 = None

    def check(self, fr, sm, tag, rows=None):
        H, W = fr["color"].shape[:2]  # (the frame's own size: tests/test_gpu_material_zoo.py draws another)
        cfg, z = self.cfg, np.zeros((H, W, 4), f32)
        p = self.prev
        ri, rm = self.ref.reproject(fr["velocity"], fr["color"], fr["albedo"], fr["emission"],
                                    p["history_illum"] if p else z, p["reproj_moments"] if p else z,
                                    fr["normal_depth"], p["normal_depth"] if p else z, fr["fwidth"], f32(1.0 / W),
                                    f32(1.0 / H), cfg.reproj_depth_threshold, cfg.reproj_normal_threshold, sm=sm)
        if rows is not None:  # rows outside keep the textures' contents (fast driver: illum, moments[f & 1], var_out)
            keep_i = p["reproj_illum"] if p else z
            keep_m = self.prev2["reproj_moments"] if self.prev2 else z
            ri[:rows[0]], ri[rows[1]:] = keep_i[:rows[0]], keep_i[rows[1]:]
            rm[:rows[0]], rm[rows[1]:] = keep_m[:rows[0]], keep_m[rows[1]:]
        v = self.ref.variance(ri, rm, fr["normal_depth"], fr["fwidth"], cfg.sigma_l, cfg.sigma_n, sm=sm)
        if rows is not None:
            keep_v = p["variance"] if p else z
            v[:rows[0]], v[rows[1]:] = keep_v[:rows[0]], keep_v[rows[1]:]
        _eq(fr["reproj_illum"], ri, tag + ("reproj_illum",))
        _eq(fr["reproj_moments"], rm, tag + ("reproj_moments",))
        _eq(fr["variance"], v, tag + ("variance",))
        if rows is None:  # the passes behind them, on the oracle (test_gpu_parity.py's tolerance)
            a, hist = v, None
            for i in range(cfg.num_atrous_iterations):
                a = O.atrous(a, fr["normal_depth"], fr["fwidth"], 1 << i, cfg.sigma_l, cfg.sigma_n)
                if i == 1:
                    hist = a
            m = O.modulate(fr["albedo"], fr["emission"], a, fr["normal_depth"])
            for name, got, want in (("history_illum", fr["history_illum"], hist), ("modulate", fr["modulate"], m)):
                if want is None:
                    continue
                assert np.array_equal(np.isnan(got), np.isnan(want)), tag + (name, "NaN pattern")
                d = np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want.astype(np.float64)))
                assert float(np.nanmax(d)) <= 1e-3, tag + (name, float(np.nanmax(d)))
        self.prev2, self.prev = self.prev, fr
        return rm, v


def counts_124():
    """n = 1, 2 and 4 within one image (spp = 4): thirds of the width, so every 16 x 16 block holds two of them."""
    c = np.empty((H, W), np.uint8)
    c[:, :13], c[:, 13:27], c[:, 27:] = 1, 2, 4
    return c


MOVE_AT = {4: (1.0, 0.75)}  # the camera step: bilinear taps and the 3 x 3 rescue in play


@pytest.mark.parametrize("block", [0, 1])
def test_chain_over_frames(gpu, ref, scene_small, block):
    """Frame 0 has no history; the still frames 1 .. 3 take h n across 4 for n = 1 (at frame 3), 2 (frame 1) and 4
    (from the start) in one image; frame 3's reproject and variance draws cover a row range only; the camera steps
    before frame 4."""
    n = 4
    counts = counts_124()
    rows_now = {}

    def stage_rows(stage):  # (-1, -1): the whole frame again
        return rows_now.get(stage, (-1, -1)) if stage in ("reproject", "variance") else None

    r = _renderer(scene_small, n, sample_moments=True, stage_rows=stage_rows)
    import torch

    d_counts = torch.from_numpy(counts).cuda()
    torch.cuda.synchronize()
    for p, _ in r.pt_slots:
        p.set_sample_counts(d_counts.data_ptr())
    for p in r.reproject:
        p.set_uniform_int("reproj_block", block)
    chain = Chain(ref, r.cfg)
    spatial = {1: [], 2: [], 4: []}  # per frame: did some surface pixel of that n take the spatial estimate
    copied = {1: [], 2: [], 4: []}   # ... and did some pixel pass its variance through
    for f in range(5):
        rows = (5, 19) if f == 3 else None
        rows_now.clear()
        if rows:
            rows_now.update(reproject=rows, variance=rows)
        fr = _frame(gpu, r, MOVE_AT.get(f))
        samples, e, a = _oracle_samples("scene_small", scene_small, fr, n)
        _eq(fr["color"], fold_counts(samples, counts), (block, f, "color"))
        sm = ref.resolve_plane(samples, e, a, counts)
        _eq(r.sample_moments(), sm, (block, f, "moments"))
        rm, v = chain.check(fr, sm, (block, f), rows)
        surf = fr["normal_depth"][..., 3] != 1.0
        if f in MOVE_AT:  # the history is fetched between texels, and part of it survives the step
            assert np.any(fr["velocity"][..., :2][surf] != 0.0) and np.any(rm[..., 2][surf] > 1.0)
        for k in spatial:
            sel = surf & (counts == k)
            spatial[k].append(bool(np.any(sel & (rm[..., 2] * f32(k) < 4.0))))
            copied[k].append(bool(np.any(sel & (rm[..., 2] * f32(k) >= 4.0))))
    for p, _ in r.pt_slots:
        p.set_sample_counts(0)
    r.close()
    print("spatial estimate ran per frame:", spatial, "passed through:", copied)
    assert spatial[4] == [False] * 5  # n h >= 4 from the first frame on: the measured variance, never the guess
    assert all(copied[4])
    assert spatial[2][0] and not copied[2][0] and copied[2][1] and not spatial[2][1]
    assert all(spatial[1][:3]) and not any(copied[1][:3]) and copied[1][3]


def test_one_sample_counts_equal_the_unbound_chain(gpu, ref, scene_small):
    """A count plane of ones: sm = (lum, lum^2, 1, 1), and every plane of the chain is the one drawn without the
    sampler, bit for bit; both are the plane-off definition, which is the oracle's."""
    import torch

    n = 2
    ones = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = []
    for on in (False, True):
        r = _renderer(scene_small, n, sample_moments=on)
        for p, _ in r.pt_slots:
            p.set_sample_counts(ones.data_ptr())
        frames = [_frame(gpu, r, {2: (1.0, 0.75)}.get(f)) for f in range(4)]
        if on:
            sm = r.sample_moments()
            assert np.all(sm[..., 2:] == 1.0)
        for p, _ in r.pt_slots:
            p.set_sample_counts(0)
        r.close()
        out.append(frames)
    chain = Chain(ref, _cfg())
    for f, (fa, fb) in enumerate(zip(*out)):
        for k in PT + CHAIN + ("history_illum", "modulate"):
            _eq(fb[k], fa[k], ("n = 1", f, k))
        chain.check(fa, None, ("plane off", f))


# ------------------------------------------------------------------ 3. the renderer ---
TAU = 1.0  # test_gpu_adaptive.py's tolerance: leaves the surface counts neither all 2 nor all N


def _renderer_loop(gl, ref, scene, r, n, sm_on, adaptive, K, tag):
    chain = Chain(ref, r.cfg)
    prev_stats = {}
    for f in range(5):
        fr = _frame(gl, r, {3: (1.0, 0.75)}.get(f))
        samples, e, a = _oracle_samples("scene_small", scene, fr, n)
        counts = None
        if adaptive:
            counts, stats = r.sample_counts(), r.sample_stats()
            slot = f % K
            if slot in prev_stats:
                st_prev, f_prev = prev_stats[slot]
                want = derive_counts(st_prev, fr["velocity"], fr["normal_depth"], float(f - f_prev), TAU, n)
                assert np.array_equal(counts, want), tag + (f, "counts")
            else:
                assert np.all(counts == 255)
            prev_stats[slot] = (stats, f)
        full = counts if counts is not None else np.full((H, W), 255, np.uint8)
        _eq(fr["color"], fold_counts(samples, full), tag + (f, "color"))
        sm = None
        if sm_on:
            sm = ref.resolve_plane(samples, e, a, counts)
            _eq(r.sample_moments(), sm, tag + (f, "moments"))
        chain.check(fr, sm, tag + (f,))


@pytest.mark.parametrize("adaptive", [None, TAU])
@pytest.mark.parametrize("mode,K", [("fast", 1), ("fast", 3), ("reference", 1)])
def test_renderer(gpu, ref, scene_small, mode, K, adaptive):
    """Renderer(spp=4, sample_moments=True) over 5 frames with a camera step, against the loop built from spp_ref,
    the definition and the oracle."""
    n = 4
    r = _renderer(scene_small, n, mode=mode, frames_in_flight=K, adaptive=adaptive, sample_moments=True)
    _renderer_loop(gpu, ref, scene_small, r, n, True, adaptive is not None, K, (mode, K, adaptive))
    r.close()


def test_renderer_without_the_switch_is_unchanged(gpu, ref, scene_small):
    """A renderer with sample_moments=False beside one with it, in one process: today's bits (the plane-off
    definition, which tests/test_sample_moments_ref.py ties to the oracle)."""
    n = 4
    on = _renderer(scene_small, n, sample_moments=True)
    off = _renderer(scene_small, n)
    _frame(gpu, on)
    _renderer_loop(gpu, ref, scene_small, off, n, False, False, 1, ("off",))
    with pytest.raises(ValueError):
        off.sample_moments()
    _frame(gpu, on)
    on.close()
    off.close()


# -------------------------------------------------------------------- 4. refusals ---
def test_band_partition_refuses_the_plane(gpu, scene_small):
    """PT_ERR_STATE before anything launches; with the whole frame as the band again the same pass draws."""
    import torch

    from ptsvgf._lib import PtError

    gl = gpu
    r = _renderer(scene_small, 2)
    b = Bound(gl, r)
    r.frame()  # binds every uniform and sampler
    torch.cuda.synchronize()
    fill = np.full((H, W, 4), SENTINEL, f32)
    for t in r.pt_slots[0][1]:
        gl.upload_rgba(t, fill)
    b.fill()
    pt = r.pt_slots[0][0]
    gl.set_band(W, H, 8, 16, 0, H)
    try:
        with pytest.raises(PtError) as e:
            pt.draw()
        assert e.value.code == -9, e.value  # PT_ERR_STATE
    finally:
        gl.set_band(W, H, 0, H, 0, H)
    torch.cuda.synchronize()
    for t in r.pt_slots[0][1]:
        assert np.all(gl.readback(t) == SENTINEL)
    assert np.all(b.read() == SENTINEL)
    pt.draw()
    assert np.all(b.read()[..., 3] >= 1.0)
    b.close()


@pytest.mark.parametrize("which", ["reproject", "variance"])
def test_wrong_texture_size_is_refused(gpu, scene_small, which):
    from ptsvgf._lib import PtError
    from ptsvgf.gl import GL_TEXTURE_2D

    gl = gpu
    r = _renderer(scene_small, 2)
    r.frame()  # binds every other sampler
    p = r.reproject[0] if which == "reproject" else r.variance_compute_pass
    bad = gl.getTextureRGB32F(W + 1, H)
    p.set_texture_uniform(GL_TEXTURE_2D, bad, "gSampleMoments")
    with pytest.raises(PtError) as e:
        p.draw()
    assert e.value.code == -6, e.value  # PT_ERR_ARG
    r.close()
    gl.destroy_texture(bad)


def test_arguments(gpu, scene_small):
    from ptsvgf._lib import PtError

    for kw in (dict(n=1, sample_moments=True), dict(n=2, sample_moments=True, band=(0, H, 0, H)),
               dict(n=2, sample_moments=True, frames_in_flight=2, pt_source=lambda f, slot, stream: {}),
               dict(n=2, sample_moments=True, frames_in_flight=2, trace_batch=2)):
        with pytest.raises(ValueError):
            _renderer(scene_small, **kw)
    r = _renderer(scene_small, 2, sample_moments=True)
    with pytest.raises(ValueError):
        r.spp = 1
    assert r.spp == 2
    with pytest.raises(ValueError):
        r.sample_moments()  # no frame drawn yet
    with pytest.raises(PtError) as e:  # the setter is the path-tracing pass's
        r.variance_compute_pass.set_sample_moments(gpu.device_ptr(r._sm[0]))
    assert e.value.code == -6, e.value
    r.close()


# --------------------------------------------------------------------- 5. the CLI ---
def test_render_cli_sample_moments_flag(gpu, scene_cornell, tmp_path, monkeypatch):
    """--sample-moments reaches the renderer: the denoised image is no longer the one drawn without it. main() runs in
    this process on the session's library and scene, as in test_render_cli_spp.py."""
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod
    from test_render_cli_spp import _pfm

    monkeypatch.setattr(scene_mod, "build_scene", lambda name: scene_cornell)
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    out = {}
    for on in (False, True):
        pfm = str(tmp_path / f"sm{on}.pfm")
        args = ["--width", "64", "--height", "48", "--frames", "2", "--scene", "cornell_teapot", "--view",
                "svgf_modulate_pic", "--png", str(tmp_path / f"sm{on}.png"), "--pfm", pfm, "--spp", "4"]
        assert render_cli.main(args + (["--sample-moments"] if on else [])) == 0
        out[on] = _pfm(pfm)
    assert np.isfinite(out[True]).all() and out[True].any()
    assert not np.array_equal(out[False], out[True])
    with pytest.raises(ValueError):
        render_cli.main(["--width", "64", "--height", "48", "--frames", "1", "--scene", "cornell_teapot",
                         "--sample-moments"])

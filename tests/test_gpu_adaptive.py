"""Adaptive sample counts (pt_pass_set_sample_counts / pt_pass_set_sample_stats / pt_sample_counts_derive,
Renderer(spp=N, adaptive=tau); kernels_wf_shade.hip wf_shade_counted, kernels_spp.hip wf_spp_resolve_adaptive and
spp_counts_kernel) against their definition (tests/adaptive_ref.py over spp_ref.py's per-sample colours of the CPU
oracle). 160 x 96, test_gpu_spp.py's frames and scenes; every comparison is bitwise (uint32 views; counts as
integers)."""
import numpy as np
import pytest

import oracle_ref as O
from adaptive_ref import derive_counts, effective, fold_counts, stats_counts
from spp_ref import mix_last, spp_ref
from test_gpu_shade_fold import PLANES, H, W
from test_gpu_spp import SENTINEL, STILL, _renderer

pytestmark = pytest.mark.gpu

f32 = np.float32
_oracles = {}
_samples = {}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _eq(got, want, tag):
    idx = np.argwhere(np.any(_bits(got) != _bits(want), axis=-1))
    assert len(idx) == 0, (tag, len(idx), idx[:5].tolist())


def pattern(N):
    """A count plane holding every value 0 .. N and 255: per tile (10 x 6 tiles of 16 x 16) all 1, one value for the
    whole tile, a per-pixel cycle (changes inside every wave), or two values split at the tile's middle column."""
    vals = np.array(list(range(N + 1)) + [255], np.uint8)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    t = (ys // 16) * ((W + 15) // 16) + xs // 16
    cyc = vals[(xs + 3 * ys) % len(vals)]
    whole = vals[(t // 4) % len(vals)]
    split = np.where(xs % 16 < 8, vals[(t // 4 + 1) % len(vals)], vals[(t // 4 + 3) % len(vals)])
    out = np.select([t % 4 == 0, t % 4 == 1, t % 4 == 2], [np.uint8(1), whole, cyc], split).astype(np.uint8)
    assert set(out.ravel()) == set(vals.tolist())
    return out


class Bound:
    """Count and statistics planes on the device, bound to every path-tracing pass of a renderer."""

    def __init__(self, r, counts=None, stats=True):
        import torch

        self.torch = torch
        self.r = r
        self.counts = None if counts is None else torch.from_numpy(np.ascontiguousarray(counts, np.uint8)).cuda()
        self.stats = torch.full((H, W, 2), float(SENTINEL), dtype=torch.float32, device="cuda") if stats else None
        torch.cuda.synchronize()
        for p, _ in r.pt_slots:
            p.set_sample_counts(self.counts.data_ptr() if self.counts is not None else 0)
            p.set_sample_stats(self.stats.data_ptr() if self.stats is not None else 0)

    def read_stats(self):
        self.torch.cuda.synchronize()
        return self.stats.cpu().numpy()

    def unbind(self):
        for p, _ in self.r.pt_slots:
            p.set_sample_counts(0)
            p.set_sample_stats(0)


def _run(gl, scene, n, counts=None, stats=True, moves=STILL, bind=True, **kw):
    """test_gpu_spp._run with the planes bound: per frame the path tracer's planes, normal/depth, the statistics
    the draw wrote, F, eye and cameraRotate."""
    r = _renderer(scene, spp=n, **kw)
    b = Bound(r, counts, stats) if bind else None
    out = []
    for mv in moves:
        if mv:
            r.camera.orbit(*mv)
        r.camera.update()
        F = int(r.camera.frameCounter)
        r.frame()
        pl = r.planes()
        fr = {k: gl.readback(pl[k]) for k in PLANES + ("normal_depth",)}
        if b is not None and b.stats is not None:
            fr["stats"] = b.read_stats()
        fr.update(F=F, eye=np.array(r.camera.cam_position, f32), rot=np.array(r.cameraRotate, f32))
        out.append(fr)
    r.close()
    return out


def _oracle_samples(name, scene, fr, n, depth=2):
    """(samples, emission, albedo) of the definition for a recorded frame, cached per (scene, camera, F, n, depth)."""
    from ptsvgf.camera import parameter_config

    key = (name, fr["eye"].tobytes(), fr["rot"].tobytes(), fr["F"], n, depth)
    if key not in _samples:
        if name not in _oracles:
            _oracles[name] = O.OracleScene(scene)
        cfg = parameter_config()
        samples = []
        _, e, a = spp_ref(_oracles[name], W, H, fr["F"], n, fr["eye"], fr["rot"], cfg.clamp_threshold, depth, True,
                          use_normal_map=cfg.use_normal_texture, samples=samples)
        _samples[key] = (samples, e, a)
    return _samples[key]


@pytest.fixture(scope="module")
def plain(gpu, request):
    """Plain draws (nothing bound) per (scene, spp, depth), rendered once per module."""
    cache = {}

    def get(name, n, depth=2):
        if (name, n, depth) not in cache:
            cache[name, n, depth] = _run(gpu, request.getfixturevalue(name), n, bind=False, depth=depth)
        return cache[name, n, depth]

    return get


@pytest.fixture(scope="module")
def patterned(gpu, request):
    """Draws with pattern(n) and a statistics plane bound, at the renderer's defaults."""
    cache = {}

    def get(name, n, depth=2):
        if (name, n, depth) not in cache:
            cache[name, n, depth] = _run(gpu, request.getfixturevalue(name), n, pattern(n), depth=depth)
        return cache[name, n, depth]

    return get


def _same_frames(a, b, tag, keys=PLANES + ("stats",)):
    assert len(a) == len(b)
    for f, (fa, fb) in enumerate(zip(a, b)):
        for k in keys:
            _eq(fa[k], fb[k], (tag, f, k))


# ------------------------------------------------------------ 1. the definition ---
@pytest.mark.parametrize("n,depth", [(2, 2), (3, 2), (8, 2), (2, 1), (2, 3)])
@pytest.mark.parametrize("scene_name", ["scene_small", "scene_cornell", "scene_nan"])
def test_equals_the_definition(gpu, patterned, scene_name, n, depth, request):
    scene = request.getfixturevalue(scene_name)
    counts = pattern(n)
    eff = effective(counts, n)
    got = patterned(scene_name, n, depth)
    assert [f["F"] for f in got] == [0, 0, 0, 0, 1]
    for f, fr in enumerate(got):
        miss = fr["normal_depth"][..., 3] == 1.0
        for k in range(1, n + 1):  # every effective count on a primary hit and on a miss
            assert np.any((eff == k) & ~miss) and np.any((eff == k) & miss), (scene_name, f, k)
        samples, e, a = _oracle_samples(scene_name, scene, fr, n, depth)
        tag = (scene_name, n, depth, f)
        _eq(fr["color"], fold_counts(samples, counts), tag + ("color",))
        _eq(fr["emission"], e, tag + ("emission",))
        _eq(fr["albedo"], a, tag + ("albedo",))
        _eq(fr["stats"], stats_counts(samples, counts), tag + ("stats",))
    assert all(f["color"][..., :3].any() for f in got)


# ---------------------------------------------------------- 2. bit-equalities ---
@pytest.mark.parametrize("c", ["N", 255])
def test_full_counts_equal_the_plain_draw(gpu, plain, scene_small, c):
    n = 3
    got = _run(gpu, scene_small, n, np.full((H, W), n if c == "N" else 255, np.uint8))
    _same_frames(got, plain("scene_small", n), ("counts", c), PLANES)
    samples = _oracle_samples("scene_small", scene_small, got[-1], n)[0]
    _eq(got[-1]["stats"], stats_counts(samples, np.full((H, W), 255, np.uint8)), "stats at full counts")


def test_stats_alone_and_unbinding(gpu, plain, patterned, scene_small):
    """A statistics plane without counts: the plain colour, the statistics of N samples. After unbinding both planes
    the draw is the plain draw and writes no statistics."""
    n = 2
    want = plain("scene_small", n)
    got = _run(gpu, scene_small, n, None, stats=True)
    _same_frames(got, want, "stats alone", PLANES)
    _same_frames(got, _run(gpu, scene_small, n, np.full((H, W), 255, np.uint8)), "stats alone / 255", ("stats",))
    r = _renderer(scene_small, spp=n)
    b = Bound(r, pattern(n))
    r.frame()
    first = {k: gpu.readback(r.planes()[k]) for k in PLANES}
    assert not np.array_equal(_bits(first["color"]), _bits(want[0]["color"]))
    _eq(first["color"], patterned("scene_small", n)[0]["color"], "bound")
    b.unbind()
    b.stats.fill_(float(SENTINEL))
    r.camera.frameCounter -= 1  # the same frame again
    r.frame()
    again = {k: gpu.readback(r.planes()[k]) for k in PLANES}
    stats = b.read_stats()
    r.close()
    for k in PLANES:
        _eq(again[k], want[0][k], ("unbound", k))
    assert np.all(stats == SENTINEL)


def test_planes_are_ignored_at_one_sample(gpu, plain, scene_small):
    got = _run(gpu, scene_small, 1, pattern(2))
    _same_frames(got, plain("scene_small", 1), "spp=1", PLANES)
    assert all(np.all(f["stats"] == SENTINEL) for f in got)


# ------------------------------------- 3. no ray for a sample that does not exist ---
def test_absent_samples_trace_no_ray(gpu, scene_small):
    n = 4

    def go(spp, counter, counts):
        r = _renderer(scene_small, spp=spp)
        b = Bound(r, counts, stats=False) if counts is not None else None
        r.frame()  # F = 0
        r.camera.frameCounter = counter(1)
        st = r.trace_stats()  # the frame with F = 1
        color = gpu.readback(r.planes()["color"])
        r.close()
        del b
        return st, color

    st_a, col_a = go(n, lambda F: F, np.ones((H, W), np.uint8))
    st_1, col_1 = go(1, lambda F: n * F, None)
    print("counts = 1 at spp 4:", st_a, "spp 1:", st_1)
    _eq(col_a, col_1, "colour")
    for k in ("primary_rays", "bounce_rays", "shadow_rays", "shadow_point_rays"):
        assert st_a[k] == st_1[k] > 0, k
    full = go(n, lambda F: F, None)[0]
    assert full["bounce_rays"] > 2 * st_a["bounce_rays"]


# ------------------------------------------------------ 4. untouched pixels ---
def _sentinel_run(gl, scene, n, setup):
    r = _renderer(scene, spp=n)
    b = Bound(r, pattern(n))
    setup(r)
    fill = np.full((H, W, 4), SENTINEL, f32)
    for t in r.pt_slots[0][1]:
        gl.upload_rgba(t, fill)
    r.frame()
    got = {k: gl.readback(r.planes()[k]) for k in PLANES}
    got["stats"] = b.read_stats()
    r.close()
    return got


def test_rows_outside_keep_their_contents(gpu, patterned, scene_small):
    rows = (21, 70)
    want = patterned("scene_small", 2)[0]

    def setup(r):
        for p, _ in r.pt_slots:
            p.set_rows(*rows)

    got = _sentinel_run(gpu, scene_small, 2, setup)
    for k in PLANES + ("stats",):
        _eq(got[k][rows[0]:rows[1]], want[k][rows[0]:rows[1]], ("rows", k))
        assert np.all(got[k][:rows[0]] == SENTINEL) and np.all(got[k][rows[1]:] == SENTINEL), k


def test_tiles_outside_the_subset_keep_their_contents(gpu, patterned, scene_small):
    want = patterned("scene_small", 2)[0]
    ty, tx = np.meshgrid(np.arange(H) // 16, np.arange(W) // 16, indexing="ij")
    own = (ty * ((W + 15) // 16) + tx) % 2 == 1

    def setup(r):
        r.pass_path_tracing.set_uniform_int("tile_stride", 2)
        r.pass_path_tracing.set_uniform_int("tile_offset", 1)

    got = _sentinel_run(gpu, scene_small, 2, setup)
    for k in PLANES + ("stats",):
        _eq(got[k][own], want[k][own], ("subset", k))
        assert np.all(got[k][~own] == SENTINEL), k


# ------------------------------------------------------ 5. switches keep the bits ---
SWITCHES = {
    "shade_fold=0": dict(uniforms={"shade_fold": 0}),
    "trace_fork=1": dict(uniforms={"trace_fork": 1}),
    "trace_refill=0": dict(uniforms={"trace_refill": 0}),
    "point_bins=0": dict(uniforms={"point_bins": 0}),
    "point_bins=1": dict(uniforms={"point_bins": 1}),
    "reference driver": dict(mode="reference"),
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_switches_keep_the_bits(gpu, patterned, scene_small, switch):
    n = 3
    kw = dict(SWITCHES[switch])
    moves = STILL[:2] + [None] if switch == "reference driver" else STILL
    got = _run(gpu, scene_small, n, pattern(n), moves=moves, **kw)
    want = patterned("scene_small", n)
    if switch == "reference driver":  # (0, 0, 1): the first two frames are the fast driver's
        _same_frames(got[:2], want[:2], switch)
        samples = _oracle_samples("scene_small", scene_small, got[2], n)[0]
        _eq(got[2]["color"], fold_counts(samples, pattern(n)), switch)
        _eq(got[2]["stats"], stats_counts(samples, pattern(n)), switch)
    else:
        _same_frames(got, want, switch)


def test_accumulate(gpu, scene_small):
    n = 2
    counts = pattern(n)
    got = _run(gpu, scene_small, n, counts, moves=[None, None, None], accumulate=True)
    last = np.zeros((H, W, 4), f32)
    for f, fr in enumerate(got):
        assert fr["F"] == f
        samples = _oracle_samples("scene_small", scene_small, fr, n)[0]
        want = mix_last(last, fold_counts(samples, counts), f)
        _eq(fr["color"], want, ("accumulate", f))
        _eq(fr["stats"], stats_counts(samples, counts), ("accumulate stats", f))
        last = want


# ---------------------------------------------------------- 6. the derive kernel ---
def _synthetic(w, h, seed):
    """Statistics, motion and normal/depth planes with every case of the rule in them."""
    rng = np.random.default_rng(seed)
    stats = np.empty((h, w, 2), f32)
    stats[..., 0] = rng.random((h, w), dtype=f32) * f32(2.0)
    stats[..., 1] = rng.random((h, w), dtype=f32) ** 3 * f32(0.5)
    stats[..., 1][rng.random((h, w)) < 0.3] = 0.0
    for _ in range(4):  # v = -1 islands, NaN and infinite statistics
        y, x = rng.integers(0, h - 2), rng.integers(0, w - 2)
        stats[y:y + 2, x:x + 3, 1] = -1.0
    stats[h // 2, w // 3] = (np.nan, 0.1)
    stats[h // 3, w // 2] = (0.5, np.nan)
    stats[h // 4, w // 4] = (0.5, np.inf)
    stats[1, 1] = (0.0, 1e-9)
    stats[0, w - 1] = (np.inf, 0.3)
    nd = rng.random((h, w, 4), dtype=f32)
    nd[..., 3] = 0.25
    nd[: h // 3, : w // 2, 3] = 1.0  # background
    nd[h - 1, w - 1, 3] = 1.0
    return stats, nd


MOTIONS = ["zero", "whole", "half", "leaving", "random", "non-finite"]


def _motion(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w, 4), f32)
    if kind == "whole":
        m[..., 0], m[..., 1] = f32(3.0) / f32(w), f32(-2.0) / f32(h)
    elif kind == "half":
        m[..., 0], m[..., 1] = f32(0.5) / f32(w), f32(-1.5) / f32(h)
    elif kind == "leaving":
        m[..., 0], m[..., 1] = f32(0.6), f32(-0.4)
    elif kind in ("random", "non-finite"):
        m[..., :2] = (rng.random((h, w, 2), dtype=f32) - f32(0.5)) * f32(0.2)
    if kind == "non-finite":
        m[2, 3, 0] = np.nan
        m[3, 2, 1] = np.nan
        m[4, 5, 0] = np.inf
        m[5, 4, 1] = -np.inf
        m[6, 6, :2] = 3.0e38
    m[..., 2:] = rng.random((h, w, 2), dtype=f32)
    return m


@pytest.mark.parametrize("lag", [1.0, 4.0])
@pytest.mark.parametrize("size", [(37, 19), (160, 96)])
def test_derive_kernel(gpu, size, lag):
    import torch

    gl = gpu
    w, h = size
    stats, nd = _synthetic(w, h, 11)
    t_m, t_nd = gl.getTextureRGB32F(w, h), gl.getTextureRGB32F(w, h)
    gl.upload_rgba(t_nd, nd)
    d_stats = torch.from_numpy(stats).cuda()
    out = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    seen = set()
    for kind in MOTIONS:
        motion = _motion(kind, w, h, 5)
        gl.upload_rgba(t_m, motion)
        for tau, n in ((0.3, 8), (1.0, 4), (0.05, 2)):
            out.fill_(77)
            torch.cuda.synchronize()
            gl.sample_counts_derive(d_stats.data_ptr(), t_m, t_nd, lag, tau, n, out.data_ptr())
            gl.sync()
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            want = derive_counts(stats, motion, nd, lag, tau, n)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (kind, tau, n, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
            if n == 8:
                seen |= set(want.ravel().tolist())
    assert seen == set(range(1, 9))  # the cases reach every count
    gl.destroy_texture(t_m)
    gl.destroy_texture(t_nd)


# ------------------------------------------------------------ 7. the closed loop ---
TAU = 1.0  # on the CPU beforehand (the definition's derive over the oracle's N = 4 statistics of scene_small's first
#            view): 1929 / 920 / 913 surface pixels at 2 / 3 / 4; 0.5 leaves 95 % at 4 and 2.0 all at 2


@pytest.mark.parametrize("mode,K", [("fast", 1), ("fast", 2), ("reference", 1)])
def test_closed_loop(gpu, plain, scene_small, mode, K):
    """Renderer(spp=4, adaptive=TAU) over still frames: each slot's first draw is the plain frame; afterwards the
    counts are the definition's derive of the slot's previous statistics with the frame's G-buffer, and the colour
    the definition's fold of the oracle's samples under those counts."""
    n = 4
    gl = gpu
    r = _renderer(scene_small, spp=n, adaptive=TAU, frames_in_flight=K, mode=mode)
    base = plain("scene_small", n)[0]  # F = 0 at the first camera state
    prev_stats = {}
    frames = 2 * K + 2
    interesting = False
    for f in range(frames):
        r.camera.update()
        F = int(r.camera.frameCounter)
        assert F == f
        r.frame()
        pl = r.planes()
        fr = {k: gl.readback(pl[k]) for k in PLANES + ("normal_depth", "velocity")}
        fr.update(F=F, eye=np.array(r.camera.cam_position, f32), rot=np.array(r.cameraRotate, f32))
        counts, stats = r.sample_counts(), r.sample_stats()
        slot = f % K
        samples = _oracle_samples("scene_small", scene_small, fr, n)[0]
        if slot not in prev_stats:
            assert np.all(counts == 255)
            if f == 0:
                for k in PLANES:
                    _eq(fr[k], base[k], ("first draw", k))
        else:
            st_prev, f_prev = prev_stats[slot]
            want = derive_counts(st_prev, fr["velocity"], fr["normal_depth"], float(f - f_prev), TAU, n)
            surf = want[fr["normal_depth"][..., 3] != 1.0]
            if not (np.all(surf == 2) or np.all(surf == n)):
                interesting = True
            bad = np.argwhere(counts != want)
            assert len(bad) == 0, ("counts", f, len(bad), bad[:5].tolist())
        _eq(fr["color"], fold_counts(samples, counts), ("colour", f))
        _eq(stats, stats_counts(samples, counts), ("stats", f))
        prev_stats[slot] = (stats, f)
    r.close()
    assert interesting  # TAU leaves the surface counts neither all 2 nor all N


def test_python_arguments(gpu, scene_small):
    for kw in (dict(spp=1, adaptive=0.5), dict(adaptive=0.5), dict(spp=4, adaptive=0.0), dict(spp=4, adaptive=-1.0),
               dict(spp=4, adaptive=float("nan"))):
        with pytest.raises(ValueError):
            _renderer(scene_small, **kw)
    r = _renderer(scene_small, spp=2, adaptive=0.5)
    with pytest.raises(ValueError):
        r.spp = 1
    assert r.spp == 2
    r.close()
    r = _renderer(scene_small, spp=2)
    with pytest.raises(ValueError):
        r.sample_counts()
    r.close()


# ---------------------------------------------------------------- 8. refusals ---
@pytest.mark.parametrize("case", ["tau=0", "tau<0", "tau=nan", "nmax=1", "nmax=9", "sizes"])
def test_derive_refusals(gpu, case):
    import torch

    from ptsvgf._lib import PtError

    gl = gpu
    w, h = 37, 19
    t_m, t_nd = gl.getTextureRGB32F(w, h), gl.getTextureRGB32F(w + 1 if case == "sizes" else w, h)
    stats = torch.zeros((h, w, 2), dtype=torch.float32, device="cuda")
    out = torch.full((h, w), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tau = {"tau=0": 0.0, "tau<0": -0.5, "tau=nan": float("nan")}.get(case, 0.5)
    n = {"nmax=1": 1, "nmax=9": 9}.get(case, 4)
    with pytest.raises(PtError) as e:
        gl.sample_counts_derive(stats.data_ptr(), t_m, t_nd, 1.0, tau, n, out.data_ptr())
    assert e.value.code == -6, e.value  # PT_ERR_ARG
    gl.sync()
    torch.cuda.synchronize()
    assert torch.all(out == 77)
    gl.destroy_texture(t_m)
    gl.destroy_texture(t_nd)


@pytest.mark.parametrize("which", ["counts", "stats"])
def test_band_partition_refuses_the_planes(gpu, patterned, scene_small, which):
    """Either plane under an active pt_set_band partition: PT_ERR_STATE before anything launches; with the whole
    frame as the band again the same pass draws."""
    import torch

    from ptsvgf._lib import PtError

    gl = gpu
    n = 2
    r = _renderer(scene_small, spp=n)
    b = Bound(r, pattern(n) if which == "counts" else None, stats=which == "stats")
    r.frame()  # binds every uniform and sampler
    torch.cuda.synchronize()
    fill = np.full((H, W, 4), SENTINEL, f32)
    for t in r.pt_slots[0][1]:
        gl.upload_rgba(t, fill)
    if b.stats is not None:
        b.stats.fill_(float(SENTINEL))
    torch.cuda.synchronize()
    pt = r.pt_slots[0][0]
    gl.set_band(W, H, 16, 64, 0, H)
    try:
        with pytest.raises(PtError) as e:
            pt.draw()
        assert e.value.code == -9, e.value  # PT_ERR_STATE
    finally:
        gl.set_band(W, H, 0, H, 0, H)
    torch.cuda.synchronize()
    for t in r.pt_slots[0][1]:
        assert np.all(gl.readback(t) == SENTINEL)
    if b.stats is not None:
        assert np.all(b.read_stats() == SENTINEL)
    pt.draw()
    torch.cuda.synchronize()
    got = gl.readback(r.pt_slots[0][1][0])
    r.close()
    if which == "counts":
        _eq(got, patterned("scene_small", n)[0]["color"], "valid draw after")
    else:
        assert np.all(b.read_stats()[..., 1] != SENTINEL)


# ------------------------------------------------------------------- 9. the CLI ---
def test_render_cli_adaptive_flag(gpu, scene_cornell, tmp_path, monkeypatch):
    """--adaptive TAU reaches the renderer: after the first frame (N everywhere) the image is no longer the uniform
    one. main() runs in this process on the session's library and scene, as in test_render_cli_spp.py."""
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod
    from test_render_cli_spp import _pfm

    monkeypatch.setattr(scene_mod, "build_scene", lambda name: scene_cornell)
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    out = {}
    for tau in (None, 2.0):
        pfm = str(tmp_path / f"tau{tau}.pfm")
        args = ["--width", "64", "--height", "48", "--frames", "3", "--scene", "cornell_teapot", "--view",
                "path_tracing_pic_1spp", "--png", str(tmp_path / f"tau{tau}.png"), "--pfm", pfm, "--spp", "4"]
        assert render_cli.main(args + (["--adaptive", str(tau)] if tau else [])) == 0
        out[tau] = _pfm(pfm)
    assert np.isfinite(out[2.0]).all() and out[2.0].any()
    assert not np.array_equal(out[None], out[2.0])
    with pytest.raises(ValueError):
        render_cli.main(["--width", "64", "--height", "48", "--frames", "1", "--scene", "cornell_teapot", "--adaptive",
                         "0.5"])

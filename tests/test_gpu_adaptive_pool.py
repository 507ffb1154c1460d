"""Pooled adaptive sample counts (pt_sample_counts_pool, Renderer(adaptive_pool=W); kernels_spp.hip
spp_pool_kernel) against their definition (tests/adaptive_pool_ref.py): the kernel on synthetic planes, every refusal,
the closed loop over the renderer's own planes, the unchanged un-pooled path and the CLI flags. Comparisons are
bitwise (uint32 views; two NaNs count as equal whatever their payloads; counts as integers)."""
import numpy as np
import pytest

from adaptive_pool_ref import ABSOLUTE, RELATIVE, pool_step
from adaptive_ref import fold_counts, stats_counts
from test_gpu_adaptive import MOTIONS, _motion, _oracle_samples
from test_gpu_shade_fold import PLANES, H, W
from test_gpu_spp import _renderer

pytestmark = pytest.mark.gpu

f32 = np.float32
W_MAX, ZETA = 12.0, 0.1
SENT_F, SENT_B = f32(-7.25), 77
PAD = 64  # sentinel elements on either side of an output plane


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _eq(got, want, tag):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    bad = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    idx = np.argwhere(np.any(bad, axis=-1))
    assert len(idx) == 0, (tag, len(idx), idx[:5].tolist(), got[tuple(idx[0])], want[tuple(idx[0])])


def _eq_counts(got, want, tag):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (tag, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# --------------------------------------------------- 1. the kernel on synthetic planes ---
def _synthetic(w, h, n_prev, seed):
    """stats, counts_prev, pool_in and normal/depth planes with every case of the rule in them (any size >= 1 x 1)."""
    rng = np.random.default_rng(seed)
    stats = np.empty((h, w, 2), f32)
    stats[..., 0] = rng.random((h, w), dtype=f32) * f32(2.0)
    stats[..., 1] = rng.random((h, w), dtype=f32) ** 3 * f32(0.5)
    stats[..., 1][rng.random((h, w)) < 0.3] = 0.0
    nd = rng.random((h, w, 4), dtype=f32)
    nd[..., 2] = rng.random((h, w), dtype=f32) * f32(2.5) + f32(0.5)
    nd[..., 3] = 0.25
    pool = np.empty((h, w, 4), f32)
    pool[..., 0] = rng.random((h, w), dtype=f32) * f32(2.0)
    pool[..., 1] = rng.random((h, w), dtype=f32) ** 3 * f32(0.5)
    pool[..., 2] = rng.choice(np.array([0.0, 1.0, 2.5, W_MAX - 1.0, W_MAX], f32), size=(h, w))
    # depth steps at zeta's boundary: the history's z just inside, just outside (either side) and equal
    step = rng.choice(np.array([0.0, 0.0, 0.999, -0.999, 1.001, -1.001, 1.0, -1.0, 3.0], f32), size=(h, w))
    pool[..., 3] = (nd[..., 2] * (f32(1.0) + f32(ZETA) * step).astype(f32)).astype(f32)
    counts = rng.choice(np.array(list(range(n_prev + 2)) + [255], np.uint8), size=(h, w))

    def at(fy, fx):  # a pixel of the plane by fractions, so that every size has it
        return min(int(fy * h), h - 1), min(int(fx * w), w - 1)

    if h >= 8 and w >= 8:
        for _ in range(4):  # v = -1 islands in both planes, background runs
            y, x = rng.integers(0, h - 2), rng.integers(0, w - 3)
            stats[y:y + 2, x:x + 3, 1] = -1.0
            y, x = rng.integers(0, h - 2), rng.integers(0, w - 3)
            pool[y:y + 2, x:x + 3, 1] = -1.0
            y, x = rng.integers(0, h - 1), rng.integers(0, w - 6)
            nd[y, x:x + 6, 3] = 1.0
        nd[: h // 3, : w // 2, 3] = 1.0
        nd[h - 1, w - 1, 3] = 1.0
        stats[at(0.5, 0.33)] = (np.nan, 0.1)
        stats[at(0.33, 0.5)] = (0.5, np.nan)
        stats[at(0.25, 0.25)] = (0.5, np.inf)
        stats[at(0.75, 0.25)] = (np.inf, 0.3)
        stats[at(0.6, 0.6)] = (0.0, 1e-9)
        pool[at(0.5, 0.66)][:2] = (np.nan, 0.1)
        pool[at(0.66, 0.5)][:2] = (0.5, np.nan)
        pool[at(0.75, 0.75)][:2] = (0.5, np.inf)
        pool[at(0.4, 0.8)][:2] = (-np.inf, 0.2)
        pool[at(0.8, 0.4)][2] = np.nan
        pool[at(0.9, 0.6)][3] = np.nan
        pool[at(0.6, 0.9)][3] = np.inf
        nd[at(0.7, 0.6)][2] = np.nan
        nd[at(0.55, 0.7)][2] = 1e-6   # under the floor on |z|
        pool[at(0.55, 0.7)][3] = 5e-6
    return stats, counts, pool, nd


def _motions(w, h):
    for kind in MOTIONS:
        if kind == "non-finite" and (w < 8 or h < 8):  # _motion's non-finite texels need a 7 x 7 plane
            m = _motion("zero", w, h, 5)
            m[0, 0, 0] = np.nan
        else:
            m = _motion(kind, w, h, 5)
        yield kind, m


class Outputs:
    """pool_out and out_u8 on the device with PAD sentinel elements on either side."""

    def __init__(self, w, h):
        import torch

        self.torch, self.w, self.h = torch, w, h
        self.pool = torch.empty((h * w + 2 * PAD, 4), dtype=torch.float32, device="cuda")
        self.cnt = torch.empty((h * w + 2 * PAD * 16,), dtype=torch.uint8, device="cuda")
        self.reset()

    def reset(self):
        self.pool.fill_(float(SENT_F))
        self.cnt.fill_(SENT_B)
        self.torch.cuda.synchronize()

    @property
    def pool_ptr(self):
        return self.pool.data_ptr() + PAD * 16

    @property
    def cnt_ptr(self):
        return self.cnt.data_ptr() + PAD * 16

    def read(self):
        self.torch.cuda.synchronize()
        p, c = self.pool.cpu().numpy(), self.cnt.cpu().numpy()
        assert np.all(p[:PAD] == SENT_F) and np.all(p[-PAD:] == SENT_F), "pool_out sentinels"
        assert np.all(c[:PAD * 16] == SENT_B) and np.all(c[-PAD * 16:] == SENT_B), "out_u8 sentinels"
        return p[PAD:-PAD].reshape(self.h, self.w, 4), c[PAD * 16:-PAD * 16].reshape(self.h, self.w)

    def untouched(self):
        self.torch.cuda.synchronize()
        return bool(self.torch.all(self.pool == float(SENT_F))) and bool(self.torch.all(self.cnt == SENT_B))


ABSENT = [(), ("stats",), ("counts",), ("pool",), ("stats", "counts", "pool")]


@pytest.mark.parametrize("rule", [RELATIVE, ABSOLUTE])
@pytest.mark.parametrize("lag", [1.0, 4.0])
@pytest.mark.parametrize("size", [(1, 1), (16, 16), (37, 19), (160, 96)])
def test_kernel_equals_the_definition(gpu, size, lag, rule):
    import torch

    gl = gpu
    w, h = size
    n_prev = 3
    stats, counts, pool, nd = _synthetic(w, h, n_prev, 11)
    t_m, t_nd = gl.getTextureRGB32F(w, h), gl.getTextureRGB32F(w, h)
    gl.upload_rgba(t_nd, nd)
    d_stats, d_counts, d_pool = (torch.from_numpy(a).cuda() for a in (stats, counts, pool))
    out = Outputs(w, h)
    seen, cases = set(), set()
    for kind, motion in _motions(w, h):
        gl.upload_rgba(t_m, motion)
        for absent in ABSENT:
            for tau, n in ((0.3, 8), (1.0, 4)):
                out.reset()
                gl.sample_counts_pool(0 if "stats" in absent else d_stats.data_ptr(),
                                      0 if "counts" in absent else d_counts.data_ptr(), n_prev,
                                      0 if "pool" in absent else d_pool.data_ptr(), t_m, t_nd, lag, W_MAX, ZETA, rule,
                                      tau, n, out.pool_ptr, out.cnt_ptr)
                gl.sync()
                got_pool, got_cnt = out.read()
                want_pool, want_cnt = pool_step(None if "stats" in absent else stats,
                                                None if "counts" in absent else counts, n_prev,
                                                None if "pool" in absent else pool, motion, nd, lag, W_MAX, ZETA, rule,
                                                tau, n)
                tag = (size, lag, rule, kind, absent, tau, n)
                _eq(got_pool, want_pool, tag)
                _eq_counts(got_cnt, want_cnt, tag)
                if n == 8:
                    seen |= set(want_cnt.ravel().tolist())
                    cases |= set(want_pool[..., 2].ravel().tolist())
    if size == (160, 96):  # the planes reach every count ...
        assert seen == set(range(1, 9)), seen
    if w * h >= 256:  # ... and weights that are empty, kept, combined and capped
        assert {0.0, 1.0, 2.5, 3.0, 4.0, 5.5, W_MAX} <= cases, cases
    gl.destroy_texture(t_m)
    gl.destroy_texture(t_nd)


# ------------------------------------------------------------------ 2. refusals ---
REFUSALS = {
    "pool_out null": (dict(pool_out=0), -6),
    "out_u8 null": (dict(out=0), -6),
    "pool_out is pool_in": (dict(alias_pool=True), -6),
    "out_u8 is counts_prev": (dict(alias_counts=True), -6),
    "tau=0": (dict(tau=0.0), -6),
    "tau<0": (dict(tau=-0.5), -6),
    "tau=nan": (dict(tau=float("nan")), -6),
    "zeta=0": (dict(zeta=0.0), -6),
    "zeta=nan": (dict(zeta=float("nan")), -6),
    "wmax<2": (dict(wmax=1.5), -6),
    "wmax=nan": (dict(wmax=float("nan")), -6),
    "rule=2": (dict(rule=2), -6),
    "rule=-1": (dict(rule=-1), -6),
    "nmax=1": (dict(n=1), -6),
    "nmax=9": (dict(n=9), -6),
    "nmax_prev=1": (dict(n_prev=1), -6),
    "nmax_prev=9": (dict(n_prev=9), -6),
    "sizes": (dict(sizes=True), -6),
    "no texture": (dict(no_texture=True), -4),   # PT_ERR_MISSING_TEXTURE
    "band": (dict(band=True), -9),               # PT_ERR_STATE
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_leave_the_outputs_untouched(gpu, case):
    import torch

    from ptsvgf._lib import PtError

    gl = gpu
    kw, code = REFUSALS[case]
    t_m, t_nd = gl.getTextureRGB32F(W, H), gl.getTextureRGB32F(W + 1 if kw.get("sizes") else W, H)
    stats = torch.zeros((H, W, 2), dtype=torch.float32, device="cuda")
    counts = torch.full((H, W), 2, dtype=torch.uint8, device="cuda")
    pool = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = Outputs(W, H)
    args = [stats.data_ptr(), out.cnt_ptr if kw.get("alias_counts") else counts.data_ptr(), kw.get("n_prev", 4),
            out.pool_ptr if kw.get("alias_pool") else pool.data_ptr(), 0xFFFFF0 if kw.get("no_texture") else t_m, t_nd,
            1.0, kw.get("wmax", 8.0), kw.get("zeta", 0.1), kw.get("rule", 0), kw.get("tau", 0.5), kw.get("n", 4),
            kw.get("pool_out", out.pool_ptr), kw.get("out", out.cnt_ptr)]
    if kw.get("band"):
        gl.set_band(W, H, 16, 64, 0, H)
    try:
        with pytest.raises(PtError) as e:
            gl.sample_counts_pool(*args)
        assert e.value.code == code, e.value
    finally:
        if kw.get("band"):
            gl.set_band(W, H, 0, H, 0, H)
    gl.sync()
    assert out.untouched()
    gl.destroy_texture(t_m)
    gl.destroy_texture(t_nd)


# --------------------------------------------------------------- 3. the closed loop ---
TAU = 1.0
POOL = 16.0
ORBIT = (1.0, 0.0)  # degrees per frame


@pytest.mark.parametrize("camera", ["still", "orbit"])
@pytest.mark.parametrize("mode,K", [("fast", 1), ("fast", 2), ("reference", 1)])
def test_closed_loop(gpu, scene_small, mode, K, camera):
    """Renderer(spp=4, adaptive=TAU, adaptive_pool=POOL) over 6 frames: every frame's count and pool planes are the
    definition's step over the slot's own previous statistics, counts and pool plane (none at the slot's first frame)
    with the frame's G-buffer; the colour and the statistics are adaptive_ref's under those counts."""
    n = 4
    gl = gpu
    rule = "absolute" if camera == "orbit" else "relative"
    r = _renderer(scene_small, spp=n, adaptive=TAU, adaptive_pool=POOL, adaptive_rule=rule, frames_in_flight=K,
                  mode=mode)
    prev = {}
    spread = set()
    for f in range(6):
        if camera == "orbit":
            r.camera.orbit(*ORBIT)
        r.camera.update()
        F = int(r.camera.frameCounter)
        assert F == (f if camera == "still" else 0)
        r.frame()
        pl = r.planes()
        fr = {k: gl.readback(pl[k]) for k in PLANES + ("normal_depth", "velocity")}
        fr.update(F=F, eye=np.array(r.camera.cam_position, f32), rot=np.array(r.cameraRotate, f32))
        counts, stats, pool = r.sample_counts(), r.sample_stats(), r.sample_pool()
        slot = f % K
        st_prev, c_prev, p_prev, f_prev = prev.get(slot, (None, None, None, f - 1))
        want_pool, want_counts = pool_step(st_prev, c_prev, n, p_prev, fr["velocity"], fr["normal_depth"],
                                           float(f - f_prev), POOL, 0.1, int(rule == "absolute"), TAU, n)
        _eq_counts(counts, want_counts, ("counts", f))
        _eq(pool, want_pool, ("pool", f))
        surf = fr["normal_depth"][..., 3] != 1.0
        if slot not in prev:
            assert np.all(counts[surf] == n) and np.all(counts[~surf] == 1) and np.all(pool[..., :3] == 0)
        else:
            spread |= set(counts[surf].tolist())
        samples = _oracle_samples("scene_small", scene_small, fr, n)[0]
        _eq(fr["color"], fold_counts(samples, counts), ("colour", f))
        _eq(stats, stats_counts(samples, counts), ("stats", f))
        prev[slot] = (stats, counts, pool, f)
    r.close()
    print("surface counts after the first draws:", sorted(spread))
    assert 1 in spread and len(spread) >= 2, spread  # surfaces reach one sample, and not all of them


# ------------------------------------------------------------- 4. the unchanged path ---
def test_unpooled_path_is_unchanged(gpu, scene_small):
    """adaptive=tau with adaptive_pool=None: the planes of a renderer built without the new arguments."""
    n = 4

    def run(**kw):
        r = _renderer(scene_small, spp=n, adaptive=TAU, **kw)
        out = []
        for f in range(4):
            if f == 3:
                r.camera.orbit(*ORBIT)
            r.camera.update()
            r.frame()
            pl = r.planes()
            fr = {k: gl.readback(pl[k]) for k in PLANES}
            fr["counts"], fr["stats"] = r.sample_counts(), r.sample_stats()
            out.append(fr)
        with pytest.raises(ValueError):
            r.sample_pool()
        r.close()
        return out

    gl = gpu
    old = run()
    new = run(adaptive_pool=None, adaptive_rule="relative", adaptive_zeta=0.1)
    for f, (a, b) in enumerate(zip(old, new)):
        assert np.array_equal(a["counts"], b["counts"]), f
        for k in PLANES + ("stats",):
            _eq(b[k], a[k], ("unchanged", f, k))
    assert np.all(old[0]["counts"] == 255) and old[1]["counts"].min() == 1 and old[1]["counts"].max() <= n


# ------------------------------------------------------------------- 5. the CLI ---
def test_render_cli_adaptive_pool_flags(gpu, scene_cornell, tmp_path, monkeypatch):
    """--adaptive-pool W --adaptive-rule R reach the renderer and an image is written; main() runs in this process on
    the session's library and scene, as in test_gpu_adaptive.py."""
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod
    from test_render_cli_spp import _pfm

    monkeypatch.setattr(scene_mod, "build_scene", lambda name: scene_cornell)
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    base = ["--width", "64", "--height", "48", "--frames", "3", "--scene", "cornell_teapot", "--view",
            "path_tracing_pic_1spp", "--spp", "4", "--adaptive", "2.0"]
    out = {}
    for name, extra in (("plain", []), ("relative", ["--adaptive-pool", "8"]),
                        ("absolute", ["--adaptive-pool", "8", "--adaptive-rule", "absolute"])):
        png, pfm = tmp_path / f"{name}.png", tmp_path / f"{name}.pfm"
        assert render_cli.main(base + ["--png", str(png), "--pfm", str(pfm)] + extra) == 0
        assert png.stat().st_size > 0
        out[name] = _pfm(str(pfm))
        assert np.isfinite(out[name]).all() and out[name].any()
    assert not np.array_equal(out["plain"], out["relative"])
    with pytest.raises(ValueError):
        render_cli.main(base[:-4] + ["--spp", "4", "--adaptive-pool", "8"])
    with pytest.raises(ValueError):
        render_cli.main(base + ["--adaptive-rule", "absolute"])

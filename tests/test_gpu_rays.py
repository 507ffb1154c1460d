"""Ray queries on the GPU (pt_rays_closest / pt_rays_occluded / pt_rays_primary, Renderer.cast_rays / occluded / pick,
render_cli --pick): every comparison is bit for bit on all eight words of a hit against tests/ray_query_ref.py run on
the buffers' host contents."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

import ray_query_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 129, 1000)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _bounds(tri_enc):
    P = tri_enc[:, :9].reshape(-1, 3)
    P = P[np.all(np.isfinite(P), axis=1)]
    return P.min(0), P.max(0)


def _rays_inside(rng, tri_enc, n, shrink=0.8):
    """n rays from inside the scene's bounds with random directions of length 0.5 .. 2 (never normalised)."""
    lo, hi = _bounds(tri_enc)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * shrink
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = c + rng.uniform(-1, 1, size=(n, 3)) * h
    r[:, 4:7] = _unit(rng, n) * rng.uniform(0.5, 2.0, size=(n, 1)).astype(np.float32)
    r[:, 7] = np.inf
    return r


def _same_bits(got, want, tag):
    g, w = R.bits(got), R.bits(want)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, (tag, bad[:5].tolist(), got[bad[:3]], want[bad[:3]])


@pytest.fixture(scope="module")
def cornell(gpu, scene_cornell):
    """The Cornell scene's buffers on the device, 1000 seeded rays of every kind in a seeded order (so every prefix
    mixes them), and the definition's hits for them, computed once."""
    rng = np.random.default_rng(20240607)
    tri = scene_cornell.tri_enc
    w = R.Walker(tri, scene_cornell.node_enc)
    lo, hi = _bounds(tri)
    a = _rays_inside(rng, tri, 400)
    z1 = _rays_inside(rng, tri, 150)                       # one exact zero component
    z1[np.arange(150), 4 + rng.integers(0, 3, 150)] = 0.0
    z2 = _rays_inside(rng, tri, 150)                       # two exact zeros: axis-parallel, either sign
    keep = rng.integers(0, 3, 150)
    for k in range(150):
        s = np.float32(rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0))
        z2[k, 4:7] = 0.0
        z2[k, 4 + keep[k]] = s
    ha = w.hits(a)
    on = ha["tri"] >= 0
    b = _rays_inside(rng, tri, 200)                        # origins that are the P of earlier hits
    b[:, 0:3] = ha["P"][on][:200] if on.sum() >= 200 else np.resize(ha["P"][on], (200, 3))
    out = _rays_inside(rng, tri, 100)                      # outside the room, pointing away
    sgn = rng.choice([-1.0, 1.0], size=(100, 3)).astype(np.float32)
    out[:, 0:3] = (lo + hi) / 2 + sgn * ((hi - lo) / 2 + rng.uniform(0.5, 3.0, size=(100, 3)).astype(np.float32))
    out[:, 4:7] = np.abs(out[:, 4:7]) * sgn
    rays = np.concatenate([a, z1, z2, b, out])[rng.permutation(1000)].astype(np.float32)
    hits = w.hits(rays)
    assert (hits["tri"] >= 0).sum() > 500 and (hits["tri"] < 0).sum() >= 100
    tt, nt = gpu.texture_buffer(tri), gpu.texture_buffer(scene_cornell.node_enc)
    yield dict(tri_tex=tt, node_tex=nt, rays=rays, hits=hits, walker=w)
    gpu.destroy_texture(tt)
    gpu.destroy_texture(nt)


# ---------------------------------------------------------------- 1. closest hits ---
@pytest.mark.parametrize("variant", (0, 1))
def test_closest_matches_the_definition(gpu, cornell, variant):
    gpu.rays_variant(variant)
    try:
        for n in SIZES:
            got = gpu.rays_closest(cornell["tri_tex"], cornell["node_tex"], cornell["rays"][:n])
            assert got.shape == (n,) and got.dtype == R.HIT_DTYPE
            _same_bits(got, cornell["hits"][:n], (variant, n))
            assert gpu.rays_state()["variant"] == variant
    finally:
        gpu.rays_variant(-1)


def test_empty_list_and_the_bytes_past_the_list(gpu, cornell):
    import torch

    from ptsvgf._lib import check, pt

    assert pt().pt_rays_closest(cornell["tri_tex"], cornell["node_tex"], None, 0, None) == 0
    assert pt().pt_rays_occluded(cornell["tri_tex"], cornell["node_tex"], None, 0, None) == 0
    assert pt().pt_rays_closest(cornell["tri_tex"], 0xFFFF, None, 0, None) == -1  # PT_ERR_INVALID_HANDLE comes first
    assert gpu.rays_closest(cornell["tri_tex"], cornell["node_tex"], np.zeros((0, 8), np.float32)).shape == (0,)
    n, extra = 129, 4
    rays = torch.from_numpy(cornell["rays"][:n]).cuda()
    out = torch.full(((n + extra) * 8,), -123.25, dtype=torch.float32, device="cuda")
    occ = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    check(pt().pt_rays_closest(cornell["tri_tex"], cornell["node_tex"], C.c_void_p(rays.data_ptr()), n,
                               C.c_void_p(out.data_ptr())))
    check(pt().pt_rays_occluded(cornell["tri_tex"], cornell["node_tex"], C.c_void_p(rays.data_ptr()), n,
                                C.c_void_p(occ.data_ptr())))
    gpu.sync()
    o = out.cpu().numpy()
    _same_bits(o[:n * 8].view(R.HIT_DTYPE), cornell["hits"][:n], "over-allocated")
    assert np.all(o[n * 8:] == np.float32(-123.25))
    oc = occ.cpu().numpy()
    assert np.all(oc[n:] == 0xAB) and set(np.unique(oc[:n]).tolist()) <= {0, 1}
    # a torch tensor goes by pointer and a tensor comes back
    t = gpu.rays_closest(cornell["tri_tex"], cornell["node_tex"], rays)
    gpu.sync()
    assert t.is_cuda and tuple(t.shape) == (n, 8)
    _same_bits(t.cpu().numpy().reshape(-1).view(R.HIT_DTYPE), cornell["hits"][:n], "tensor")


# ------------------------------------------------------------------ 2. occlusion ---
@pytest.mark.parametrize("variant", (0, 1))
def test_occlusion_is_the_closest_hit_before_tmax(gpu, cornell, variant):
    rays, hits, w = cornell["rays"], cornell["hits"], cornell["walker"]
    hit = hits["tri"] >= 0
    gpu.rays_variant(variant)
    try:
        for name, tmax, want in (
                ("any hit", np.full(1000, np.inf, np.float32), hit),
                ("tmax = t: not before it", hits["t"].copy(), np.zeros(1000, bool)),
                ("the next float after t", np.nextafter(hits["t"], np.float32(np.inf)), hit),
                ("half of t", hits["t"] * np.float32(0.5), np.zeros(1000, bool)),
                ("a large finite bound", np.full(1000, 1.0e30, np.float32), hit)):
            rr = rays.copy()
            rr[:, 7] = tmax
            assert np.array_equal(w.occluded(rr, hits), want), name  # the definition, derived from the closest hit
            for n in (65, 1000):
                got = gpu.rays_occluded(cornell["tri_tex"], cornell["node_tex"], rr[:n])
                assert got.dtype == bool and np.array_equal(got, want[:n]), (name, n, np.nonzero(got != want[:n])[0][:8])
    finally:
        gpu.rays_variant(-1)


# ------------------------------------------------------------ 3. the deep chain tree ---
def test_deep_chain_tree_spills_and_allocates_once(gpu, scene_cornell):
    from test_gpu_deep import chain_bvh

    tri = scene_cornell.tri_enc[np.random.default_rng(7).permutation(scene_cornell.ntris)]
    node = chain_bvh(tri)
    rays = _rays_inside(np.random.default_rng(3), tri, 200)
    w = R.Walker(tri, node)
    want = w.hits(rays)
    assert (want["tri"] >= 0).sum() > 100
    tt, nt = gpu.texture_buffer(tri), gpu.texture_buffer(node)
    try:
        for variant in (0, 1):
            gpu.rays_variant(variant)
            _same_bits(gpu.rays_closest(tt, nt, rays), want, ("deep", variant))
            st = gpu.rays_state()
            assert st["stack_kind"] == 2 and st["scratch_allocs"] >= 1 and st["scratch_bytes"] > 0, st
            _same_bits(gpu.rays_closest(tt, nt, rays), want, ("deep again", variant))
            assert np.array_equal(gpu.rays_occluded(tt, nt, rays), want["tri"] >= 0)
            st2 = gpu.rays_state()
            assert st2["scratch_allocs"] == st["scratch_allocs"] and st2["scratch_bytes"] == st["scratch_bytes"], (st, st2)
    finally:
        gpu.rays_variant(-1)
        gpu.destroy_texture(tt)
        gpu.destroy_texture(nt)


# -------------------------------------------------------------------- 4. exact ties ---
def test_exact_ties_take_the_references_triangle(gpu):
    """The clock plus 40 exactly coincident triangles (as test_gpu_deep builds 400): rays through the stack meet 40
    triangles at one t; `tri` is the one the reference's depth-first order meets first."""
    from ptsvgf.scene import SceneBuilder, material, transform

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    b = SceneBuilder()
    b.add_obj(os.path.join(repo, "assets", "models", "clock.obj"), material(baseColor=(0.8, 0.6, 0.3)), transform(),
              True, 0)
    n = 40
    tri = np.array([[-1.0, -0.4, 1.2], [-0.2, -0.4, 1.2], [-0.6, 0.3, 1.2]], np.float32)
    b.add_mesh(np.tile(tri, (n, 1)), np.arange(3 * n, dtype=np.int32).reshape(n, 3),
               material(baseColor=(0.3, 0.6, 0.8)), transform(), False, 1)
    b.build(8)
    t, nd, _ = b.encode()
    rng = np.random.default_rng(11)
    m = 96
    rays = np.zeros((m, 8), np.float32)
    rays[:, 0:3] = np.float32([-0.6, -0.1, 3.0]) + rng.uniform(-0.3, 0.3, size=(m, 3)).astype(np.float32)
    target = np.float32([-0.6, -0.15, 1.2]) + np.float32([0.15, 0.15, 0.0]) * rng.uniform(-1, 1, size=(m, 3)).astype(np.float32)
    rays[:, 4:7] = target - rays[:, 0:3]
    rays[:m // 3, 4:7] = np.float32([0.0, 0.0, -1.0])      # and axis-parallel ones, straight through the stack
    rays[:, 7] = np.inf
    w = R.Walker(t, nd)
    want = w.hits(rays)
    stack = (want["obj"] == 1)
    assert stack.sum() > m // 2  # most rays pass through the stack: forty triangles at one t each
    tt, nt = gpu.texture_buffer(t), gpu.texture_buffer(nd)
    try:
        for variant in (0, 1):
            gpu.rays_variant(variant)
            _same_bits(gpu.rays_closest(tt, nt, rays), want, ("ties", variant))
    finally:
        gpu.rays_variant(-1)
        gpu.destroy_texture(tt)
        gpu.destroy_texture(nt)


# ------------------------------------------------------------ 5. a device-built scene ---
def test_device_built_scene_and_a_pose(gpu, scene_small):
    from ptsvgf.renderer import Renderer

    scene = dataclasses.replace(scene_small, tri_enc=scene_small.tri_enc.copy())
    r = Renderer(scene, 32, 24, mode="fast", run_taa=False, run_output=False)
    try:
        r.rebuild_bvh()

        def built():
            t = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
            nd = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
            return t, nd

        t0, n0 = built()
        # 200 rays from around the scene, 100 from the renderer's eye at the centroids of object 1's triangles
        rng = np.random.default_rng(5)
        rays = _rays_inside(rng, t0, 300, shrink=1.2)
        own = t0[t0[:, 42] == 1.0]
        assert own.shape[0] >= 100
        cen = own[rng.choice(own.shape[0], 100, replace=False), :9].reshape(100, 3, 3).mean(axis=1)
        eye = np.asarray(r.camera.cam_position, np.float32)
        rays[200:, 0:3] = eye
        rays[200:, 4:7] = (cen - eye).astype(np.float32)
        want0 = R.Walker(t0, n0).hits(rays)
        for variant in (0, 1):
            gpu.rays_variant(variant)
            _same_bits(r.cast_rays(rays), want0, ("built", variant))
            assert np.array_equal(r.occluded(rays), want0["tri"] >= 0)
        # object 1 mirrored in x about its middle and lifted by twice its height: it leaves the volume it stood in, so
        # the rays aimed at where it stood find something else (or nothing)
        lo, hi = _bounds(own)
        M = np.eye(4, dtype=np.float32)
        M[0, 0] = -1.0
        M[0, 3] = lo[0] + hi[0]
        M[1, 3] = 2.0 * (hi[1] - lo[1])
        r.pose_objects({1: M.T.reshape(16)}, motion=False)  # glm column-major
        t1, n1 = built()
        assert not np.array_equal(t0, t1)
        want1 = R.Walker(t1, n1).hits(rays)
        changed = want0["obj"] != want1["obj"]
        print("rays whose object changed with the pose:", int(changed.sum()))
        assert changed.any()
        for variant in (0, 1):
            gpu.rays_variant(variant)
            _same_bits(r.cast_rays(rays), want1, ("posed", variant))
    finally:
        gpu.rays_variant(-1)
        r.close()


# ------------------------------------------------------------------ 6. primary rays ---
@pytest.mark.parametrize("aspect", (False, True))
def test_primary_rays_are_the_path_tracers(gpu, scene_cornell, aspect):
    from ptsvgf._lib import PtError
    from ptsvgf.camera import rigid_inverse
    from ptsvgf.renderer import Renderer

    W, H = 32, 24
    r = Renderer(scene_cornell, W, H, mode="fast", aspect_corrected=aspect, run_taa=False, run_output=False)
    try:
        r.frame()
        eye, rot = r.camera.cam_position, rigid_inverse(r.camera.cam_view_mat)
        rays = gpu.rays_primary(eye, rot, W, H, aspect)
        assert rays.shape == (W * H, 8) and np.all(rays[:, 0:3] == np.asarray(eye, np.float32))
        assert np.all(rays[:, 3] == 0.0) and np.all(np.isposinf(rays[:, 7]))
        # the restated direction agrees to the last bits of normalize
        d = np.array([R.primary_dir(rot, W, H, aspect, x, y) for y in range(H) for x in range(W)])
        assert np.abs(d - rays[:, 4:7]).max() < 4e-7
        # a list of pixels gives the same records; one outside the frame is refused on the host side
        xy = np.array([[0, 0], [31, 23], [5, 17]], np.int32)
        sub = gpu.rays_primary(eye, rot, W, H, aspect, xy)
        assert np.array_equal(sub.view(np.uint32), rays[xy[:, 1] * W + xy[:, 0]].view(np.uint32))
        with pytest.raises(PtError, match="PT_ERR_ARG"):
            gpu.rays_primary(eye, rot, W, H, aspect, np.array([[32, 0]], np.int32))
        hits = r.cast_rays(rays)
        _same_bits(hits, R.Walker(scene_cornell.tri_enc, scene_cornell.node_enc).hits(rays), "primary")
        hit = hits["tri"] >= 0
        assert hit.sum() > W * H // 4
        albedo = gpu.readback(r.planes()["albedo"]).reshape(H * W, 4)
        want = np.ascontiguousarray(scene_cornell.tri_enc[hits["tri"][hit], 21:24])
        assert np.array_equal(np.ascontiguousarray(albedo[hit][:, :3]).view(np.uint32), want.view(np.uint32))
        for k in np.nonzero(hit)[0][:: max(1, int(hit.sum()) // 5)][:5]:
            p = r.pick(int(k % W), int(k // W))
            assert p is not None and (p["obj"], p["tri"]) == (int(hits["obj"][k]), int(hits["tri"][k])), (k, p)
            assert np.float32(p["t"]) == hits["t"][k] and p["inside"] == bool(hits["inside"][k])
        miss = np.nonzero(~hit)[0]
        if miss.size:
            assert r.pick(int(miss[0] % W), int(miss[0] // W)) is None
    finally:
        r.close()


def test_pixel_outside_the_frame_on_the_device_misses(gpu, cornell):
    import torch

    eye, rot = np.zeros(3, np.float32), np.eye(4, dtype=np.float32).reshape(16)
    xy = torch.tensor([[3, 2], [-1, 0], [0, 24], [32, 5]], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rays = gpu.rays_primary(eye, rot, 32, 24, True, xy)
    hits = gpu.rays_closest(cornell["tri_tex"], cornell["node_tex"], rays)
    gpu.sync()
    rr = rays.cpu().numpy()
    assert np.all(rr[1:, 4:7] == 0.0) and np.any(rr[0, 4:7] != 0.0) and np.all(np.isposinf(rr[:, 7]))
    h = hits.cpu().numpy().reshape(-1).view(R.HIT_DTYPE)
    assert np.all(h["tri"][1:] == -1) and np.all(h["t"][1:] == R.INF)


# --------------------------------------------------------------- 7. nothing else moves ---
def test_queries_leave_the_draws_alone(gpu, scene_cornell, cornell):
    from ptsvgf.renderer import Renderer
    from ptsvgf.scene import material

    W, H = 32, 24
    probe = cornell["rays"][:1000]

    def run(query):
        scene = dataclasses.replace(scene_cornell, tri_enc=scene_cornell.tri_enc.copy())
        r = Renderer(scene, W, H, mode="fast", frames_in_flight=3, run_taa=True, run_output=False)
        picks = []
        try:
            for f in range(4):
                r.frame()
                if query:
                    picks.append(r.pick(16, 6))
                    _same_bits(r.cast_rays(probe), cornell["hits"][:1000], ("between frames", f))
            planes = {k: gpu.readback(v) for k, v in r.planes().items()}
            counts = [p.stage_counts() for p, _ in r.pt_slots] + [p.stage_counts() for p in r.init_pass]
            if query:
                before = r.pick(16, 6)
                assert before is not None and all(p == before for p in picks)
                r.set_materials({before["obj"]: material(baseColor=(0.2, 0.3, 0.9))})
                after = r.pick(16, 6)  # right after the update: the query reads the new version, the geometry stands
                assert after is not None and (after["obj"], after["tri"]) == (before["obj"], before["tri"])
                r.frame()
                assert (r.pick(16, 6)["obj"], r.pick(16, 6)["tri"]) == (before["obj"], before["tri"])
            return planes, counts
        finally:
            r.close()

    plain, c0 = run(False)
    with_q, c1 = run(True)
    assert c0 == c1, (c0, c1)
    assert sum(reuses for _, reuses in c0) > 0  # a standing view: the static-view caches were in use
    for k in plain:
        assert np.array_equal(plain[k].view(np.uint32), with_q[k].view(np.uint32)), k


# ------------------------------------------------------------------- 8. the CLI ---
def test_render_cli_pick(gpu, scene_cornell, tmp_path, monkeypatch, capsys):
    """--pick prints one JSON line per flag, the line Renderer.pick gives. main() runs in this process on the
    session's library and scene, as in test_render_cli_spp.py."""
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod
    from ptsvgf.renderer import Renderer

    monkeypatch.setattr(scene_mod, "build_scene", lambda name: scene_cornell)
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    W, H = 32, 24
    r = Renderer(scene_cornell, W, H, run_taa=True, run_output=True)
    try:
        r.frame()
        want = [r.pick(16, 6), r.pick(0, 23)]
    finally:
        r.close()
    assert want[0] is not None
    capsys.readouterr()
    args = ["--width", str(W), "--height", str(H), "--frames", "1", "--scene", "cornell_teapot", "--png",
            str(tmp_path / "p.png"), "--pick", "16,6", "--pick", "0,23"]
    assert render_cli.main(args) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [set(ln) for ln in lines] == [{"pick"}, {"pick"}]
    assert [ln["pick"] for ln in lines] == want
    assert set(want[0]) == {"obj", "tri", "t", "point", "inside"}
    with pytest.raises(SystemExit):
        render_cli.main(["--width", str(W), "--height", str(H), "--frames", "1", "--pick", "32,0"])

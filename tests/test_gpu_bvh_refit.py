"""BVH refit on the device (pt_bvh_refit, pt_raster_pass_refit_device, Renderer.refit_bvh; csrc/kernels_bvh.hip
refit_nodes) for geometry that moves but keeps its triangles and their order.

* The refitted buffers equal the definition (tests/lbvh_refit_ref.py) bit for bit: the triangles permuted by the
  build's leaf order, the topology texels untouched, every box the fold in the written operand order, on tiny,
  multi-block, flat-axis and NaN inputs, as a plain LBVH and under a PLOC top; unmoved geometry gives the build back,
  and so does moving there and back (the kept state and the arrival counters are reused).
* The walk trees derived after a refit equal the host functions on the refitted texels.
* Rendering over refitted buffers is bit-exact against the oracle path tracer on the same buffers; the refitted
  G-buffer pass draws the planes of a host bind to the moved list, and the motion vectors of a rebuild.
* Argument and state errors return before any launch and leave buffers and passes as they were.
* A build, a refit and a pose write the same bytes with and without out_ms, and report a time above zero."""
import dataclasses

import numpy as np
import pytest

import lbvh_refit_ref as R
import lbvh_trees_ref as T
import oracle_ref as O

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _random_tris(n, seed=0, flat_axis=None):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 45), np.float32)
    t[:, :9] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    if flat_axis is not None:
        t[:, flat_axis:9:3] = 0.5
    t[:, 42] = np.arange(n)
    return t


def _displaced(t, seed):
    rng = np.random.default_rng(seed)
    out = t.copy()
    out[:, :9] += rng.uniform(-0.3, 0.3, (t.shape[0], 9)).astype(np.float32)  # every vertex by its own vector
    out[:, 9:12] = rng.uniform(0, 1, (t.shape[0], 3)).astype(np.float32)  # any other field may differ too
    return out


class _Built:
    """A pt_bvh_build pair and what the tests read from it; `with` destroys the handles."""

    def __init__(self, gl, tri, leaf_n, ploc):
        self.gl, self.tri = gl, tri
        self.to = gl.texture_buffer(np.zeros(3, np.float32))
        self.no = gl.texture_buffer(np.zeros(3, np.float32))
        self.extra = []
        src = gl.texture_buffer(tri)
        try:
            gl.bvh_build(src, self.to, self.no, leaf_n, ploc)
        finally:
            gl.destroy_texture(src)
        self.tri_out, self.nodes = self.read()
        # the build's permutation, checked before anything relies on it
        self.order = gl.lbvh_order(self.no)
        assert np.array_equal(np.sort(self.order), np.arange(len(tri)))
        assert _same(tri[self.order], self.tri_out)

    def read(self):
        return self.gl.buffer_readback(self.to).reshape(-1, 45), self.gl.buffer_readback(self.no).reshape(-1, 12)

    def refit(self, tri):
        src = self.gl.texture_buffer(tri)
        try:
            return self.gl.bvh_refit(src, self.to, self.no)
        finally:
            self.gl.destroy_texture(src)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for h in [self.to, self.no] + self.extra:
            self.gl.destroy_texture(h)


def _check_refit(b, tri_new):
    want_tri, want_nodes = R.refit(tri_new, b.order, b.nodes)
    got_tri, got_nodes = b.read()
    assert _same(got_tri, want_tri)
    assert _same(got_nodes[:, :6], b.nodes[:, :6])  # childs and leafInfo: untouched
    assert _same(got_nodes[0], b.nodes[0])          # the dummy node
    assert _same(got_nodes, want_nodes)
    return got_tri, got_nodes


@pytest.mark.parametrize("ploc", [0, 16])
@pytest.mark.parametrize("leaf_n", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 1000, 20000])
def test_refit_equals_the_restatement(gpu, n, leaf_n, ploc):
    """n = 1: the root is a leaf (no climb); n = 2: the first climb; 1000 and 20000: several blocks."""
    t = _random_tris(n, seed=n + 7)
    with _Built(gpu, t, leaf_n, ploc) as b:
        moved = _displaced(t, seed=n)
        ms = b.refit(moved)
        _, nodes = _check_refit(b, moved)
        if n > 1:
            assert not np.array_equal(nodes[1:, 6:], b.nodes[1:, 6:])
        print(f"n {n} leaf_n {leaf_n} ploc {ploc}: {len(nodes)} nodes, refit {ms:.3f} ms")


def test_refit_flat_axis_equals_the_restatement(gpu):
    t = _random_tris(1000, seed=5, flat_axis=2)
    with _Built(gpu, t, 4, 16) as b:
        moved = _displaced(t, seed=2)
        moved[:, 2:9:3] = 0.25  # still flat, elsewhere
        b.refit(moved)
        _check_refit(b, moved)


@pytest.mark.parametrize("ploc", [0, 16])
def test_refit_nan_vertices_equal_the_restatement(gpu, ploc):
    """NaN positions in a few triangles of the new list: the fold's operand order decides what a box keeps, the
    device equals the definition bit for bit, and the climb ends."""
    t = _random_tris(300, seed=9)
    with _Built(gpu, t, 4, ploc) as b:
        moved = _displaced(t, seed=4)
        moved[[5, 77, 150], 0] = np.nan
        moved[[77, 201], 7] = np.nan
        # glm's min / max drop a NaN second operand: one that has to stay is p1 of the first triangle of a leaf
        leaf = b.nodes[1:][b.nodes[1:, 3] > 0][3]
        moved[b.order[int(leaf[4])], 0] = np.nan
        b.refit(moved)
        _, nodes = _check_refit(b, moved)
        assert np.isnan(nodes[1:, 6:]).any()


@pytest.mark.parametrize("leaf_n,ploc", [(4, 0), (3, 32)])
def test_refit_unmoved_and_there_and_back(gpu, leaf_n, ploc):
    t = _random_tris(1000, seed=11)
    with _Built(gpu, t, leaf_n, ploc) as b:
        b.refit(t)  # the build's own input
        tri, nodes = b.read()
        assert _same(tri, b.tri_out)
        assert _same(nodes[:, :6], b.nodes[:, :6])
        assert np.array_equal(nodes[:, 6:], b.nodes[:, 6:])  # as values: only the sign of a zero may differ
        moved = _displaced(t, seed=1)
        b.refit(moved)
        _check_refit(b, moved)
        b.refit(t)
        tri, nodes = _check_refit(b, t)
        assert _same(tri, b.tri_out)
        assert np.array_equal(nodes[:, 6:], b.nodes[:, 6:])


@pytest.mark.parametrize("n,leaf_n,ploc", [(1, 4, 0), (2, 1, 0), (1000, 4, 16), (20000, 3, 32)])
def test_trees_derived_after_a_refit(gpu, n, leaf_n, ploc):
    """pt_debug_lbvh_trees: the device stage's buffers (source 0) equal the host functions run on the host mirror of
    the refitted texels (source 1), which has to read as the refit contents, and the restatement."""
    t = _random_tris(n, seed=n + 3)
    with _Built(gpu, t, leaf_n, ploc) as b:
        before = gpu.lbvh_trees(b.no, 0)
        b.refit(_displaced(t, seed=n + 1))
        dev, host = gpu.lbvh_trees(b.no, 0), gpu.lbvh_trees(b.no, 1)
        want = T.trees(b.read()[1])
        for name in ("binary", "leaves", "wide"):
            assert _same(dev[name], host[name]), name
            assert _same(dev[name], want[name]), name
        assert dev["info"][:7] == host["info"][:7] == want["info"][:7]
        assert not _same(before["leaves"], dev["leaves"])


def _plant(scene):
    n_plant = int(np.sum(scene.tri_enc[:, 42] == 2.0))
    assert 0 < n_plant < scene.ntris
    return slice(scene.raster.size // 18 - n_plant, None)  # the last object emitted


def _moved_tri(scene, dy):
    """The plant (objIndex 2) lifted by dy: Triangle_encoded positions."""
    tri = scene.tri_enc.copy()
    sel = tri[:, 42] == 2.0
    for v in range(3):
        tri[sel, 3 * v + 1] += np.float32(dy)
    return tri


def _moved_raster(scene, dy):
    v = scene.raster.reshape(-1, 3, 6).copy()
    v[_plant(scene), :, 1] += np.float32(dy)
    return v.reshape(-1)


@pytest.mark.parametrize("lbvh_wide", [1, 0])
def test_render_over_refitted_buffers_matches_oracle(gpu, scene_small, lbvh_wide):
    """Against the oracle on the same (refitted) buffers, not a render over a fresh rebuild: exact-t ties depend on
    the tree."""
    from ptsvgf.renderer import Renderer

    W, H = 96, 64
    r = Renderer(scene_small, W, H, mode="fast", frames_in_flight=2, run_taa=False, run_output=False)
    nodes0, _ = r.rebuild_bvh(leaf_n=8, ploc_radius=16)
    r.set_lbvh_wide(bool(lbvh_wide))
    r.frame()
    old_nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    order = gpu.lbvh_order(r.nodesTextureBuffer)
    moved = _moved_tri(scene_small, 0.05)
    ms = r.refit_bvh(moved)
    assert ms > 0.0
    tri = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    assert len(nodes) == nodes0
    want_tri, want_nodes = R.refit(moved, order, old_nodes)
    assert _same(tri, want_tri) and _same(nodes, want_nodes)
    assert not _same(nodes, old_nodes)
    ref = O.OracleFrameLoop(dataclasses.replace(scene_small, tri_enc=tri, node_enc=nodes), W, H, run_taa=False)
    ref.frame()  # the oracle reaches the renderer's frame counter (static camera)
    r.frame()
    want = ref.frame()
    got = {k: gpu.readback(v) for k, v in r.planes().items()}
    r.close()
    for key in ("color", "emission", "albedo"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key


GBUF = ("normal_depth", "velocity", "fwidth", "world")


def _gbuf(gpu, r):
    got = r.planes()
    return {k: gpu.readback(got[k]) for k in GBUF}


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_refitted_gbuffer_equals_host_bind_and_rebuild_motion(gpu, scene_small, gbuffer_mode):
    from ptsvgf.renderer import Renderer

    W, H = 160, 96
    old = scene_small.raster
    tri, moved = _moved_tri(scene_small, 0.05), _moved_raster(scene_small, 0.05)

    def renderer(scene):
        r = Renderer(scene, W, H, mode="fast", run_taa=False, run_output=False)
        for p in r.init_pass:
            p.set_uniform_int("gbuffer_mode", gbuffer_mode)
        return r

    r = renderer(scene_small)
    r.rebuild_bvh(raster=old, leaf_n=8, ploc_radius=16)
    r.frame()
    before = _gbuf(gpu, r)
    r.refit_bvh(tri, raster=moved)
    r.frame()
    refit_plain = _gbuf(gpu, r)
    r.refit_bvh(tri, raster=moved, prev_raster=old)
    r.frame()
    refit_motion = _gbuf(gpu, r)
    r.frame()  # the frame after: object_motion = 0 again
    refit_after = _gbuf(gpu, r)
    r.close()

    h = renderer(dataclasses.replace(scene_small, raster=moved))  # bound on the host to the moved list
    h.frame()
    host_plain = _gbuf(gpu, h)
    h.rebuild_bvh(tri_enc=tri, raster=moved, leaf_n=8, ploc_radius=16, prev_raster=old)
    h.frame()
    rebuild_motion = _gbuf(gpu, h)
    h.close()

    for k in GBUF:
        assert np.array_equal(_bits(refit_plain[k]), _bits(host_plain[k])), k
        assert np.array_equal(_bits(refit_motion[k]), _bits(rebuild_motion[k])), k
        assert np.array_equal(_bits(refit_after[k]), _bits(host_plain[k])), k
    assert not np.array_equal(_bits(before["world"]), _bits(refit_plain["world"]))  # the plant moved in the image
    assert not np.array_equal(_bits(refit_motion["velocity"]), _bits(refit_plain["velocity"]))
    assert 0.05 < float(np.mean(host_plain["normal_depth"][..., 3] != 1.0)) < 0.95


def test_refit_errors_leave_the_buffers_unchanged(gpu):
    from ptsvgf._lib import PtError

    t = _random_tris(100, seed=2)
    moved = _displaced(t, seed=3)
    with _Built(gpu, t, 4, 16) as b:
        src = gpu.texture_buffer(moved)
        b.extra.append(src)

        def refused(code, tri_in, tri_out, node_out, pair=(b.to, b.no), want=(b.tri_out, b.nodes)):
            with pytest.raises(PtError) as e:
                gpu.bvh_refit(tri_in, tri_out, node_out)
            assert e.value.code == code, str(e.value)
            assert _same(gpu.buffer_readback(pair[0]).reshape(-1, 45), want[0])
            assert _same(gpu.buffer_readback(pair[1]).reshape(-1, 12), want[1])

        # buffers a host upload wrote (the very contents of a build)
        up_t, up_n = gpu.texture_buffer(b.tri_out), gpu.texture_buffer(b.nodes)
        b.extra += [up_t, up_n]
        refused(-9, src, up_t, up_n, pair=(up_t, up_n))
        refused(-9, src, up_t, b.no)  # not a pair
        refused(-9, src, b.to, up_n)
        # a triangle count off by one, either way; records that are not whole
        for rows in (moved[:-1], np.concatenate([moved, moved[:1]])):
            bad = gpu.texture_buffer(rows)
            b.extra.append(bad)
            refused(-6, bad, b.to, b.no)
        bad = gpu.texture_buffer(moved.reshape(-1)[:-3])
        b.extra.append(bad)
        refused(-6, bad, b.to, b.no)
        # a repeated handle
        refused(-6, src, b.to, b.to)
        refused(-6, src, src, b.no)
        refused(-6, b.no, b.to, b.no)
        # the pair still refits, and its trees are the old pair's until then
        assert gpu.lbvh_trees(b.no, 0)["info"][:7] == gpu.lbvh_trees(b.no, 1)["info"][:7]
        b.refit(moved)
        _check_refit(b, moved)
        # tri_out written by another build since: neither node buffer is its pair with the old version
        refitted = b.read()
        no2 = gpu.texture_buffer(np.zeros(3, np.float32))
        b.extra.append(no2)
        s2 = gpu.texture_buffer(t)
        b.extra.append(s2)
        gpu.bvh_build(s2, b.to, no2, 4, 0)
        rebuilt = gpu.buffer_readback(b.to).reshape(-1, 45), refitted[1]
        refused(-9, src, b.to, b.no, want=rebuilt)
        gpu.bvh_refit(src, b.to, no2)  # the new pair is one


def test_out_ms_is_optional_and_changes_nothing(gpu):
    """pt_bvh_build, pt_bvh_refit and pt_pose_apply (two objects over the same list), each called without and with
    out_ms: both calls leave byte-identical triangle and node buffers and the same counters of the derived trees (the
    first seven info words of pt_debug_lbvh_trees; the eighth is the stage's measured time), and the time reported is
    finite and above zero. The timed calls read their events after the call's own synchronisation."""
    import ctypes as C

    from ptsvgf._lib import check, pt
    from ptsvgf.scene import transform

    t = _random_tris(100, seed=2)
    t[:, 42] = np.arange(100) % 2
    mats = np.ascontiguousarray(np.stack([transform(), transform(rot=(10, 40, -20), trans=(0.3, -0.1, 0.2))]),
                                np.float32).reshape(-1, 16)
    src, moved = gpu.texture_buffer(t), gpu.texture_buffer(_displaced(t, seed=3))
    to, no = gpu.texture_buffer(np.zeros(3, np.float32)), gpu.texture_buffer(np.zeros(3, np.float32))
    poses = []

    def state():
        return (gpu.buffer_readback(to).tobytes(), gpu.buffer_readback(no).tobytes(), gpu.lbvh_trees(no, 0)["info"][:7])

    def without_and_with(call):
        check(call(None))
        plain = state()
        ms = C.c_float(-1.0)
        check(call(C.byref(ms)))
        assert state() == plain
        assert np.isfinite(ms.value) and ms.value > 0.0, ms.value

    try:
        without_and_with(lambda ms: pt().pt_bvh_build(src, 4, 16, to, no, None, ms))
        assert len(gpu.buffer_readback(to)) == t.size
        without_and_with(lambda ms: pt().pt_bvh_refit(moved, to, no, ms))
        poses.append(gpu.pose_create(src))
        mp = mats.ctypes.data_as(C.POINTER(C.c_float))
        without_and_with(lambda ms: pt().pt_pose_apply(poses[0], mp, 2, to, no, 0, 1, ms))
    finally:
        for p in poses:
            gpu.pose_destroy(p)
        for h in (src, moved, to, no):
            gpu.destroy_texture(h)


def test_raster_refit_errors_leave_the_pass_drawing(gpu, scene_small):
    """A host-bound pass (PT_ERR_STATE: bind again), a sharing pass and another triangle count (PT_ERR_ARG): the
    passes draw what they drew before."""
    import torch

    from ptsvgf._lib import PtError
    from ptsvgf.renderer import Renderer

    W, H = 96, 64
    r = Renderer(scene_small, W, H, mode="fast", run_taa=False, run_output=False)
    v = torch.from_numpy(_moved_raster(scene_small, 0.05)).cuda()
    torch.cuda.synchronize()
    want = []
    for _ in range(2):
        r.frame()
        want.append(_gbuf(gpu, r))
    with pytest.raises(PtError) as e:  # bound on the host by the constructor
        r.init_pass[0].refit_vertices_device(v.data_ptr(), v.numel())
    assert e.value.code == -9
    with pytest.raises(PtError) as e:  # the scene buffers are the host-built ones
        r.refit_bvh(_moved_tri(scene_small, 0.05))
    assert e.value.code == -9 and "rebuild_bvh" in str(e.value)
    r.rebuild_bvh(raster=scene_small.raster, leaf_n=8, ploc_radius=16)  # init_pass[1] now shares init_pass[0]
    for p, size in ((r.init_pass[1], v.numel()), (r.init_pass[0], v.numel() - 18), (r.init_pass[0], v.numel() + 18)):
        with pytest.raises(PtError) as e:
            p.refit_vertices_device(v.data_ptr(), size)
        assert e.value.code == -6
    for k in range(2):
        r.frame()
        got = _gbuf(gpu, r)
        for key in GBUF:
            assert np.array_equal(_bits(got[key]), _bits(want[k][key])), (k, key)
    r.close()

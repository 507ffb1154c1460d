"""Objects posed by matrix on the device (pt_pose_create / pt_pose_apply, Renderer.pose_objects; csrc/kernels_bvh.hip
pose_tris, pose_raster).

* The refitted buffers equal the definitions bit for bit: tests/pose_ref.py for the posed records, then
  tests/lbvh_refit_ref.py for the refit over them, on a single leaf, less than a wave, less than a block and many
  blocks, as a plain LBVH and under a PLOC top, with records that name no object; the walk trees derived after it
  equal the host functions on the refreshed mirror.
* Matrices are absolute: identities give pt_bvh_refit of the rest buffer, and a pose followed by identities gives
  that again, with the rest raster list current.
* The posed raster lists alternate: G-buffer planes and motion vectors equal those of a renderer driven through
  refit_bvh with the host arrays the definition produces.
* Rendering over posed buffers is bit-exact against the oracle path tracer on the same buffers.
* Every error returns before the first launch and leaves buffers, trees and planes as they were.

Comparisons are bitwise through a uint32 view wherever the restatement is not NaN, and NaN wherever it is."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import lbvh_refit_ref as R
import oracle_ref as O
import pose_ref as P

pytestmark = pytest.mark.gpu

GBUF = ("normal_depth", "velocity", "fwidth", "world")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Bit for bit where the restatement b is not NaN, NaN where it is."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(b)
    return bool(np.array_equal(_bits(a)[~nan], _bits(b)[~nan]) and np.all(np.isnan(a[nan])))


def _mats():
    """Object 0 keeps the identity, 1 gets a similarity, 2 a rotation with a non-uniform scale."""
    from ptsvgf.scene import transform

    return np.stack([transform(),
                     transform(rot=(10, 40, -20), trans=(0.3, -0.1, 0.2), scale=(1.25, 1.25, 1.25)),
                     transform(rot=(25, -15, 60), trans=(-0.2, 0.1, 0.05), scale=(1, 0.5, 2))])


def _rest_tris(n, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 45), np.float32)
    t[:, :9] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    t[:, 9:18] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)  # normals of any length: the pose normalises
    t[:, 18:42] = rng.uniform(0, 1, (n, 24)).astype(np.float32)
    t[:, 42] = (np.arange(n) + 1) % 3  # n = 1: object 1, which moves
    if n >= 17:
        t[3, 42], t[5, 42], t[11, 42], t[13, 42] = 7.0, -1.0, 2.5, np.nan  # records of no object
        t[7, 12:15] = 0.0  # a zero normal: NaN once posed (object 2)
    return t


def _rest_raster(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, n * 18).astype(np.float32)
    obj = (np.arange(n) % 3).astype(np.int32)
    if n >= 17:
        obj[[2, 9]] = 7, -1
    return v, obj


class _Built:
    """A pt_bvh_build pair over `tri`, a pose over the same rows, and what the tests read; `with` destroys them."""

    def __init__(self, gl, tri, leaf_n, ploc, raster=None, raster_obj=None):
        self.gl, self.tri = gl, tri
        self.to = gl.texture_buffer(np.zeros(3, np.float32))
        self.no = gl.texture_buffer(np.zeros(3, np.float32))
        self.extra, self.poses = [], []
        src = gl.texture_buffer(tri)
        try:
            gl.bvh_build(src, self.to, self.no, leaf_n, ploc)
            self.pose = gl.pose_create(src, raster, raster_obj)  # src may go afterwards
            self.poses.append(self.pose)
        finally:
            gl.destroy_texture(src)
        self.tri_out, self.nodes = self.read()
        self.order = gl.lbvh_order(self.no)
        assert np.array_equal(np.sort(self.order), np.arange(len(tri)))

    def read(self):
        return self.gl.buffer_readback(self.to).reshape(-1, 45), self.gl.buffer_readback(self.no).reshape(-1, 12)

    def apply(self, mats, **kw):
        return self.gl.pose_apply(self.pose, mats, self.to, self.no, **kw)

    def check(self, mats):
        want_tri, want_nodes = R.refit(P.tris(self.tri, mats), self.order, self.nodes)
        got_tri, got_nodes = self.read()
        assert _same(got_tri, want_tri)
        assert np.array_equal(_bits(got_nodes[:, :6]), _bits(self.nodes[:, :6]))  # childs and leafInfo: untouched
        assert _same(got_nodes, want_nodes)
        return got_tri, got_nodes

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.poses:
            self.gl.pose_destroy(p)
        for h in [self.to, self.no] + self.extra:
            self.gl.destroy_texture(h)


@pytest.mark.parametrize("ploc", [0, 16])
@pytest.mark.parametrize("leaf_n", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 17, 1000, 20000])
def test_posed_buffers_equal_the_restatement(gpu, n, leaf_n, ploc):
    """n = 1: the root is a leaf; 2 and 17: less than a wave of texels per record group, less than a block; 1000 and
    20000: many blocks. One call poses by all three matrices (objIndex (i + 1) % 3)."""
    t = _rest_tris(n, seed=n + 5)
    mats = _mats()
    with _Built(gpu, t, leaf_n, ploc) as b:
        ms = b.apply(mats)
        assert ms > 0.0
        tri, nodes = b.check(mats)
        moved = P.objects_of(tri[:, 42], 3) > 0
        assert moved.any() and not np.array_equal(_bits(tri[moved, :18]), _bits(b.tri_out[moved, :18]))
        if n >= 17:
            assert np.isnan(tri[:, 9:18]).any() and not np.isnan(tri[:, :9]).any()
        dev, host = gpu.lbvh_trees(b.no, 0), gpu.lbvh_trees(b.no, 1)
        for name in ("binary", "leaves", "wide"):
            assert np.array_equal(_bits(dev[name]), _bits(host[name])), name
        assert dev["info"][:7] == host["info"][:7]
        print(f"n {n} leaf_n {leaf_n} ploc {ploc}: {len(nodes)} nodes, pose {ms:.3f} ms")


def test_identity_and_absolute_matrices(gpu):
    n = 1000
    t = _rest_tris(n, seed=21)
    rv, ro = _rest_raster(300, seed=22)
    mats, ident = _mats(), np.tile(P.IDENTITY, (3, 1))
    with _Built(gpu, t, 4, 16, rv, ro) as b:
        assert np.array_equal(_bits(gpu.pose_raster(b.pose, 0)), _bits(rv))
        b.apply(ident)
        a_tri, a_nodes = b.read()
        src = gpu.texture_buffer(t)
        b.extra.append(src)
        gpu.bvh_refit(src, b.to, b.no)  # the same pair, refitted with the rest rows
        r_tri, r_nodes = b.read()
        assert np.array_equal(_bits(a_tri), _bits(r_tri)) and np.array_equal(_bits(a_nodes), _bits(r_nodes))
        assert np.array_equal(_bits(a_tri), _bits(b.tri_out))
        b.apply(mats)
        b.check(mats)
        posed = P.raster(rv, ro, mats)
        assert _same(gpu.pose_raster(b.pose, 0), posed) and not _same(posed, rv)
        assert np.array_equal(_bits(gpu.pose_raster(b.pose, 1)), _bits(rv))
        b.apply(ident)
        tri, nodes = b.read()
        assert np.array_equal(_bits(tri), _bits(a_tri)) and np.array_equal(_bits(nodes), _bits(a_nodes))
        assert np.array_equal(_bits(gpu.pose_raster(b.pose, 0)), _bits(rv))
        assert _same(gpu.pose_raster(b.pose, 1), posed)


def _gbuf(gpu, r):
    got = r.planes()
    return {k: gpu.readback(got[k]) for k in GBUF}


def _moves():
    from ptsvgf.scene import transform

    return transform(trans=(0, 0.05, 0)), transform(rot=(0, 5, 0), trans=(0, 0.05, 0))


def _renderer(scene, W, H, gbuffer_mode=None, **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, W, H, mode="fast", run_taa=False, run_output=False, **kw)
    if gbuffer_mode is not None:
        for p in r.init_pass:
            p.set_uniform_int("gbuffer_mode", gbuffer_mode)
    return r


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_posed_raster_lists_alternate(gpu, scene_small, gbuffer_mode):
    """Two poses and a frame after, against a renderer driven through refit_bvh with the definition's host arrays:
    previous list = rest for the first move, the first posed list for the second, no motion on the frame after."""
    W, H = 160, 96
    s = scene_small
    m_a, m_b = _moves()
    tabs = [P.table({2: m}, 3) for m in (m_a, m_b)]
    lists = [P.raster(s.raster, s.raster_obj, tab) for tab in tabs]
    assert not np.array_equal(_bits(lists[0]), _bits(s.raster)) and not np.array_equal(_bits(lists[0]), _bits(lists[1]))

    r = _renderer(s, W, H, gbuffer_mode)
    r.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    got = []
    assert r.pose_objects({2: m_a}) > 0.0
    assert _same(gpu.pose_raster(r._pose, 0), lists[0])
    assert np.array_equal(_bits(gpu.pose_raster(r._pose, 1)), _bits(s.raster))
    r.frame()
    got.append(_gbuf(gpu, r))
    r.pose_objects({2: m_b})
    assert _same(gpu.pose_raster(r._pose, 0), lists[1]) and _same(gpu.pose_raster(r._pose, 1), lists[0])
    r.frame()
    got.append(_gbuf(gpu, r))
    r.frame()  # the frame after: object_motion = 0 again
    got.append(_gbuf(gpu, r))
    r.pose_objects({2: m_b}, motion=False)  # the same pose without records
    r.frame()
    plain = _gbuf(gpu, r)
    r.close()

    h = _renderer(s, W, H, gbuffer_mode)
    h.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    want = []
    h.refit_bvh(P.tris(s.tri_enc, tabs[0]), raster=lists[0], prev_raster=s.raster)
    h.frame()
    want.append(_gbuf(gpu, h))
    h.refit_bvh(P.tris(s.tri_enc, tabs[1]), raster=lists[1], prev_raster=lists[0])
    h.frame()
    want.append(_gbuf(gpu, h))
    h.frame()
    want.append(_gbuf(gpu, h))
    h.close()

    for f in range(3):
        for k in GBUF:
            assert np.array_equal(_bits(got[f][k]), _bits(want[f][k])), (f, k)
    for k in GBUF:
        assert np.array_equal(_bits(plain[k]), _bits(got[2][k])), k
    assert not np.array_equal(_bits(got[1]["velocity"]), _bits(plain["velocity"]))  # the records did something
    assert not np.array_equal(_bits(got[0]["world"]), _bits(got[1]["world"]))        # and the plant moved again
    assert 0.05 < float(np.mean(got[2]["normal_depth"][..., 3] != 1.0)) < 0.95


@pytest.mark.parametrize("lbvh_wide", [1, 0])
def test_render_over_posed_buffers_matches_oracle(gpu, scene_small, lbvh_wide):
    """Against the oracle on the same (posed, refitted) buffers; without a raster list only the path tracer's tree
    is posed."""
    W, H = 96, 64
    s = scene_small
    m_a, _ = _moves()
    r = _renderer(s, W, H, frames_in_flight=2)
    nodes0, _ = r.rebuild_bvh(leaf_n=8, ploc_radius=16)
    r.set_lbvh_wide(bool(lbvh_wide))
    r.frame()
    old_nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    order = gpu.lbvh_order(r.nodesTextureBuffer)
    assert r.pose_objects({2: m_a}) > 0.0
    tri = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    assert len(nodes) == nodes0
    want_tri, want_nodes = R.refit(P.tris(s.tri_enc, P.table({2: m_a}, 3)), order, old_nodes)
    assert _same(tri, want_tri) and _same(nodes, want_nodes)
    assert not np.array_equal(_bits(nodes), _bits(old_nodes))
    ref = O.OracleFrameLoop(dataclasses.replace(s, tri_enc=tri, node_enc=nodes), W, H, run_taa=False)
    ref.frame()  # the oracle reaches the renderer's frame counter (static camera)
    r.frame()
    want = ref.frame()
    got = {k: gpu.readback(v) for k, v in r.planes().items()}
    r.close()
    for key in ("color", "emission", "albedo"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), key


def test_pose_errors_leave_the_buffers_unchanged(gpu):
    from ptsvgf._lib import PtError, fptr, pt

    t = _rest_tris(100, seed=31)
    rv, ro = _rest_raster(100, seed=32)
    mats = _mats()
    with _Built(gpu, t, 4, 16, rv, ro) as b:
        src = gpu.texture_buffer(t)
        b.extra.append(src)
        bare = gpu.pose_create(src)  # no raster list
        b.poses.append(bare)
        trees0 = gpu.lbvh_trees(b.no, 0)

        def refused(code, call, pair=(b.to, b.no), want=(b.tri_out, b.nodes)):
            with pytest.raises(PtError) as e:
                call()
            assert e.value.code == code, str(e.value)
            assert np.array_equal(_bits(gpu.buffer_readback(pair[0]).reshape(-1, 45)), _bits(want[0]))
            assert np.array_equal(_bits(gpu.buffer_readback(pair[1]).reshape(-1, 12)), _bits(want[1]))
            assert np.array_equal(_bits(gpu.pose_raster(b.pose, 0)), _bits(rv))  # nothing became current

        def raw(pose, mats16, n_obj, to, no, rpass=0):
            ms = C.c_float()
            rc = pt().pt_pose_apply(pose, mats16, n_obj, to, no, rpass, 1, C.byref(ms))
            if rc < 0:
                raise PtError(rc, (pt().pt_last_error() or b"").decode())

        m = np.ascontiguousarray(mats, np.float32)
        refused(-6, lambda: raw(b.pose, fptr(m), 0, b.to, b.no))
        refused(-6, lambda: b.apply(np.tile(P.IDENTITY, (4097, 1))))
        refused(-6, lambda: raw(b.pose, None, 3, b.to, b.no))
        refused(-6, lambda: raw(bare, fptr(m), 3, b.to, b.no, rpass=12345))  # a pass for a pose without a raster list
        refused(-6, lambda: gpu.pose_apply(b.pose, mats, b.to, b.to))        # a handle used twice
        refused(-1, lambda: gpu.pose_apply(987654, mats, b.to, b.no))        # never a pose
        # buffers a host upload wrote (the very contents of the build): not a pair
        up_t, up_n = gpu.texture_buffer(b.tri_out), gpu.texture_buffer(b.nodes)
        b.extra += [up_t, up_n]
        refused(-9, lambda: gpu.pose_apply(b.pose, mats, up_t, up_n), pair=(up_t, up_n))
        refused(-9, lambda: gpu.pose_apply(b.pose, mats, up_t, b.no))
        # a pair of another triangle count
        with _Built(gpu, _rest_tris(64, seed=33), 4, 0) as other:
            refused(-6, lambda: gpu.pose_apply(b.pose, mats, other.to, other.no), pair=(other.to, other.no),
                    want=(other.tri_out, other.nodes))
        trees1 = gpu.lbvh_trees(b.no, 0)
        for name in ("binary", "leaves", "wide"):
            assert np.array_equal(_bits(trees0[name]), _bits(trees1[name])), name
        # a following valid pose still works, with either pose
        b.apply(mats)
        b.check(mats)
        gpu.pose_apply(bare, np.tile(P.IDENTITY, (3, 1)), b.to, b.no)
        b.check(np.tile(P.IDENTITY, (3, 1)))
        # tri_out written by another build since: the old pair is none
        posed = b.read()
        no2 = gpu.texture_buffer(np.zeros(3, np.float32))
        b.extra.append(no2)
        gpu.bvh_build(src, b.to, no2, 4, 0)
        rebuilt = gpu.buffer_readback(b.to).reshape(-1, 45), posed[1]
        with pytest.raises(PtError) as e:
            gpu.pose_apply(b.pose, mats, b.to, b.no)
        assert e.value.code == -9
        assert np.array_equal(_bits(gpu.buffer_readback(b.to).reshape(-1, 45)), _bits(rebuilt[0]))
        assert np.array_equal(_bits(gpu.buffer_readback(b.no).reshape(-1, 12)), _bits(rebuilt[1]))
        # use after destroy
        gpu.pose_destroy(bare)
        b.poses.remove(bare)
        with pytest.raises(PtError) as e:
            gpu.pose_apply(bare, mats, b.to, no2)
        assert e.value.code == -1
        with pytest.raises(PtError) as e:
            gpu.pose_destroy(bare)
        assert e.value.code == -1


def test_pose_objects_errors_leave_the_renderer_drawing(gpu, scene_small):
    """Before any rebuild_bvh (refit_bvh's PT_ERR_STATE text), after a refit_bvh, and a table too large for the
    library, with the G-buffer pass given: the planes, the scene buffers and the pose are as before."""
    from ptsvgf._lib import PtError

    W, H = 96, 64
    s = scene_small
    m_a, m_b = _moves()
    r = _renderer(s, W, H)
    r.frame()
    before = _gbuf(gpu, r)
    with pytest.raises(PtError) as e:
        r.pose_objects({2: m_a})
    assert e.value.code == -9 and "rebuild_bvh" in str(e.value)
    r.frame()
    got = _gbuf(gpu, r)
    for k in GBUF:
        assert np.array_equal(_bits(got[k]), _bits(before[k])), k
    r.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    r.pose_objects({2: m_a})
    r.frame()
    r.frame()  # no motion left
    posed = _gbuf(gpu, r)
    tri = gpu.buffer_readback(r.trianglesTextureBuffer)
    nodes = gpu.buffer_readback(r.nodesTextureBuffer)
    cur = gpu.pose_raster(r._pose, 0)
    with pytest.raises(PtError) as e:
        r.pose_objects(np.tile(P.IDENTITY, (4097, 1)))
    assert e.value.code == -6
    r.frame()
    got = _gbuf(gpu, r)
    for k in GBUF:
        assert np.array_equal(_bits(got[k]), _bits(posed[k])), k
    assert np.array_equal(_bits(gpu.buffer_readback(r.trianglesTextureBuffer)), _bits(tri))
    assert np.array_equal(_bits(gpu.buffer_readback(r.nodesTextureBuffer)), _bits(nodes))
    assert np.array_equal(_bits(gpu.pose_raster(r._pose, 0)), _bits(cur))
    assert not np.array_equal(_bits(posed["world"]), _bits(before["world"]))
    r.pose_objects({2: m_b})  # a following valid pose still works
    r.frame()
    assert not np.array_equal(_bits(_gbuf(gpu, r)["world"]), _bits(posed["world"]))
    # mixing with refit_bvh needs a rebuild_bvh in between
    r.refit_bvh(P.tris(s.tri_enc, P.table({2: m_a}, 3)))
    with pytest.raises(PtError) as e:
        r.pose_objects({2: m_b})
    assert e.value.code == -9 and "rebuild_bvh" in str(e.value)
    r.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    assert r.pose_objects({2: m_b}) > 0.0
    r.close()

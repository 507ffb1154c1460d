"""Skinned objects on the device (pt_pose_set_skin / pt_pose_apply_skin, Renderer.set_skin / skin_objects;
csrc/kernels_bvh.hip skin_tris, skin_raster).

* The refitted buffers equal the definitions bit for bit: tests/skin_ref.py for the skinned records, then
  tests/lbvh_refit_ref.py for the refit over them, on a single leaf, less than a wave, less than a block and many
  blocks, as a plain LBVH and under a PLOC top, with 1, 3, 300 and 4096 bones and every influence pattern in one list;
  the walk trees derived after it equal the host functions on the refreshed mirror.
* Matrices are absolute and a skin is interchangeable with a pose: all-zero weights give pt_bvh_refit of the rest
  buffer, as a pose by identities does; skin, pose, skin gives the first skin's bits; the raster lists alternate.
* A corner with one influence of weight 1 equals pt_pose_apply with that bone as the object's matrix.
* G-buffer planes and motion vectors equal those of a renderer driven through refit_bvh with the host arrays the
  definition produces; rendering over skinned buffers is bit-exact against the oracle path tracer.
* Every error returns before the first launch and leaves buffers, trees, planes and the current list as they were.
* render_cli --sway bends the plant.

Comparisons are bitwise through a uint32 view wherever the restatement is not NaN, and NaN wherever it is."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import lbvh_refit_ref as R
import oracle_ref as O
import pose_ref as P
import skin_ref as S

pytestmark = pytest.mark.gpu

GBUF = ("normal_depth", "velocity", "fwidth", "world")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Bit for bit where the restatement b is not NaN, NaN where it is."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(b)
    return bool(np.array_equal(_bits(a)[~nan], _bits(b)[~nan]) and np.all(np.isnan(a[nan])))


def _rest_tris(n, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 45), np.float32)
    t[:, :9] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    t[:, 9:18] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)  # normals of any length: the skin normalises
    t[:, 18:42] = rng.uniform(0, 1, (n, 24)).astype(np.float32)
    t[:, 42] = (np.arange(n) + 1) % 3
    if n >= 17:
        t[7, 12:15] = 0.0  # a zero rest normal: NaN once skinned (corner 22: one influence)
    return t


def _rest_raster(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n * 18).astype(np.float32)


def _bones(n_bones, seed=0):
    """Bone 0 a rotation with a translation; with three or more, bone 1 mirrors and bone 2 scales by zero (NaN
    normals, finite positions); the others turn by -40 .. 40 degrees about z and translate by up to 0.3."""
    from ptsvgf.scene import transform

    rng = np.random.default_rng(seed)
    a = np.radians(rng.uniform(-40, 40, n_bones))
    b = np.tile(P.IDENTITY, (n_bones, 1))
    b[:, 0], b[:, 1], b[:, 4], b[:, 5] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    b[:, 12:15] = rng.uniform(-0.3, 0.3, (n_bones, 3))
    b[0] = transform(rot=(10, 40, -20), trans=(0.3, -0.1, 0.2))
    if n_bones >= 3:
        b[1] = transform(rot=(0, 25, 0), trans=(0.1, 0.0, -0.2), scale=(-1, 1, 1))
        b[2] = transform(trans=(0.2, 0.1, -0.1), scale=(0, 0, 0))
    return b.astype(np.float32)


def _influences(nc, n_bones, seed):
    """Every pattern in one list, by corner index mod 7: kept; one influence of weight 1 in any slot; two; four; four
    that do not sum to 1; the mirroring bone alone; the zero-scale bone alone. Then NaN weights, and indices at both
    ends of the table."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_bones, (nc, 4)).astype(np.uint16)
    w = np.zeros((nc, 4), np.float32)
    pat = np.arange(nc) % 7
    one = np.nonzero(pat == 1)[0]
    w[one, rng.integers(0, 4, len(one))] = 1.0
    two = np.nonzero(pat == 2)[0]
    f = rng.uniform(0.1, 0.9, len(two)).astype(np.float32)
    w[two, 0], w[two, 1] = F(1.0) - f, f
    four = np.nonzero(pat == 3)[0]
    v = rng.uniform(0.1, 1.0, (len(four), 4))
    w[four] = (v / v.sum(axis=1, keepdims=True)).astype(np.float32)
    off = np.nonzero(pat == 4)[0]
    w[off] = rng.uniform(0.1, 0.9, (len(off), 4)).astype(np.float32)
    for p, bone in ((5, 1), (6, 2)):
        sel = np.nonzero(pat == p)[0]
        idx[sel, 0] = min(bone, n_bones - 1)
        w[sel, 0] = 1.0
    if nc > 10:
        idx[10] = (0, n_bones - 1, n_bones // 2, 1 % n_bones)  # four influences spanning the table
    if nc >= 51:
        w[15, 1] = np.nan                 # a NaN weight among others
        w[28] = (0.0, np.nan, 0.0, 0.0)   # and alone: not == 0, so not kept
    return idx, w


class _Built:
    """A pt_bvh_build pair over `tri`, a pose over the same rows, and what the tests read; `with` destroys them."""

    def __init__(self, gl, tri, leaf_n, ploc, raster=None):
        self.gl, self.tri = gl, tri
        self.to = gl.texture_buffer(np.zeros(3, np.float32))
        self.no = gl.texture_buffer(np.zeros(3, np.float32))
        self.extra, self.poses = [], []
        src = gl.texture_buffer(tri)
        try:
            gl.bvh_build(src, self.to, self.no, leaf_n, ploc)
            obj = None if raster is None else (np.arange(raster.size // 18) % 3).astype(np.int32)
            self.raster_obj = obj
            self.pose = gl.pose_create(src, raster, obj)
            self.poses.append(self.pose)
        finally:
            gl.destroy_texture(src)
        self.tri_out, self.nodes = self.read()
        self.order = gl.lbvh_order(self.no)
        assert np.array_equal(np.sort(self.order), np.arange(len(tri)))

    def read(self):
        return self.gl.buffer_readback(self.to).reshape(-1, 45), self.gl.buffer_readback(self.no).reshape(-1, 12)

    def skin(self, bones, **kw):
        return self.gl.pose_apply_skin(self.pose, bones, self.to, self.no, **kw)

    def check(self, want_rows):
        want_tri, want_nodes = R.refit(want_rows, self.order, self.nodes)
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


def _check_buffers(gpu, n, leaf_n, ploc, n_bones):
    t = _rest_tris(n, seed=n + 5)
    idx, w = _influences(3 * n, n_bones, seed=n + n_bones)
    bones = _bones(n_bones, seed=n_bones)
    with _Built(gpu, t, leaf_n, ploc) as b:
        gpu.pose_set_skin(b.pose, idx, w)
        ms = b.skin(bones)
        assert ms > 0.0
        want = S.tris(t, idx, w, bones)
        tri, nodes = b.check(want)
        assert not np.array_equal(_bits(want[:, :18]), _bits(t[:, :18]))
        kept = np.all(w == 0, axis=1)
        assert kept.any() and np.array_equal(_bits(want[:, :9].reshape(-1, 3)[kept]), _bits(t[:, :9].reshape(-1, 3)[kept]))
        if n >= 17:
            assert np.isnan(want[:, 9:18]).any() and np.isnan(want[:, :9]).any()  # NaN weights, the zero normal
            if n_bones >= 3:
                flat = np.nonzero(np.arange(3 * n) % 7 == 6)[0]  # the zero-scale bone alone
                assert np.all(np.isnan(want[:, 9:18].reshape(-1, 3)[flat]))
                assert np.all(np.isfinite(want[:, :9].reshape(-1, 3)[flat]))
        dev, host = gpu.lbvh_trees(b.no, 0), gpu.lbvh_trees(b.no, 1)
        for name in ("binary", "leaves", "wide"):
            assert np.array_equal(_bits(dev[name]), _bits(host[name])), name
        assert dev["info"][:7] == host["info"][:7]
        print(f"n {n} leaf_n {leaf_n} ploc {ploc} bones {n_bones}: {len(nodes)} nodes, skin {ms:.3f} ms")


@pytest.mark.parametrize("n_bones", [1, 3, 300])
@pytest.mark.parametrize("leaf_n,ploc", [(1, 0), (4, 16)])
@pytest.mark.parametrize("n", [1, 2, 17, 1000, 20000])
def test_skinned_buffers_equal_the_restatement(gpu, n, leaf_n, ploc, n_bones):
    """n = 1: the root is a leaf; 2 and 17: less than a wave, less than a block of texels; 1000 and 20000: many
    blocks."""
    _check_buffers(gpu, n, leaf_n, ploc, n_bones)


def test_skinned_buffers_with_the_largest_table(gpu):
    """4096 bones, the indices spanning the table."""
    idx, _ = _influences(3000, 4096, seed=1000 + 4096)
    assert idx.min() == 0 and idx.max() == 4095
    _check_buffers(gpu, 1000, 4, 16, 4096)


def _pose_mats():
    """Three matrices, none the identity (a pose keeps an identity's records, a skin normalises their normals) and
    none holding a -0."""
    from ptsvgf.scene import transform

    m = np.stack([transform(rot=(5, -30, 15), trans=(0.1, 0.2, -0.1)),
                  transform(rot=(10, 40, -20), trans=(0.3, -0.1, 0.2), scale=(1.25, 1.25, 1.25)),
                  transform(rot=(25, -15, 60), trans=(-0.2, 0.1, 0.05), scale=(1, 0.5, 2))]).astype(np.float32) + F(0.0)
    assert not np.any(np.signbit(m) & (m == 0))
    return m


def test_absolute_and_interchangeable_with_a_pose(gpu):
    n, nr = 1000, 300
    t = _rest_tris(n, seed=21)
    rv = _rest_raster(nr, seed=22)
    idx, w = _influences(3 * n, 3, seed=23)
    ridx, rw = _influences(3 * nr, 3, seed=24)
    bones, mats, ident = _bones(3, seed=25), _pose_mats(), np.tile(P.IDENTITY, (3, 1))
    with _Built(gpu, t, 4, 16, rv) as b:
        # all-zero weights: pt_bvh_refit of the rest buffer, the rest raster list current
        gpu.pose_set_skin(b.pose, idx, np.zeros_like(w), ridx, np.zeros_like(rw))
        b.skin(bones)
        a_tri, a_nodes = b.read()
        assert np.array_equal(_bits(gpu.pose_raster(b.pose, 0)), _bits(rv))
        src = gpu.texture_buffer(t)
        b.extra.append(src)
        gpu.bvh_refit(src, b.to, b.no)
        r_tri, r_nodes = b.read()
        assert np.array_equal(_bits(a_tri), _bits(r_tri)) and np.array_equal(_bits(a_nodes), _bits(r_nodes))
        assert np.array_equal(_bits(a_tri), _bits(b.tri_out))
        gpu.pose_apply(b.pose, ident, b.to, b.no)  # so does a pose by identities
        i_tri, i_nodes = b.read()
        assert np.array_equal(_bits(i_tri), _bits(a_tri)) and np.array_equal(_bits(i_nodes), _bits(a_nodes))
        # a second pt_pose_set_skin replaces the skin; skin, pose, skin: the first skin's bits
        gpu.pose_set_skin(b.pose, idx, w, ridx, rw)
        b.skin(bones)
        s_tri, s_nodes = b.check(S.tris(t, idx, w, bones))
        skinned = S.raster(rv, ridx, rw, bones)
        assert _same(gpu.pose_raster(b.pose, 0), skinned) and not _same(skinned, rv)
        assert np.array_equal(_bits(gpu.pose_raster(b.pose, 1)), _bits(rv))
        gpu.pose_apply(b.pose, mats, b.to, b.no)
        b.check(P.tris(t, mats))
        posed = P.raster(rv, b.raster_obj, mats)
        assert _same(gpu.pose_raster(b.pose, 0), posed) and _same(gpu.pose_raster(b.pose, 1), skinned)
        b.skin(bones)
        tri, nodes = b.read()
        assert np.array_equal(_bits(tri), _bits(s_tri)) and np.array_equal(_bits(nodes), _bits(s_nodes))
        assert _same(gpu.pose_raster(b.pose, 0), skinned) and _same(gpu.pose_raster(b.pose, 1), posed)


def test_single_influence_equals_a_pose(gpu):
    """Corner influences (objIndex, 1, 0 ...) with the pose's matrices as bones: pt_pose_apply's bits."""
    n, nr = 1000, 300
    t = _rest_tris(n, seed=41)
    t[3, 42], t[5, 42], t[11, 42], t[13, 42] = 7.0, -1.0, 2.5, np.nan  # records of no object: kept by both
    rv = _rest_raster(nr, seed=42)
    mats = _pose_mats()
    rng = np.random.default_rng(43)

    def influences(obj):
        obj = np.repeat(obj, 3)
        idx = rng.integers(0, 3, (len(obj), 4)).astype(np.uint16)  # weight 0: any valid index
        w = np.zeros((len(obj), 4), np.float32)
        named = obj >= 0
        idx[named, 0] = obj[named]
        w[named, 0] = 1.0
        return idx, w

    with _Built(gpu, t, 4, 16, rv) as b:
        b.raster_obj[[2, 9]] = 7, -1
        gpu.pose_destroy(b.pose)
        src = gpu.texture_buffer(t)
        b.extra.append(src)
        b.pose = gpu.pose_create(src, rv, b.raster_obj)
        b.poses = [b.pose]
        gpu.pose_apply(b.pose, mats, b.to, b.no)
        p_tri, p_nodes = b.check(P.tris(t, mats))
        p_raster = gpu.pose_raster(b.pose, 0)
        gpu.pose_apply(b.pose, np.tile(P.IDENTITY, (3, 1)), b.to, b.no)
        idx, w = influences(P.objects_of(t[:, 42], 3))
        ridx, rw = influences(P.objects_of(b.raster_obj.astype(np.int64), 3))
        gpu.pose_set_skin(b.pose, idx, w, ridx, rw)
        b.skin(mats)
        s_tri, s_nodes = b.read()
        assert np.array_equal(_bits(s_tri), _bits(p_tri)) and np.array_equal(_bits(s_nodes), _bits(p_nodes))
        assert np.array_equal(_bits(gpu.pose_raster(b.pose, 0)), _bits(p_raster))
        assert not np.array_equal(_bits(s_tri), _bits(b.tri_out))


def _gbuf(gpu, r):
    got = r.planes()
    return {k: gpu.readback(got[k]) for k in GBUF}


def _renderer(scene, W, H, gbuffer_mode=None, **kw):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene, W, H, mode="fast", run_taa=False, run_output=False, **kw)
    if gbuffer_mode is not None:
        for p in r.init_pass:
            p.set_uniform_int("gbuffer_mode", gbuffer_mode)
    return r


@pytest.fixture(scope="module")
def plant(scene_small):
    """The small scene's plant (object 2) on a chain of 4 bones up its height: the influences of both lists, and
    the skinned host arrays of two bends."""
    from ptsvgf import skin

    s = scene_small
    tp, rp = skin.corner_positions(s.tri_enc), skin.corner_positions_raster(s.raster)
    tmask, rmask = np.repeat(s.tri_enc[:, 42] == 2.0, 3), np.repeat(s.raster_obj == 2, 3)
    lo, hi = tp[tmask].min(axis=0), tp[tmask].max(axis=0)
    base = np.array([(lo[0] + hi[0]) / 2, lo[1], (lo[2] + hi[2]) / 2])
    tip = np.array([base[0], hi[1], base[2]])
    tb, tw = skin.chain_weights(tp, base, tip, 4, tmask)
    rb, rw = skin.chain_weights(rp, base, tip, 4, rmask)
    bends = [skin.chain_bones(base, tip, 4, deg, (0, 0, 1)) for deg in (6.0, 12.0)]
    tris = [S.tris(s.tri_enc, tb, tw, m) for m in bends]
    lists = [S.raster(s.raster, rb, rw, m) for m in bends]
    return dict(skin=(tb, tw, rb, rw), bends=bends, tris=tris, lists=lists)


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_skinned_raster_lists_alternate(gpu, scene_small, plant, gbuffer_mode):
    """Two bends and a frame after, against a renderer driven through refit_bvh with the definition's host arrays:
    previous list = rest for the first bend, the first skinned list for the second, no motion on the frame after."""
    W, H = 160, 96
    s = scene_small
    lists, bends = plant["lists"], plant["bends"]
    assert not np.array_equal(_bits(lists[0]), _bits(s.raster)) and not np.array_equal(_bits(lists[0]), _bits(lists[1]))

    r = _renderer(s, W, H, gbuffer_mode)
    r.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    r.set_skin(*plant["skin"])
    got = []
    assert r.skin_objects(bends[0]) > 0.0
    assert _same(gpu.pose_raster(r._pose, 0), lists[0])
    assert np.array_equal(_bits(gpu.pose_raster(r._pose, 1)), _bits(s.raster))
    r.frame()
    got.append(_gbuf(gpu, r))
    r.skin_objects(bends[1])
    assert _same(gpu.pose_raster(r._pose, 0), lists[1]) and _same(gpu.pose_raster(r._pose, 1), lists[0])
    r.frame()
    got.append(_gbuf(gpu, r))
    r.frame()  # the frame after: object_motion = 0 again
    got.append(_gbuf(gpu, r))
    r.skin_objects(bends[1], motion=False)  # the same bend without records
    r.frame()
    plain = _gbuf(gpu, r)
    r.close()

    h = _renderer(s, W, H, gbuffer_mode)
    h.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    want = []
    h.refit_bvh(plant["tris"][0], raster=lists[0], prev_raster=s.raster)
    h.frame()
    want.append(_gbuf(gpu, h))
    h.refit_bvh(plant["tris"][1], raster=lists[1], prev_raster=lists[0])
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
    assert not np.array_equal(_bits(got[0]["world"]), _bits(got[1]["world"]))        # and the plant bent further


@pytest.mark.parametrize("lbvh_wide", [1, 0])
def test_render_over_skinned_buffers_matches_oracle(gpu, scene_small, plant, lbvh_wide):
    """Against the oracle on the same (skinned, refitted) buffers; without a raster list only the path tracer's tree
    is skinned."""
    W, H = 96, 64
    s = scene_small
    r = _renderer(s, W, H, frames_in_flight=2)
    nodes0, _ = r.rebuild_bvh(leaf_n=8, ploc_radius=16)
    r.set_lbvh_wide(bool(lbvh_wide))
    r.set_skin(*plant["skin"][:2])
    r.frame()
    old_nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    order = gpu.lbvh_order(r.nodesTextureBuffer)
    assert r.skin_objects(plant["bends"][1]) > 0.0
    tri = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    assert len(nodes) == nodes0
    want_tri, want_nodes = R.refit(plant["tris"][1], order, old_nodes)
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


def test_skin_errors_leave_the_buffers_unchanged(gpu):
    from ptsvgf._lib import PtError, fptr, pt

    n = 100
    t = _rest_tris(n, seed=31)
    rv = _rest_raster(n, seed=32)
    idx, w = _influences(3 * n, 3, seed=33)   # the largest index: 2
    bones = _bones(3, seed=34)
    u16 = C.POINTER(C.c_uint16)
    with _Built(gpu, t, 4, 16, rv) as b:
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

        def raw(pose, bones16, n_bones, to, no, rpass=0):
            ms = C.c_float()
            rc = pt().pt_pose_apply_skin(pose, bones16, n_bones, to, no, rpass, 1, C.byref(ms))
            if rc < 0:
                raise PtError(rc, (pt().pt_last_error() or b"").decode())

        def raw_set(pose, tb, tw, rb, rw):
            rc = pt().pt_pose_set_skin(pose, None if tb is None else tb.ctypes.data_as(u16),
                                       None if tw is None else fptr(tw), None if rb is None else rb.ctypes.data_as(u16),
                                       None if rw is None else fptr(rw))
            if rc < 0:
                raise PtError(rc, (pt().pt_last_error() or b"").decode())

        m = np.ascontiguousarray(bones, np.float32)
        big = np.tile(P.IDENTITY, (4097, 1))
        refused(-9, lambda: b.skin(bones))                       # no skin yet
        refused(-9, lambda: raw(b.pose, None, 0, b.to, b.to))    # reported before anything else of the call
        idx1, w1 = np.ascontiguousarray(idx.reshape(-1)), np.ascontiguousarray(w.reshape(-1))
        refused(-6, lambda: raw_set(b.pose, idx1, w1, None, None))     # a raster list needs its influences
        refused(-6, lambda: raw_set(b.pose, idx1, w1, idx1, None))
        refused(-6, lambda: raw_set(bare, idx1, w1, idx1, w1))         # and a pose without one takes none
        refused(-6, lambda: raw_set(b.pose, None, w1, idx1, w1))
        refused(-6, lambda: raw_set(b.pose, idx1, None, idx1, w1))
        refused(-1, lambda: raw_set(987654, idx1, w1, idx1, w1))
        refused(-9, lambda: b.skin(bones))                       # still none
        gpu.pose_set_skin(b.pose, idx, w, idx, w)
        gpu.pose_set_skin(bare, idx, w)
        refused(-6, lambda: raw(b.pose, None, 3, b.to, b.no))
        refused(-6, lambda: raw(b.pose, fptr(m), 0, b.to, b.no))
        refused(-6, lambda: raw(b.pose, fptr(m), -1, b.to, b.no))
        refused(-6, lambda: b.skin(big))
        refused(-6, lambda: raw(b.pose, fptr(m), 2, b.to, b.no))       # the skin names bone 2
        refused(-6, lambda: raw(bare, fptr(m), 3, b.to, b.no, rpass=12345))  # a pass for a pose without a raster list
        refused(-1, lambda: raw(b.pose, fptr(m), 3, b.to, b.no, rpass=0xFFFFFFF0))  # no such pass
        refused(-6, lambda: gpu.pose_apply_skin(b.pose, bones, b.to, b.to))    # a handle used twice
        refused(-1, lambda: gpu.pose_apply_skin(987654, bones, b.to, b.no))    # never a pose
        # buffers a host upload wrote (the very contents of the build): not a pair
        up_t, up_n = gpu.texture_buffer(b.tri_out), gpu.texture_buffer(b.nodes)
        b.extra += [up_t, up_n]
        refused(-9, lambda: gpu.pose_apply_skin(b.pose, bones, up_t, up_n), pair=(up_t, up_n))
        refused(-9, lambda: gpu.pose_apply_skin(b.pose, bones, up_t, b.no))
        # a pair of another triangle count
        with _Built(gpu, _rest_tris(64, seed=35), 4, 0) as other:
            refused(-6, lambda: gpu.pose_apply_skin(b.pose, bones, other.to, other.no), pair=(other.to, other.no),
                    want=(other.tri_out, other.nodes))
        trees1 = gpu.lbvh_trees(b.no, 0)
        for name in ("binary", "leaves", "wide"):
            assert np.array_equal(_bits(trees0[name]), _bits(trees1[name])), name
        # a following valid call still works, with either pose, and a larger table than the skin needs
        b.skin(bones)
        want = S.tris(t, idx, w, bones)
        b.check(want)
        assert _same(gpu.pose_raster(b.pose, 0), S.raster(rv, idx, w, bones))
        gpu.pose_apply_skin(bare, _bones(7, seed=34)[:7], b.to, b.no)
        b.check(S.tris(t, idx, w, _bones(7, seed=34)))
        # use after destroy
        gpu.pose_destroy(bare)
        b.poses.remove(bare)
        with pytest.raises(PtError) as e:
            gpu.pose_apply_skin(bare, bones, b.to, b.no)
        assert e.value.code == -1
        with pytest.raises(PtError) as e:
            gpu.pose_set_skin(bare, idx, w)
        assert e.value.code == -1


def test_skin_objects_errors_leave_the_renderer_drawing(gpu, scene_small, plant):
    """Before any rebuild_bvh, without a skin, with raster influences missing, with a table too small or too large,
    and after a refit_bvh: the planes, the scene buffers and the pose's current list are as before."""
    from ptsvgf._lib import PtError

    W, H = 96, 64
    s = scene_small
    tb, tw, rb, rw = plant["skin"]
    bends = plant["bends"]
    r = _renderer(s, W, H)
    r.frame()
    before = _gbuf(gpu, r)
    for call in (lambda: r.skin_objects(bends[0]), lambda: r.set_skin(tb, tw, rb, rw)):
        with pytest.raises(PtError) as e:
            call()
        assert e.value.code == -9 and "rebuild_bvh" in str(e.value)
    r.frame()
    got = _gbuf(gpu, r)
    for k in GBUF:
        assert np.array_equal(_bits(got[k]), _bits(before[k])), k
    r.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    with pytest.raises(PtError) as e:
        r.skin_objects(bends[0])  # no set_skin
    assert e.value.code == -9 and "set_skin" in str(e.value)
    with pytest.raises(ValueError):
        r.set_skin(tb, tw)  # rebuild_bvh got a raster list
    with pytest.raises(ValueError):
        r.set_skin(tb, tw, rb[:-1], rw[:-1])
    with pytest.raises(PtError) as e:
        r.skin_objects(bends[0])  # a refused set_skin set nothing
    assert e.value.code == -9
    r.frame()
    got = _gbuf(gpu, r)
    for k in GBUF:
        assert np.array_equal(_bits(got[k]), _bits(before[k])), k
    r.set_skin(tb, tw, rb, rw)
    r.skin_objects(bends[0])
    r.frame()
    r.frame()  # no motion left
    bent = _gbuf(gpu, r)
    tri = gpu.buffer_readback(r.trianglesTextureBuffer)
    nodes = gpu.buffer_readback(r.nodesTextureBuffer)
    cur = gpu.pose_raster(r._pose, 0)
    for bad in (np.tile(P.IDENTITY, (4097, 1)), bends[1][:3]):  # too large for the library; the skin names bone 3
        with pytest.raises(PtError) as e:
            r.skin_objects(bad)
        assert e.value.code == -6
        r.frame()
        got = _gbuf(gpu, r)
        for k in GBUF:
            assert np.array_equal(_bits(got[k]), _bits(bent[k])), k
        assert np.array_equal(_bits(gpu.buffer_readback(r.trianglesTextureBuffer)), _bits(tri))
        assert np.array_equal(_bits(gpu.buffer_readback(r.nodesTextureBuffer)), _bits(nodes))
        assert np.array_equal(_bits(gpu.pose_raster(r._pose, 0)), _bits(cur))
    assert not np.array_equal(_bits(bent["world"]), _bits(before["world"]))
    r.skin_objects(bends[1])  # a following valid call still works
    r.frame()
    assert not np.array_equal(_bits(_gbuf(gpu, r)["world"]), _bits(bent["world"]))
    # pose_objects and skin_objects alternate on the one pose
    from ptsvgf.scene import transform

    r.pose_objects({2: transform(trans=(0, 0.05, 0))})
    r.skin_objects(bends[0])
    assert _same(gpu.pose_raster(r._pose, 0), plant["lists"][0])
    # a refit_bvh drops the rest pose and the skin with it
    r.refit_bvh(plant["tris"][0])
    with pytest.raises(PtError) as e:
        r.skin_objects(bends[1])
    assert e.value.code == -9 and "rebuild_bvh" in str(e.value)
    r.rebuild_bvh(raster=s.raster, leaf_n=8, ploc_radius=16)
    with pytest.raises(PtError) as e:
        r.skin_objects(bends[1])  # the skin went with the rest pose
    assert e.value.code == -9 and "set_skin" in str(e.value)
    r.set_skin(tb, tw, rb, rw)
    assert r.skin_objects(bends[1]) > 0.0
    r.close()


def test_cli_sway_bends_the_plant(gpu, scene_small, tmp_path, monkeypatch):
    """render_cli.main on the session's library and small scene, 3 frames at 96 x 64, with --sway 8 and without."""
    from ptsvgf import gl, render_cli
    from ptsvgf import scene as scene_mod

    monkeypatch.setattr(scene_mod, "build_scene", lambda name: scene_small)
    monkeypatch.setattr(gl, "init", lambda device=0: None)
    monkeypatch.setattr(gl, "shutdown", lambda: None)
    out = {}
    for sway in (True, False):
        png = str(tmp_path / f"sway{int(sway)}.png")
        args = ["--width", "96", "--height", "64", "--frames", "3", "--png", png]
        assert render_cli.main(args + (["--sway", "8"] if sway else [])) == 0
        assert os.path.getsize(png) > 0
        out[sway] = open(png, "rb").read()
    assert out[True][:8] == b"\x89PNG\r\n\x1a\n"
    assert out[True] != out[False]

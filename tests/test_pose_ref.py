"""Posed objects on the CPU: which raster triangle belongs to which object (pts_scene_raster_objects), and the
definition of a pose (tests/pose_ref.py) checked against what a user expects of it: the host builder run with the
composed matrix, which transforms the vertices first and recomputes the normals from them."""
import os

import numpy as np
import pytest

import pose_ref as P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(REPO, "assets", "models")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_raster_objects_of_the_small_scene(scene_small):
    obj = scene_small.raster_obj
    assert obj is not None and obj.dtype == np.int32
    assert obj.shape == (scene_small.raster.size // 18,)
    assert np.all(np.diff(obj) >= 0)  # runs in emission order: table, clock, plant
    want = np.bincount(scene_small.tri_enc[:, 42].astype(np.int64))
    assert np.array_equal(np.bincount(obj), want)
    assert len(want) == 3 and np.all(want > 0)


def test_raster_objects_entry_point_checks_its_size():
    import ctypes as C

    from ptsvgf._lib import pts
    from ptsvgf.scene import SceneBuilder, gen_cornell, material, transform

    b = SceneBuilder()
    pos, idx = gen_cornell()
    b.add_mesh(pos, idx, material(), transform(), False, 5)
    b.add_mesh(pos, idx, material(), transform(trans=(3, 0, 0)), False, 2)
    assert np.array_equal(b.raster_objects(), np.repeat([5, 2], len(idx)).astype(np.int32))
    out = np.zeros(4 * len(idx), np.int32)
    for n in (2 * len(idx) - 1, 2 * len(idx) + 1):
        assert pts().pts_scene_raster_objects(b._s, out.ctypes.data_as(C.POINTER(C.c_int)), n) < 0
    assert pts().pts_scene_raster_objects(b._s, None, 2 * len(idx)) < 0


def _rows(n, seed=0):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, (n, 45)).astype(np.float32)
    t[:, 42] = np.arange(n) % 3
    t[:, 43:] = 0
    return t


def test_identity_and_records_of_no_object_keep_their_bits():
    from ptsvgf.scene import transform

    t = _rows(64, seed=1)
    t[5, 3] = np.nan  # any bit pattern is kept
    t[6, 10] = -0.0
    ident = np.tile(transform(), (3, 1))
    assert np.array_equal(ident[0], P.IDENTITY)
    assert np.array_equal(_bits(P.tris(t, ident)), _bits(t))
    M = transform(rot=(10, 40, -20), trans=(0.3, -0.1, 0.2), scale=(1.25, 1.25, 1.25))
    for bad in (3.0, 7.0, -1.0, 2.5, np.nan, np.inf, -0.5):
        u = t.copy()
        u[:, 42] = bad
        assert np.array_equal(_bits(P.tris(u, np.tile(M, (3, 1)))), _bits(u)), bad
    # the raster list: ints outside [0, n_obj)
    r = np.random.default_rng(2).uniform(-1, 1, 40 * 18).astype(np.float32)
    for bad in (3, 7, -1, 2 ** 31 - 1, -2 ** 31):
        assert np.array_equal(_bits(P.raster(r, np.full(40, bad), np.tile(M, (3, 1)))), _bits(r)), bad
    assert np.array_equal(_bits(P.raster(r, np.arange(40) % 3, ident)), _bits(r))
    # only the object with a matrix moves, and only positions and normals of its rows
    got = P.tris(t, P.table({1: M}, 3))
    moved = t[:, 42] == 1
    assert np.array_equal(_bits(got[~moved]), _bits(t[~moved]))
    assert np.array_equal(_bits(got[:, 18:]), _bits(t[:, 18:]))
    assert not np.any(_bits(got[moved, :18]) == _bits(t[moved, :18]))
    # absolute: a pose is a function of the rest rows alone, the identity gives them back
    assert np.array_equal(_bits(P.tris(t, P.table({}, 3))), _bits(t))


def _compose(M, T0):
    """M * T0 of two glm column-major mat4s, formed in float64 and rounded once."""
    a = np.asarray(M, np.float64).reshape(4, 4).T
    b = np.asarray(T0, np.float64).reshape(4, 4).T
    return np.ascontiguousarray((a @ b).T).reshape(16).astype(np.float32)


def _three_objects(trans, smooth):
    from ptsvgf.scene import SceneBuilder, gen_plant, material

    b = SceneBuilder()
    b.add_obj(os.path.join(MODELS, "clock.obj"), material(), trans, smooth, 0)
    b.add_obj(os.path.join(MODELS, "table.obj"), material(), trans, smooth, 1)
    pos, idx = gen_plant(0, 40)
    b.add_mesh(pos, idx, material(), trans, smooth, 2)
    b.build(8)
    return b.encode()[2], b.raster_objects()


@pytest.mark.parametrize("smooth", [True, False])
def test_pose_equals_the_host_builder_with_the_composed_matrix(smooth):
    """pose_ref(raster(T0), M) against raster(M T0) for a similarity M: the builder transforms the vertices and
    recomputes the normals, the pose transforms both. Measured with exactly these inputs: positions differ by at
    most 2.4e-7 (2.0e-7 of the 1.19 extent, the largest axis range of the posed positions); the normals' largest component difference has median 2-4e-6 and maximum
    9.3e-4 (smooth) / 2.8e-3 (flat), on slivers whose recomputed normal is itself ill-conditioned; 0.21 % (smooth) /
    0.08 % (flat) of the vertices are beyond 1e-4."""
    from ptsvgf.scene import transform

    T0 = transform(rot=(0, 30, 0), trans=(0.1, 0.2, 0), scale=(0.5, 0.5, 0.5))
    M = transform(rot=(10, 40, -20), trans=(0.3, -0.1, 0.2), scale=(1.25, 1.25, 1.25))
    rest, obj = _three_objects(T0, smooth)
    want, obj2 = _three_objects(_compose(M, T0), smooth)
    assert rest.size == want.size == 18313 * 18 and np.array_equal(obj, obj2)
    got = P.raster(rest, obj, np.tile(M, (3, 1)))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    g, w = got.reshape(-1, 6).astype(np.float64), want.reshape(-1, 6).astype(np.float64)
    extent = float(np.max(w[:, :3].max(axis=0) - w[:, :3].min(axis=0)))
    dpos = float(np.max(np.abs(g[:, :3] - w[:, :3])))
    dn = np.max(np.abs(g[:, 3:] - w[:, 3:]), axis=1)
    print(f"smooth {smooth}: extent {extent:.3f}, positions differ by {dpos:.3g}; normals: median {np.median(dn):.3g}, "
          f"max {dn.max():.3g}, beyond 1e-4: {100 * np.mean(dn > 1e-4):.2f} %")
    # four float32 roundings of operands no larger than the extent, with a margin of 4x
    assert dpos <= 1e-6 * extent
    assert np.mean(dn > 1e-4) <= 0.01
    assert dn.max() <= 1e-2


def _flat_mesh():
    """Flat-shaded triangles away from degeneracy: the Cornell box and the teapot stand-in."""
    from ptsvgf.scene import SceneBuilder, gen_cornell, gen_teapot, material, transform

    b = SceneBuilder()
    pos, idx = gen_cornell()
    b.add_mesh(pos, idx, material(), transform(rot=(0, 30, 0), trans=(0.1, 0.2, 0)), False, 0)
    pos, idx = gen_teapot(12)
    b.add_mesh(pos, idx, material(), transform(rot=(20, 0, 10), scale=(0.5, 0.5, 0.5)), False, 1)
    b.build(8)
    return b.encode()[2], b.raster_objects()


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _well_shaped(rest):
    """Triangles whose rest normal is well conditioned: no sliver (smallest height at least 5 % of the longest
    edge), so the float32 normal of the rest pose is itself good to a few ulp."""
    v = rest.reshape(-1, 3, 6)[:, :, :3].astype(np.float64)
    e = [v[:, 1] - v[:, 0], v[:, 2] - v[:, 1], v[:, 0] - v[:, 2]]
    longest = np.max([np.linalg.norm(x, axis=1) for x in e], axis=0)
    area2 = np.linalg.norm(np.cross(e[0], -e[2]), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return area2 / longest >= 0.05 * longest


def test_mirror_flips_and_nonuniform_scale_keeps_normals_perpendicular():
    from ptsvgf.scene import transform

    rest, obj = _flat_mesh()
    keep = _well_shaped(rest)
    assert keep.sum() > 100
    mirror = transform(scale=(-1, 1, 1))
    got = P.raster(rest, obj, np.tile(mirror, (2, 1))).reshape(-1, 3, 6)[keep].astype(np.float64)
    face = _unit(np.cross(got[:, 1, :3] - got[:, 0, :3], got[:, 2, :3] - got[:, 0, :3]))
    for v in range(3):
        assert np.max(np.abs(got[:, v, 3:] - face)) <= 1e-5
    # flipped with the winding: the mirrored direction (-x, y, z), negated
    r = rest.reshape(-1, 3, 6)[keep].astype(np.float64)
    assert np.max(np.abs(got[:, :, 3:] - r[:, :, 3:] * np.array([1.0, -1.0, -1.0]))) <= 1e-6
    squash = transform(rot=(10, 40, -20), scale=(1, 0.5, 2))
    got = P.raster(rest, obj, np.tile(squash, (2, 1))).reshape(-1, 3, 6)[keep].astype(np.float64)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        edge = _unit(got[:, b, :3] - got[:, a, :3])
        for v in range(3):
            assert np.max(np.abs(np.sum(got[:, v, 3:] * edge, axis=1))) <= 1e-5
    assert np.max(np.abs(np.linalg.norm(got[:, 0, 3:], axis=1) - 1.0)) <= 1e-6

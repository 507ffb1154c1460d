"""The definition of a skin (tests/skin_ref.py) on the CPU, checked against what a user expects of linear blend
skinning: a float64 LBS, a pose where a corner has one influence, the bone itself where the weights of one bone sum
to 1; then its rules: kept corners, NaN weights, non-finite bones named with weight 0, singular blends, and that equal
inputs give equal bits.

The input is that of the prototype the definition was measured on: 200 000 random corners in [-1, 1]^3 and 7 bones
that rotate by -20 .. 40 degrees and translate by up to 0.3, two to four influences per corner. Measured there: at
most 2.1e-7 from float64 in a position and 2.0e-7 in a normal component, the smallest |det| of a blended 3x3 0.75.
The bars are 1e-6 x the coordinate extent and 1e-5: 5x and 50x over that."""
import numpy as np
import pytest

import pose_ref as P
import skin_ref as S

F = np.float32
N = 200_000
N_BONES = 7


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bones():
    """Rotations of -20 .. 40 degrees about x, y, z in turn, translations up to 0.3; no -0 among the floats."""
    from ptsvgf.scene import transform

    rng = np.random.default_rng(7)
    out = []
    for k, a in enumerate(np.linspace(-20.0, 40.0, N_BONES)):
        rot = [0.0, 0.0, 0.0]
        rot[k % 3] = float(a)
        out.append(transform(rot=tuple(rot), trans=tuple(rng.uniform(-0.3, 0.3, 3))))
    return np.stack(out).astype(np.float32) + F(0.0)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    pos = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    nrm = rng.normal(size=(N, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    idx = rng.integers(0, N_BONES, (N, 4)).astype(np.uint16)
    w = rng.uniform(0.1, 1.0, (N, 4))
    used = rng.integers(2, 5, N)  # two to four influences
    w[np.arange(4)[None, :] >= used[:, None]] = 0.0
    w = (w / w.sum(axis=1, keepdims=True)).astype(np.float32)
    bones = _bones()
    got = S.corners(pos, nrm, idx, w, bones)
    return dict(pos=pos, nrm=nrm, idx=idx, w=w, bones=bones, got=got)


def test_definition_against_float64_lbs(data):
    pos, nrm, idx, w, bones = (data[k] for k in ("pos", "nrm", "idx", "w", "bones"))
    B = bones.astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)  # row-major 4x4s
    M = np.einsum("ns,nsij->nij", w.astype(np.float64), B[idx.astype(np.int64)])
    want_p = np.einsum("nij,nj->ni", M[:, :3, :3], pos.astype(np.float64)) + M[:, :3, 3]
    det = np.linalg.det(M[:, :3, :3])
    v = np.einsum("nji,nj->ni", np.linalg.inv(M[:, :3, :3]), nrm.astype(np.float64))  # inverse transpose
    want_n = v / np.linalg.norm(v, axis=1, keepdims=True)
    got_p, got_n = data["got"]
    extent = float(np.max(want_p.max(axis=0) - want_p.min(axis=0)))
    dp = float(np.max(np.abs(got_p - want_p)))
    dn = float(np.max(np.abs(got_n - want_n)))
    print(f"extent {extent:.3f}, smallest |det| {np.abs(det).min():.3f}: positions differ by {dp:.3g}, "
          f"normal components by {dn:.3g}")
    assert np.abs(det).min() >= 0.5  # the blend stays well conditioned: what the bars below presuppose
    assert np.all(det > 0)
    assert dp <= 1e-6 * extent
    assert dn <= 1e-5


def test_single_influence_equals_a_pose(data):
    pos, nrm, bones = data["pos"][:20000], data["nrm"][:20000], data["bones"]
    rng = np.random.default_rng(3)
    for k in range(N_BONES):
        idx = rng.integers(0, N_BONES, (len(pos), 4)).astype(np.uint16)  # weight 0: any valid index
        w = np.zeros((len(pos), 4), np.float32)
        slot = rng.integers(0, 4, len(pos))
        idx[np.arange(len(pos)), slot] = k
        w[np.arange(len(pos)), slot] = 1.0
        got_p, got_n = S.corners(pos, nrm, idx, w, bones)
        assert np.array_equal(_bits(got_p), _bits(P.points(bones[k], pos))), k
        assert np.array_equal(_bits(got_n), _bits(P.normals(bones[k], nrm))), k


def test_half_weights_on_one_bone_give_the_bone_back(data):
    bones = data["bones"]
    for k in range(N_BONES):
        m = S.blend(bones, [[k, k, 0, 0]], np.array([[0.5, 0.5, 0, 0]], np.float32))[0]
        assert np.array_equal(_bits(m[list(S.AFFINE)]), _bits(bones[k][list(S.AFFINE)])), k


def test_kept_corners_keep_their_bits(data):
    pos, nrm, idx, w, bones = (data[k][:64].copy() for k in ("pos", "nrm", "idx", "w", "bones"))
    bones = data["bones"]
    pos[3, 1], nrm[4, 0], pos[5, 2] = np.nan, -0.0, np.inf  # any bit pattern is kept
    zero = np.zeros_like(w)
    zero[7] = -0.0  # -0 == 0
    got_p, got_n = S.corners(pos, nrm, idx, zero, bones)
    assert np.array_equal(_bits(got_p), _bits(pos)) and np.array_equal(_bits(got_n), _bits(nrm))
    # only the skinned corners move, and a corner naming no bone of the table is kept
    w2 = w.copy()
    w2[::2] = 0.0
    idx2 = idx.copy()
    idx2[1, 2] = N_BONES
    got_p, got_n = S.corners(pos, nrm, idx2, w2, bones)
    kept = np.zeros(64, bool)
    kept[::2] = True
    kept[1] = True
    assert np.array_equal(_bits(got_p[kept]), _bits(pos[kept])) and np.array_equal(_bits(got_n[kept]), _bits(nrm[kept]))
    moved = ~kept & np.all(np.isfinite(pos), axis=1)
    assert not np.any(np.all(_bits(got_p[moved]) == _bits(pos[moved]), axis=1))
    # the rest of a Triangle_encoded row is copied, and rows and the raster list agree corner for corner
    rng = np.random.default_rng(5)
    rows = rng.uniform(-1, 1, (8, 45)).astype(np.float32)
    t = S.tris(rows, idx[:24], w[:24], bones)
    assert np.array_equal(_bits(t[:, 18:]), _bits(rows[:, 18:]))
    rl = np.concatenate([rows[:, 0:9].reshape(-1, 3), rows[:, 9:18].reshape(-1, 3)], axis=1).reshape(-1)
    r = S.raster(rl, idx[:24], w[:24], bones).reshape(-1, 6)
    assert np.array_equal(_bits(r[:, :3]), _bits(t[:, 0:9].reshape(-1, 3)))
    assert np.array_equal(_bits(r[:, 3:]), _bits(t[:, 9:18].reshape(-1, 3)))


def test_nan_rules(data):
    pos, nrm, idx, w = (data[k][:16].copy() for k in ("pos", "nrm", "idx", "w"))
    bones = data["bones"].copy()
    # a NaN weight is not == 0: the corner is skinned, to NaN, also when the other three are 0
    w[2] = (0.0, np.nan, 0.0, 0.0)
    w[3, 0] = np.nan
    got_p, got_n = S.corners(pos, nrm, idx, w, bones)
    for c in (2, 3):
        assert np.all(np.isnan(got_p[c])) and np.all(np.isnan(got_n[c]))
    ok = np.ones(16, bool)
    ok[[2, 3]] = False
    assert np.all(np.isfinite(got_p[ok])) and np.all(np.isfinite(got_n[ok]))
    # all four terms are evaluated: a non-finite float in a bone named with weight 0 yields NaN
    w = data["w"][:16].copy()
    idx[:] = 1
    idx[:, 3] = 6
    w[:, 3] = 0.0
    bones[6, 13] = np.inf  # translation y
    got_p, got_n = S.corners(pos, nrm, idx, w, bones)
    assert np.all(np.isnan(got_p[:, 1])) and np.all(np.isfinite(got_p[:, [0, 2]])) and np.all(np.isfinite(got_n))
    bones[6, 13] = 0.0
    bones[6, 5] = np.nan  # the upper 3x3: the normal goes too
    got_p, got_n = S.corners(pos, nrm, idx, w, bones)
    assert np.all(np.isnan(got_p[:, 1])) and np.all(np.isnan(got_n))
    # floats 3, 7, 11, 15 are not read
    bones = data["bones"].copy()
    ref = S.corners(pos, nrm, data["idx"][:16], data["w"][:16], bones)
    bones[:, [3, 7, 11, 15]] = np.nan
    got = S.corners(pos, nrm, data["idx"][:16], data["w"][:16], bones)
    assert np.array_equal(_bits(got[0]), _bits(ref[0])) and np.array_equal(_bits(got[1]), _bits(ref[1]))


def test_singular_blend_and_zero_normal():
    from ptsvgf.scene import transform

    pos = np.array([[0.3, -0.2, 0.5]] * 3, np.float32)
    nrm = np.array([[0.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    bones = np.stack([transform(trans=(0.1, 0.2, 0.3), scale=(0, 0, 0)), transform(rot=(0, 30, 0))]).astype(np.float32)
    idx = np.array([[0, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0]], np.uint16)
    w = np.array([[1, 0, 0, 0], [0.5, 0.5, 0, 0], [1, 0, 0, 0]], np.float32)
    got_p, got_n = S.corners(pos, nrm, idx, w, bones)
    assert np.all(np.isfinite(got_p))
    assert np.all(np.isnan(got_n[0]))       # a zero scale: every cofactor is 0, and 0 has no direction
    assert np.all(np.isfinite(got_n[1]))    # half of it: regular again
    assert np.all(np.isnan(got_n[2]))       # a zero rest normal has no direction


def test_equal_inputs_give_equal_bits(data):
    pos, nrm, idx, w, bones = (data[k] for k in ("pos", "nrm", "idx", "w", "bones"))
    got_p, got_n = data["got"]
    # the same corners again, at other places of a shorter list
    sel = np.random.default_rng(9).permutation(N)[:5000]
    again_p, again_n = S.corners(pos[sel], nrm[sel], idx[sel], w[sel], bones)
    assert np.array_equal(_bits(again_p), _bits(got_p[sel])) and np.array_equal(_bits(again_n), _bits(got_n[sel]))
    # absolute: a function of the rest corners alone
    assert np.array_equal(_bits(S.corners(pos, nrm, idx, w, bones)[0]), _bits(got_p))

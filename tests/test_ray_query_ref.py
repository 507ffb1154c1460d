"""tests/ray_query_ref.py, the ray queries' definition, pinned on the CPU: hand-written expectations on a hand-made
scene, and an anchor to the oracle's path tracer (the albedo texel of a primary hit is the baseColor of the triangle
the restatement finds)."""
import numpy as np
import pytest

import oracle_ref as O
import ray_query_ref as R


@pytest.fixture(scope="module")
def handmade():
    """Two parallel quads facing +z (object 0 at z = 0, object 1 at z = -1) and two exactly coincident triangles
    (objects 2 and 3) beside them, leaves of one triangle each, so the coincident pair lies in two leaves."""
    from ptsvgf.scene import SceneBuilder, material, transform

    b = SceneBuilder()
    quad = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)
    idx = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    b.add_mesh(quad, idx, material(baseColor=(0.9, 0.1, 0.1)), transform(), False, 0)
    b.add_mesh(quad + np.float32([0, 0, -1]), idx, material(baseColor=(0.1, 0.9, 0.1)), transform(), False, 1)
    tri = np.array([[3, 0, 0], [4, 0, 0], [3.5, 1, 0]], np.float32)
    for obj in (2, 3):
        b.add_mesh(tri, np.array([[0, 1, 2]], np.int32), material(baseColor=(0.1, 0.1, 0.9)), transform(), False, obj)
    b.build(1)
    t, nd, _ = b.encode()
    assert b.counts()["max_leaf"] == 1
    return t, nd


def _find(tri_enc, obj, corner):
    """The record of object `obj` that has `corner` among its vertices (one per quad half: the corner off the diagonal)."""
    hit = [i for i in range(tri_enc.shape[0]) if tri_enc[i, 42] == obj and
           any(np.array_equal(tri_enc[i, 3 * k:3 * k + 3], np.float32(corner)) for k in range(3))]
    assert len(hit) == 1, (obj, corner, hit)
    return hit[0]


def _ray(S, d, tmax=np.inf):
    return np.array([*S, 0.0, *d, tmax], np.float32)


def test_handwritten_cases(handmade):
    tri_enc, node_enc = handmade
    w = R.Walker(tri_enc, node_enc)
    a_upper = _find(tri_enc, 0, (-1, 1, 0))    # the half of quad 0 above the diagonal y = x
    b_upper = _find(tri_enc, 1, (-1, 1, -1))
    b_lower = _find(tri_enc, 1, (1, -1, -1))
    # the coincident pair: sibling leaves with equal boxes, so hitAABB gives equal distances and the reference pushes
    # left then right (:412-415): the right child is popped, and met, first
    pair = [_find(tri_enc, o, (3.5, 1, 0)) for o in (2, 3)]
    leaf_of = {int(w.index[k]): k for k in range(1, node_enc.shape[0]) if w.n[k] == 1}
    parents = [k for k in range(1, node_enc.shape[0]) if w.n[k] == 0 and
               {int(w.left[k]), int(w.right[k])} == {leaf_of[pair[0]], leaf_of[pair[1]]}]
    assert len(parents) == 1, "the coincident triangles are sibling leaves"
    first = int(w.index[w.right[parents[0]]])
    cases = [
        # (ray, (t, tri, obj, inside, P))
        ("through both quads", _ray((0, 0.5, 1), (0.125, 0, -1)), (1.0, a_upper, 0, 0, (0.125, 0.5, 0.0))),
        ("starts on a quad: t < 0.0005 is no hit", _ray((0, 0.5, 0), (0.125, 0, -1)), (1.0, b_upper, 1, 0, (0.125, 0.5, -1.0))),
        ("back face", _ray((0.5, -0.625, -2), (0, 0.125, 1)), (1.0, b_lower, 1, 1, (0.5, -0.5, -1.0))),
        ("two exact zeros", _ray((0.25, 0.5, 1), (0, 0, -1)), (1.0, a_upper, 0, 0, (0.25, 0.5, 0.0))),
        ("scaled direction: t in units of d", _ray((0.25, 0.5, 1), (0, 0, -4)), (0.25, a_upper, 0, 0, (0.25, 0.5, 0.0))),
        ("miss", _ray((5, 5, 5), (0, 1, 0)), (114514.0, -1, -1, 0, (0.0, 0.0, 0.0))),
        ("coincident pair", _ray((3.5, 0.25, 1), (0, 0, -1)), (1.0, first, int(tri_enc[first, 42]), 0, (3.5, 0.25, 0.0))),
    ]
    rays = np.stack([c[1] for c in cases])
    got = w.hits(rays)
    for (name, _, want), g in zip(cases, got):
        exp = np.zeros(1, R.HIT_DTYPE)
        exp[0] = want
        assert np.array_equal(R.bits(g.reshape(1)), R.bits(exp)), (name, g, want)
    assert first in pair and {int(tri_enc[p, 42]) for p in pair} == {2, 3}
    # occlusion, derived: strictly before tmax, in units of t
    for tmax, want in ((np.inf, [1, 1, 1, 1, 1, 0, 1]), (1.0, [0, 0, 0, 0, 1, 0, 0]),
                       (np.nextafter(np.float32(1.0), np.float32(2.0)), [1, 1, 1, 1, 1, 0, 1]), (0.25, [0] * 7)):
        rr = rays.copy()
        rr[:, 7] = tmax
        assert w.occluded(rr, got).tolist() == [bool(v) for v in want], tmax


def test_obj_index_conversion():
    t = np.zeros((5, 45), np.float32)
    t[:, 42] = [3.75, -2.5, np.nan, np.inf, 2.0 ** 25]
    assert [R.obj_of(t, i) for i in range(5)] == [3, -2, -1, -1, -1]


def test_anchored_to_the_oracle_path_tracer(scene_cornell):
    """orc_path_trace's albedo texel of a primary hit is the baseColor (floats 21-23) of the triangle the restatement
    finds for the restated primary ray, bit for bit, wherever the 3 x 3 neighbours agree on the object (Python's
    normalize need not match the last bit on a silhouette)."""
    from ptsvgf.camera import Camera, rigid_inverse

    W, H = 32, 24
    cam = Camera(W, H)
    cam.update()
    rot = rigid_inverse(cam.cam_view_mat)
    _, _, al = O.OracleScene(scene_cornell).path_trace(W, H, 0, cam.cam_position, rot, aspect_corrected=True)
    w = R.Walker(scene_cornell.tri_enc, scene_cornell.node_enc)
    rays = np.zeros((H * W, 8), np.float32)
    rays[:, 0:3] = cam.cam_position
    rays[:, 7] = np.inf
    for y in range(H):
        for x in range(W):
            rays[y * W + x, 4:7] = R.primary_dir(rot, W, H, True, x, y)
    hits = w.hits(rays).reshape(H, W)
    obj = hits["obj"]
    hit = hits["tri"] >= 0
    pad = np.pad(obj, 1, mode="edge")
    same = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            same &= pad[dy:dy + H, dx:dx + W] == obj
    sel = hit & same
    share = sel.sum() / max(hit.sum(), 1)
    print(f"hit pixels {hit.sum()} of {H * W}, compared {sel.sum()} ({share:.2%})")
    assert hit.sum() > H * W // 4 and share >= 0.5
    want = scene_cornell.tri_enc[hits["tri"][sel], 21:24]
    assert np.array_equal(al[sel][:, :3].view(np.uint32), np.ascontiguousarray(want).view(np.uint32))

"""The predicate that decides in which cube-map cells the point-light bins list a triangle (csrc/pb_overlap.h, the
code pb_bin runs, called on the host through pt_debug_point_bins_overlap): a cell may be dropped only if no point
within fw of the projected polygon lies in it. Seeded property test over convex polygons in cell coordinates; for long
diagonal slivers the kept cells must be fewer than the box's, so the predicate is not vacuous."""
import numpy as np
import pytest

R = 64
FW = (0.02, 0.1, 0.25, 0.47)  # 0.02: the rounding term alone; 0.47: the most the build can ask for at R = 128


def _box(px, py, fw, r=R):
    """The build's first filter: the cells of the polygon's extent widened by fw, clamped to the face."""
    cx0, cx1 = max(int(np.floor(px.min() - fw)), 0), min(int(np.floor(px.max() + fw)), r - 1)
    cy0, cy1 = max(int(np.floor(py.min() - fw)), 0), min(int(np.floor(py.max() + fw)), r - 1)
    return cx0, cy0, cx1, cy1


def _convex(rng, n, kind):
    """n vertices of a convex polygon, float32, in either orientation, starting anywhere."""
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    p = np.stack([np.cos(ang), np.sin(ang)], 1)
    if kind == "sliver":  # long and thin, at any angle: a plant leaf seen obliquely
        p *= [rng.uniform(4, 20), rng.uniform(0.005, 0.4)]
    elif kind == "near_degenerate":  # thinner than float32 resolves at these magnitudes, or almost a point
        p *= [rng.choice([1e-6, 1e-3, 8.0]), rng.choice([1e-7, 1e-6, 1e-5])]
    else:
        p *= rng.uniform(0.2, 6.0, 2)
    t = rng.uniform(0, 2 * np.pi)
    p = p @ np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    p += rng.uniform(8, R - 8, 2)
    if kind == "integer":  # vertices on cell corners (rounding keeps the cyclic order; the hull is what is tested)
        p = np.round(p)
    if rng.random() < 0.5:
        p = p[::-1]
    p = np.roll(p, int(rng.integers(n)), 0)
    if kind == "duplicate":  # a clipped vertex that fell on a triangle vertex
        p[1] = p[0]
    return p.astype(np.float32)


def _points_near(rng, p, fw, count):
    """Points within fw (in x and in y, which holds every point within the distance fw) of the vertices' hull."""
    w = rng.dirichlet(np.full(len(p), 0.3), count)
    w[: len(p)] = np.eye(len(p))  # the vertices themselves
    q = w @ p.astype(np.float64)
    off = rng.uniform(-1, 1, (count, 2))
    off[: count // 4] = np.sign(off[: count // 4])  # the corners of the widening
    return q + off * fw * 0.9999


def _check(gl, p, fw, rng, count=64):
    px, py = p[:, 0], p[:, 1]
    box = _box(px, py, fw)
    kept, deg = gl.point_bins_overlap(px, py, fw, R, box)
    q = _points_near(rng, p, fw, count)
    # a ray's position lies on the face, [0, R], up to rounding (the build clips to 1 % more); half a cell is allowed
    q = q[np.all((q >= -0.5) & (q <= R + 0.5), 1)]
    cx =np.clip(np.floor(q[:, 0]).astype(int), 0, R - 1)
    cy = np.clip(np.floor(q[:, 1]).astype(int), 0, R - 1)
    assert np.all((cx >= box[0]) & (cx <= box[2]) & (cy >= box[1]) & (cy <= box[3])), (p, fw)
    ok = kept[cy - box[1], cx - box[0]]
    assert ok.all(), (p.tolist(), fw, q[~ok].tolist())
    return kept, deg


@pytest.mark.parametrize("kind", ["plain", "sliver", "near_degenerate", "integer", "duplicate"])
def test_cells_near_the_polygon_are_kept(kind):
    from ptsvgf import gl

    rng = np.random.default_rng({"plain": 1, "sliver": 2, "near_degenerate": 3, "integer": 4, "duplicate": 5}[kind])
    dropped = 0
    for it in range(400):
        n = int(rng.integers(3, 8))
        fw = FW[it % len(FW)]
        kept, _ = _check(gl, _convex(rng, n, kind), fw, rng)
        dropped += int(kept.size - kept.sum())
    print(kind, "cells dropped over 400 polygons:", dropped)


def test_edge_through_cell_corners():
    """An edge along a diagonal of cell corners: the cells it touches only in a corner are kept."""
    from ptsvgf import gl

    rng = np.random.default_rng(6)
    for p in ([[10, 10], [30, 30], [10, 30]], [[10, 10], [30, 30], [30, 30.25]], [[5, 40], [25, 20], [25.5, 20]]):
        for fw in FW:
            _check(gl, np.array(p, np.float32), fw, rng, 256)


def test_face_border_cells_take_clamped_positions():
    """A ray's cell coordinate just outside [0, R] is clamped into the border cell: a polygon in the widened rim keeps
    that cell."""
    from ptsvgf import gl

    rng = np.random.default_rng(7)
    for p in ([[-0.6, 3.2], [-0.01, 9.7], [-0.5, 9.0]], [[R + 0.01, 50], [R + 0.6, 60], [R + 0.3, 63.9]],
              [[20, R + 0.3], [30, R + 0.01], [31, R + 0.6]]):
        for fw in FW:
            _check(gl, np.array(p, np.float32), fw, rng, 256)


def test_degenerate_and_small_boxes_keep_the_box():
    from ptsvgf import gl

    line = np.array([[3, 3], [9, 9], [15, 15]], np.float32)  # zero area
    kept, deg = gl.point_bins_overlap(line[:, 0], line[:, 1], 0.25, R, _box(line[:, 0], line[:, 1], 0.25))
    assert deg and kept.all()
    two = np.array([[3, 3], [9, 9], [3, 3]], np.float32)  # two distinct vertices
    kept, deg = gl.point_bins_overlap(two[:, 0], two[:, 1], 0.25, R, _box(two[:, 0], two[:, 1], 0.25))
    assert deg and kept.all()
    nan = np.array([[3, 3], [9, np.nan], [3, 12]], np.float32)
    kept, deg = gl.point_bins_overlap(nan[:, 0], nan[:, 1], 0.25, R, (3, 3, 9, 12))
    assert deg and kept.all()
    # a sliver across two cells: both stay, though its line leaves most of each empty
    s = np.array([[4.1, 4.5], [5.9, 4.55], [5.9, 4.5]], np.float32)
    kept, deg = gl.point_bins_overlap(s[:, 0], s[:, 1], 0.02, R, (4, 4, 5, 4))
    assert not deg and kept.shape == (1, 2) and kept.all()


def test_long_diagonal_slivers_drop_most_of_the_box():
    from ptsvgf import gl

    rng = np.random.default_rng(8)
    for it in range(100):
        t = rng.uniform(np.pi / 6, np.pi / 3) + rng.integers(4) * np.pi / 2  # within 15 degrees of a diagonal
        ln, wd = rng.uniform(12, 24), rng.uniform(0.01, 0.3)
        c = rng.uniform(24, R - 24, 2)
        u, v = np.array([np.cos(t), np.sin(t)]), np.array([-np.sin(t), np.cos(t)])
        p = np.array([c - u * ln / 2, c + u * ln / 2 + v * wd, c + u * ln / 2 - v * wd], np.float32)
        kept, deg = _check(gl, p, 0.25, rng)
        assert not deg
        # the cells reached are those whose centre lies in the sliver widened by a square of side 1 + 2 fw: an area of
        # about ln (wd + 1.5 (|cos t| + |sin t|)) < 2.5 ln, against a box of about (ln |cos t| + 1.5)(ln |sin t| + 1.5)
        # > 0.43 ln^2: under half of it from ln = 12 on
        assert kept.sum() * 2 < kept.size, (p.tolist(), int(kept.sum()), kept.size)

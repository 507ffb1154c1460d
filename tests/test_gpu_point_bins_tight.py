"""The point-light bins list a triangle in the cells its projected polygon reaches (pass uniform point_bins_tight = 1,
the default; 0: every cell of the polygon's box) in 8-byte entries: the same verdict for every ray as the tree walk,
so the planes are bit-identical with either binning, and the polygon's lists are shorter than the box's."""
import numpy as np
import pytest

from test_gpu_point_bins import KEEP, _check_stats, _pt  # noqa: F401
from test_gpu_primary_tri import MOVES, _same

pytestmark = pytest.mark.gpu

W, H = 160, 96
EW, EH = 96, 64
R = 64
FLOOR_Y = -0.8
# light 0 (exact in float32) sees the slivers; they lie in the plane one unit below it, so on its -y face a world
# offset (dx, dz) has the cell coordinates ((dz + 1) 32, (dx + 1) 32) at R = 64
L0 = np.array([0.0, 1.25, 0.5])
SLIVER_LIGHTS = np.array([
    [L0[0], L0[1], L0[2], 10, 10, 10],
    [-1.5, 1.0, 1.0, 4, 3, 2],
    [1.5, 0.8, 0.0, 2, 3, 4],
    [0.3, 0.6, 1.5, 3, 3, 3],
], np.float32)
NFAN = 12


def _sliver_tris():
    """(name, three world points) of the thin triangles; every coordinate exact in float32 where it matters."""
    out = []
    y = L0[1] - 1.0
    # an edge through cell corners: cell coordinates (16, 16), (40, 40), (40, 41) from light 0
    out.append(("corners", [[-0.5, y, 0.0], [0.25, y, 0.75], [0.28125, y, 0.75]]))
    # across the edge between light 0's -y and +x faces (directions (1, -1, *))
    out.append(("two_faces", [[0.6, 0.25, 0.7], [1.4, 0.45, 0.1], [1.4, 0.47, 0.12]]))
    # 1e-3 above the floor: near sits just under the bound of the rays that start beside it
    out.append(("on_floor", [[-1.0, FLOOR_Y + 1e-3, 0.2], [-0.2, FLOOR_Y + 1e-3, 1.0], [-0.2, FLOOR_Y + 1e-3, 0.97]]))
    # a fan of long diagonal slivers a little above and below that plane: 0.9 long (29 cells), 0.012 wide
    for k in range(NFAN):
        t = np.pi / 4 + (k - NFAN / 2) * 0.05 + (np.pi / 2 if k % 2 else 0.0)
        c = np.array([-0.35 + 0.06 * k, 0.0, 0.45 + 0.02 * (k % 3)])
        u, v = np.array([np.cos(t), 0, np.sin(t)]), np.array([-np.sin(t), 0, np.cos(t)])
        yk = y + 0.01 * (k - NFAN / 2)
        p = [c - u * 0.45, c + u * 0.45 + v * 0.006, c + u * 0.45 - v * 0.006]
        out.append((f"fan{k}", [[q[0], yk, q[2]] for q in p]))
    return out


def _sliver_scene():
    """For the initial camera (eye about (0, 0.35, 1.97), looking at the origin): a floor and a back wall as
    receivers, the thin triangles of _sliver_tris between them and the lights."""
    from ptsvgf.scene import Scene, SceneBuilder, env_map, hdr_cache, material, transform

    b = SceneBuilder()
    tri = np.array([[0, 1, 2]], np.int32)
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    y = FLOOR_Y
    b.add_mesh(np.array([[-2, y, 2.5], [2, y, 2.5], [2, y, -1.5], [-2, y, -1.5]], np.float32), quad,
               material(baseColor=(0.7, 0.7, 0.7)), transform(), False, 0)
    b.add_mesh(np.array([[-2, -0.8, -1.5], [2, -0.8, -1.5], [2, 2.0, -1.5], [-2, 2.0, -1.5]], np.float32), quad,
               material(baseColor=(0.6, 0.7, 0.8)), transform(), False, 1)
    for i, (_, p) in enumerate(_sliver_tris()):
        b.add_mesh(np.array(p, np.float32), tri, material(baseColor=(0.9, 0.3, 0.2)), transform(), False, 2 + i)
    b.build(8)
    tri_enc, node, raster = b.encode()
    hdr = env_map(128, 64)
    return Scene("point_bins_slivers", tri_enc, node, raster, SLIVER_LIGHTS.copy(), hdr, hdr_cache(hdr), b.counts())


# ------------------------------------------------- the two binnings, restated in numpy ---
def _clip(poly, axis, sgn):
    """Sutherland-Hodgman against 1.01 w + sgn * (x or y) >= 0 of vertices (x, y, w)."""
    out = []
    for i in range(len(poly)):
        a, b = poly[i], poly[(i + 1) % len(poly)]
        da, db = 1.01 * a[2] + sgn * a[axis], 1.01 * b[2] + sgn * b[axis]
        if da >= 0:
            out.append(a)
        if (da >= 0) != (db >= 0):
            out.append(a + da / (da - db) * (b - a))
    return out


def _restate(tris, light, r=R, fw=0.25):
    """Entries of one light's lists when every triangle (n, 3, 3) is listed in each cell of its projected polygon's
    box widened by fw, and when only in the cells no polygon edge separates from the widened polygon: float64, fw at
    the bound the footprint term has at R = 64 (the build's is smaller)."""
    box_n = tight_n = 0
    for t in np.asarray(tris, np.float64):
        q = t - light
        for fc in range(6):
            a, sg = fc >> 1, -1.0 if fc & 1 else 1.0
            poly = [np.array([v[(a + 1) % 3], v[(a + 2) % 3], sg * v[a]]) for v in q]
            for axis, sgn in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0)):
                poly = _clip(poly, axis, sgn)
                if not poly:
                    break
            if not poly:
                continue
            p = np.array(poly)
            px, py = (p[:, 0] / p[:, 2] + 1) * 0.5 * r, (p[:, 1] / p[:, 2] + 1) * 0.5 * r
            cx0, cx1 = max(int(np.floor(px.min() - fw)), 0), min(int(np.floor(px.max() + fw)), r - 1)
            cy0, cy1 = max(int(np.floor(py.min() - fw)), 0), min(int(np.floor(py.max() + fw)), r - 1)
            if cx0 > cx1 or cy0 > cy1:
                continue
            ncell = (cx1 - cx0 + 1) * (cy1 - cy0 + 1)
            box_n += ncell
            area = sum((px[k] - px[0]) * (py[k + 1] - py[0]) - (py[k] - py[0]) * (px[k + 1] - px[0])
                       for k in range(1, len(px) - 1))
            if ncell <= 2 or abs(area) < 1e-9:
                tight_n += ncell
                continue
            cx, cy = np.meshgrid(np.arange(cx0, cx1 + 1), np.arange(cy0, cy1 + 1))
            keep = np.ones(cx.shape, bool)
            s = np.sign(area)
            for k in range(len(px)):
                k1 = (k + 1) % len(px)
                ea, eb = -s * (py[k1] - py[k]), s * (px[k1] - px[k])  # inside: ea (x - px[k]) + eb (y - py[k]) >= 0
                qx = np.where(ea >= 0, cx + 1 + fw, cx - fw)
                qy = np.where(eb >= 0, cy + 1 + fw, cy - fw)
                keep &= ea * (qx - px[k]) + eb * (qy - py[k]) >= 0
            tight_n += int(keep.sum())
    return box_n, tight_n


# ----------------------------------------------------------------------- tests ---
def test_sliver_scene(gpu):
    scene = _sliver_scene()
    named = dict(_sliver_tris())
    # the construction holds what it says, seen from light 0 on its -y face at R = 64
    c = (np.array(named["corners"]) - L0)
    assert np.array_equal((c[:, 2] / -c[:, 1] + 1) * 32, [16, 40, 40]) and \
        np.array_equal((c[:, 0] / -c[:, 1] + 1) * 32, [16, 40, 41])
    tf = np.array(named["two_faces"]) - L0
    assert (tf[0, 0] < -tf[0, 1]) and (tf[1, 0] > -tf[1, 1]), tf  # -y dominant at one end, +x at the other
    assert abs(named["on_floor"][0][1] - FLOOR_Y - 1e-3) < 1e-9
    for k in range(NFAN):
        f = np.array(named[f"fan{k}"]) - L0
        cells = np.stack([(f[:, 2] / -f[:, 1] + 1) * 32, (f[:, 0] / -f[:, 1] + 1) * 32], 1)
        assert np.all(np.ptp(cells, 0) >= 12), (k, cells)
        assert np.all(np.abs(f[:, [0, 2]]) < -f[:, [1]]), (k, f)  # wholly on the -y face
    # the restatement alone: the polygon's cells are at most half of the box's for light 0
    tris = np.array([p for _, p in _sliver_tris()])
    y = FLOOR_Y
    recv = [[[-2, y, 2.5], [2, y, 2.5], [2, y, -1.5]], [[-2, y, 2.5], [2, y, -1.5], [-2, y, -1.5]],
            [[-2, -0.8, -1.5], [2, -0.8, -1.5], [2, 2.0, -1.5]], [[-2, -0.8, -1.5], [2, 2.0, -1.5], [-2, 2.0, -1.5]]]
    box_n, tight_n = _restate(np.concatenate([np.array(recv, np.float64), tris]), L0)
    print("restated entries of light 0: box", box_n, "polygon", tight_n)
    assert 2 * tight_n <= box_n, (box_n, tight_n)

    moves = [None, (0.5, 0.25), (-1.0, -0.5)]
    for depth in (1, 2):
        want, st0 = _pt(gpu, scene, EW, EH, 0, moves, depth=depth)
        u = {"point_bins_r": R}
        got1, st1 = _pt(gpu, scene, EW, EH, 1, moves, depth=depth, uniforms={**u, "point_bins_tight": 1})
        got0, stb = _pt(gpu, scene, EW, EH, 1, moves, depth=depth, uniforms={**u, "point_bins_tight": 0})
        _same(got1, want, f"slivers/tight/depth{depth}")
        _same(got0, want, f"slivers/box/depth{depth}")
        _check_stats(st1, st0, f"slivers/tight/depth{depth}", binned_share=0.9)
        _check_stats(stb, st0, f"slivers/box/depth{depth}", binned_share=0.9)
        per1, per0 = st1["bins_info"]["per_light"], stb["bins_info"]["per_light"]
        print("entries per light: box", [q["entries"] for q in per0], "polygon", [q["entries"] for q in per1])
        assert [q["off"] for q in per1] == [0, 0, 0, 0] == [q["off"] for q in per0], (per1, per0)
        assert all(q["catch_all"] == 0 for q in per1), per1
        assert 2 * per1[0]["entries"] <= per0[0]["entries"], (per1[0], per0[0])
        assert st1["bins_info"]["entry_bytes"] == 8
        assert per1[0]["list_bytes"] == 8 * per1[0]["entries"]


def test_bench_scene_lists_shrink(gpu, scene_bench):
    want, st0 = _pt(gpu, scene_bench, W, H, 0, MOVES[:2])
    got1, st1 = _pt(gpu, scene_bench, W, H, 1, MOVES[:2], uniforms={"point_bins_tight": 1})
    _, stb = _pt(gpu, scene_bench, W, H, 1, MOVES[:1], uniforms={"point_bins_tight": 0})
    _same(got1, want, "bench/tight")
    _check_stats(st1, st0, "bench/tight", binned_share=0.9)
    per1, per0 = st1["bins_info"]["per_light"], stb["bins_info"]["per_light"]
    print("bench scene entries per light: box", [q["entries"] for q in per0], "polygon", [q["entries"] for q in per1],
          "allocated", st1["bins_info"]["bytes"], "cap", st1["bins_info"]["cap"])
    assert [q["off"] for q in per1] == [0, 0, 0, 0] == [q["off"] for q in per0]
    for a, b in zip(per1, per0):
        assert 0 < a["entries"] < b["entries"], (a, b)


@pytest.mark.parametrize("r", [32, 64, 128])
def test_other_cell_counts(gpu, scene_small, r):
    want, st0 = _pt(gpu, scene_small, W, H, 0, MOVES[:2])
    got, st1 = _pt(gpu, scene_small, W, H, 1, MOVES[:2], uniforms={"point_bins_r": r, "point_bins_tight": 1})
    _same(got, want, f"R{r}")
    _check_stats(st1, st0, f"R{r}", binned_share=0.9)
    assert st1["bins_info"]["R"] == r


def test_switching_the_binning_rebuilds(gpu, scene_small):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene_small, W, H, mode="fast", aspect_corrected=True, run_taa=False, run_output=False)
    seen = []
    for tight in (1, 0, 1):
        for p, _ in r.pt_slots:
            p.set_uniform_int("point_bins", 1)
            p.set_uniform_int("point_bins_tight", tight)
        r.frame()
        seen.append([q["entries"] for q in gpu.point_bins_info(r.trianglesTextureBuffer,
                                                                r.nodesTextureBuffer)["per_light"]])
    r.close()
    print("entries per light, tight 1 / 0 / 1:", seen)
    assert seen[0] == seen[2] and all(a < b for a, b in zip(seen[0], seen[1])), seen

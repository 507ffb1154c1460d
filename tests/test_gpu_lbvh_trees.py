"""The walk trees pt_bvh_build derives on the device (csrc/kernels_bvh.hip lbvh_trees_launch): the packed binary tree,
the leaf list and the greedy 4-wide tree of a GPU-built scene.

* Bitwise: the device stage's buffers and counters (pt_debug_lbvh_trees source 0) equal the library's host functions
  run on the host mirror of the same texels (source 1: pack_bvh, upload_leaves, pack_wide) and the Python restatement
  (tests/lbvh_trees_ref.py), on tiny, multi-block, flat-axis (zero areas: the tie rule), coincident and NaN inputs.
* Rendering a GPU-built scene through its 4-wide tree (pass uniform lbvh_wide = 1) gives the bits of the binary walk
  (lbvh_wide = 0) and of the oracle path tracer on the same buffers, with the same rays and fewer node + triangle visits.
* A rebuild in place for moved geometry replaces the trees; pt_raster_pass_bind_device, which now takes its packed
  tree from the stage, still draws the host bind's G-buffer."""
import dataclasses

import numpy as np
import pytest

import lbvh_trees_ref as T
import oracle_ref as O

pytestmark = pytest.mark.gpu

W, H = 96, 64


def _random_tris(n, seed=0, flat_axis=None):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 45), np.float32)
    t[:, :9] = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    if flat_axis is not None:
        t[:, flat_axis:9:3] = 0.5
    t[:, 42] = np.arange(n)
    return t


def _input(name):
    if name == "flat":
        return _random_tris(1000, seed=5, flat_axis=2)
    if name == "point":  # every box the same point: every area 0
        t = _random_tris(2000, seed=3)
        t[:, :9] = np.tile(np.float32([0.25, -0.5, 0.75]), 3)
        return t
    return _random_tris(int(name), seed=int(name) + 7)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _build_and_fetch(gl, tri, leaf_n, ploc):
    src = gl.texture_buffer(tri)
    to = gl.texture_buffer(np.zeros(3, np.float32))
    no = gl.texture_buffer(np.zeros(3, np.float32))
    try:
        gl.bvh_build(src, to, no, leaf_n, ploc)
        nodes = gl.buffer_readback(no).reshape(-1, 12)
        return nodes, gl.lbvh_trees(no, 0), gl.lbvh_trees(no, 1)
    finally:
        for h in (src, to, no):
            gl.destroy_texture(h)


def _check_equal(dev, host, want, wide=True):
    for name in ("binary", "leaves") + (("wide",) if wide else ()):
        assert _same(dev[name], want[name]), f"device {name} differs from the restatement"
        assert _same(host[name], want[name]), f"host {name} differs from the restatement"
    keep = 7 if wide else 3  # without the wide tree: root_ref, need, nleaves
    assert dev["info"][:keep] == want["info"][:keep], (dev["info"], want["info"])
    assert host["info"][:keep] == want["info"][:keep], (host["info"], want["info"])


@pytest.mark.parametrize("ploc", [0, 16])
@pytest.mark.parametrize("leaf_n", [1, 4])
@pytest.mark.parametrize("name", ["1", "2", "3", "5", "17", "1000", "20000", "flat", "point"])
def test_device_trees_equal_host_and_restatement(gpu, name, leaf_n, ploc):
    nodes, dev, host = _build_and_fetch(gpu, _input(name), leaf_n, ploc)
    want = T.trees(nodes)
    _check_equal(dev, host, want)
    assert dev["nan"] == 0
    if name == "1":  # a tree that is one leaf: empty trees, the root refs are the leaf ref
        assert dev["root_ref"] == dev["root4"] == -(0 * 16 + 1) - 1 and len(dev["binary"]) == len(dev["wide"]) == 0
    if name == "5" and leaf_n == 1:  # 4 interior nodes cannot fill two 4-wide nodes
        assert np.any(dev["wide"][:, 24:28].copy().view(np.int32) == T.NONE_REF)
    print(f"{name} leaf_n {leaf_n} ploc {ploc}: {len(nodes)} nodes -> {len(dev['binary'])} binary, {dev['nleaves']} "
          f"leaves, {dev['wide_nodes']} 4-wide; need {dev['need']} / {dev['need4']}; stage {dev['stage_us']} us")


def test_trees_of_an_uploaded_buffer_are_refused(gpu):
    from ptsvgf._lib import PtError
    no = gpu.texture_buffer(np.zeros(24, np.float32))
    with pytest.raises(PtError):
        gpu.lbvh_trees(no, 0)
    with pytest.raises(PtError):
        gpu.lbvh_trees(no, 1)
    gpu.destroy_texture(no)


def _nan_tris(scene):
    t = scene.tri_enc[:300].copy()
    t[[5, 77, 150], 0] = np.nan
    return t


@pytest.mark.parametrize("ploc", [0, 16])
def test_nan_vertices_set_the_flag_and_keep_binary_and_leaves(gpu, ploc):
    t = _random_tris(300, seed=9)
    t[[5, 77, 150], 0] = np.nan
    nodes, dev, host = _build_and_fetch(gpu, t, 4, ploc)
    want = T.trees(nodes)
    assert dev["nan"] == 1 and host["nan"] == 1 and want["nan"] == 1
    _check_equal(dev, host, want, wide=False)  # NaN areas order no sort: the wide buffer is not compared


def test_nan_scene_renders_as_the_binary_walk(gpu, scene_small):
    """NaN boxes: the signed 4-wide walk is not used (nan4), so lbvh_wide changes nothing."""
    from ptsvgf.renderer import Renderer

    out = []
    for wide in (1, 0):
        r = Renderer(scene_small, W, H, mode="fast", frames_in_flight=2, run_taa=False, run_output=False)
        # leaves of one triangle: a NaN triangle's own box is a child box of the 4-wide tree whatever the unions keep
        r.rebuild_bvh(tri_enc=_nan_tris(scene_small), leaf_n=1, ploc_radius=16)
        assert gpu.lbvh_trees(r.nodesTextureBuffer, 0)["nan"] == 1
        r.set_lbvh_wide(bool(wide))
        r.frame()
        out.append({k: gpu.readback(v) for k, v in r.planes().items()})
        r.close()
    for key in ("color", "emission", "albedo"):
        assert np.array_equal(out[0][key].view(np.uint32), out[1][key].view(np.uint32)), key


@pytest.mark.parametrize("leaf_n,ploc", [(8, 16), (3, 32)])
def test_wide_walk_renders_the_binary_walk_and_the_oracle(gpu, scene_small, leaf_n, ploc):
    """(3, 32) is Renderer.rebuild_bvh's default."""
    from ptsvgf.renderer import Renderer

    out, stats, bufs = [], [], None
    for wide in (1, 0):
        r = Renderer(scene_small, W, H, mode="fast", frames_in_flight=2, run_taa=False, run_output=False)
        r.rebuild_bvh(leaf_n=leaf_n, ploc_radius=ploc)
        if not wide:  # 1 is the default
            r.set_lbvh_wide(False)
        r.frame()
        out.append({k: gpu.readback(v) for k, v in r.planes().items()})
        stats.append(r.trace_stats())
        if bufs is None:
            bufs = (gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45),
                    gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12))
        r.close()
    sc = dataclasses.replace(scene_small, tri_enc=bufs[0], node_enc=bufs[1])
    want = O.OracleFrameLoop(sc, W, H, run_taa=False).frame()
    for key in ("color", "emission", "albedo"):
        assert np.array_equal(out[0][key].view(np.uint32), out[1][key].view(np.uint32)), key
        assert np.array_equal(out[0][key].view(np.uint32), want[key].view(np.uint32)), key
    for key in ("primary_rays", "bounce_rays", "shadow_rays"):
        assert stats[0][key] == stats[1][key], key
    visits = [s["bounce_visits"] + s["shadow_visits"] for s in stats]
    print(f"leaf_n {leaf_n} ploc {ploc}: bounce + shadow visits 4-wide {visits[0]}, binary {visits[1]}, "
          f"ratio {visits[0] / max(1, visits[1]):.4f}")
    assert visits[0] < visits[1]


def _moved(scene, dy):
    """The plant (objIndex 2) lifted by dy."""
    tri = scene.tri_enc.copy()
    sel = tri[:, 42] == 2.0
    for v in range(3):
        tri[sel, 3 * v + 1] += np.float32(dy)
    return tri


def test_rebuild_in_place_replaces_the_trees(gpu, scene_small):
    from ptsvgf.renderer import Renderer

    r = Renderer(scene_small, W, H, mode="fast", frames_in_flight=2, run_taa=False, run_output=False)
    r.rebuild_bvh(leaf_n=8, ploc_radius=16)
    before = gpu.lbvh_trees(r.nodesTextureBuffer, 0)
    r.frame()
    r.rebuild_bvh(tri_enc=_moved(scene_small, 0.05), leaf_n=8, ploc_radius=16)
    after = gpu.lbvh_trees(r.nodesTextureBuffer, 0)
    tri = gpu.buffer_readback(r.trianglesTextureBuffer).reshape(-1, 45)
    nodes = gpu.buffer_readback(r.nodesTextureBuffer).reshape(-1, 12)
    _check_equal(after, gpu.lbvh_trees(r.nodesTextureBuffer, 1), T.trees(nodes))
    assert not all(_same(before[k], after[k]) for k in ("binary", "leaves", "wide"))
    ref = O.OracleFrameLoop(dataclasses.replace(scene_small, tri_enc=tri, node_enc=nodes), W, H, run_taa=False)
    ref.frame()  # the oracle reaches the renderer's frame counter (static camera)
    r.frame()
    want = ref.frame()
    got = {k: gpu.readback(v) for k, v in r.planes().items()}
    for key in ("color", "emission", "albedo"):
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
    r.close()


@pytest.mark.parametrize("gbuffer_mode", [1, 0])
def test_device_raster_bind_equals_host_bind(gpu, scene_small, gbuffer_mode):
    """The G-buffer over a tree packed by the device stage (pt_raster_pass_bind_device) equals a host bind's, in the
    tile-binned rasteriser (mode 1) and the ray cast walking the tree (mode 0)."""
    from ptsvgf.renderer import Renderer

    raster = scene_small.raster.reshape(-1, 6).copy()
    raster[:, 1] += np.float32(0.03)
    tri = scene_small.tri_enc.copy()
    tri[:, [1, 4, 7]] += np.float32(0.03)
    planes = ("normal_depth", "velocity", "fwidth", "world")
    out = []
    for device in (False, True):
        sc = dataclasses.replace(scene_small, raster=raster.reshape(-1)) if not device else scene_small
        r = Renderer(sc, W, H, mode="fast", run_taa=False, run_output=False)
        if device:
            r.rebuild_bvh(tri_enc=tri, raster=raster, leaf_n=8, ploc_radius=16)
        for p in r.init_pass:
            p.set_uniform_int("gbuffer_mode", gbuffer_mode)
        r.frame()
        got = r.planes()
        out.append({k: gpu.readback(got[k]) for k in planes})
        r.close()
    for k in planes:
        assert np.array_equal(out[0][k].view(np.uint32), out[1][k].view(np.uint32)), k
    assert 0.05 < float(np.mean(out[0]["normal_depth"][..., 3] != 1.0)) < 0.95

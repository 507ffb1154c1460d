"""The three kinds of in-place edit in flight together (Renderer.set_lights, set_materials, set_environment; DESIGN.md
"Moving point lights" describes the versions they share): one renderer with three frames in flight takes all three
between frames and reads nothing until the end; its streams are released while versions of all three exist, and the
textures that own them are destroyed right after.

The yardstick is one fresh renderer constructed with the final lights, materials and map, every cache and the bins
off, brought to the same frame counter: the path tracer's planes of a frame depend on the scene and the frame counter
alone (the three features' own tests compare against such renderers too), so the readback-per-frame rerun is not
needed."""
import dataclasses

import numpy as np
import pytest

from materials_ref import materials_ref
from test_gpu_environment import _all_off, _maps, _own, _read, _renderer
from test_gpu_primary_tri import _same

pytestmark = pytest.mark.gpu

NF = 6  # frames of the scenario: 0 1 | light moved, object 1 recoloured, map A | 2 | map B, light back | 3 4 5
K = 3   # frames in flight


def _final(scene, tri, hdr):
    """A scene of the test's own with these triangles and this map (and its cache); the lights are the fixture's."""
    return dataclasses.replace(_own(scene, hdr), tri_enc=tri.copy(), lights=scene.lights.copy())


def _frames(gl, scene, upto):
    """Frames 0 .. upto of a fresh renderer on `scene`, every cache and the bins off, each read back as it is drawn."""
    r = _renderer(scene)
    _all_off(r)
    out = []
    for _ in range(upto + 1):
        r.frame()
        out.append(_read(gl, r))
    r.close()
    return out


def test_three_edits_in_flight_and_the_teardown(gpu, scene_small):
    from ptsvgf.scene import material

    m0, a, b = _maps(scene_small)
    moved = scene_small.lights.copy()
    moved[1, :3] = np.float32([-0.3, 0.9, 0.4])
    colour = material(baseColor=(0.15, 0.35, 0.9), roughness=0.15, metallic=0.2)
    tri = materials_ref(scene_small.tri_enc, 1, colour[None])

    want = _frames(gpu, _final(scene_small, tri, b), NF - 1)
    # the edits that stand at the end are visible at all: without either, the yardstick's frame 3 is another
    for other in (_final(scene_small, scene_small.tri_enc, b), _final(scene_small, tri, m0)):
        assert not np.array_equal(want[3]["color"], _frames(gpu, other, 3)[3]["color"])

    r = _renderer(_own(scene_small), frames_in_flight=K)
    for f in range(NF):
        if f == 2:
            r.set_lights(moved[1:2], first=1)
            r.set_materials({1: colour})
            r.set_environment(a)
        if f == 3:
            r.set_environment(b)
            r.set_lights(scene_small.lights[1:2], first=1)
        r.frame()
    r.flush()
    gpu.sync()
    _same([_read(gpu, r, f) for f in range(NF - K, NF)], want[NF - K:], "in flight")
    # the bounds of the three steady-state tests for K frames in flight
    lights = gpu.lights_state(r.pointLightBuffer)
    mats = gpu.materials_state(r.trianglesTextureBuffer, r.nodesTextureBuffer)
    env = gpu.environment_state(r.hdrMap)
    print(lights, mats, env)
    assert 2 <= lights["device_versions"] <= 6, lights
    assert 2 <= mats["device_versions"] <= K + 2, mats
    assert 2 <= env["device_versions"] <= K + 2, env
    # the renderer kept its scene in step
    sc = r.scene
    assert np.array_equal(sc.lights, scene_small.lights)
    assert np.array_equal(sc.tri_enc.view(np.uint32), tri.view(np.uint32))
    assert np.array_equal(sc.hdr.view(np.uint32), b.view(np.uint32))

    # close() releases the renderer's streams first (release_stream: every reader event of theirs is forgotten while
    # the versions of all three exist), then destroys the textures that own the versions
    r.close()
    again = _renderer(_own(sc, sc.hdr), frames_in_flight=K)  # (set_environment dropped the scene's cache)
    again.frame()
    _same([_read(gpu, again)], want[:1], "after the teardown")
    again.close()

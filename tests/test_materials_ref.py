"""Material edits, the definition (tests/materials_ref.py): patching the material floats of an encoded scene gives
the encoding of the scene built with those materials, tree included. That is what makes a fresh renderer on the
patched buffer the yardstick of tests/test_gpu_materials.py."""
import numpy as np

from materials_ref import materials_ref


def _scene(mat1):
    from ptsvgf.scene import SceneBuilder, gen_cornell, gen_teapot, material, transform

    b = SceneBuilder()
    cpos, cidx = gen_cornell()
    b.add_mesh(cpos, cidx, material(baseColor=(0.73, 0.73, 0.73), roughness=0.8), transform(), False, 0)
    tpos, tidx = gen_teapot(12)
    b.add_mesh(tpos, tidx, mat1, transform(trans=(0.0, -1.0, 0.0), scale=(0.9, 0.9, 0.9)), True, 1)
    b.build(8)
    tri, node, _ = b.encode()
    return tri, node


def test_reference_equals_a_fresh_encode():
    from ptsvgf.materials import apply_materials
    from ptsvgf.scene import material

    china = material(baseColor=(0.85, 0.85, 0.80), roughness=0.25, clearcoat=1.0, clearcoatGloss=0.9)
    lamp = material(baseColor=(0.2, 0.7, 0.9), emissive=(3.0, 2.0, 1.0), roughness=0.6, metallic=0.4)
    tri_a, node_a = _scene(china)
    tri_b, node_b = _scene(lamp)
    assert np.array_equal(node_a.view(np.uint32), node_b.view(np.uint32))
    assert not np.array_equal(tri_a.view(np.uint32), tri_b.view(np.uint32))
    got = materials_ref(tri_a, 1, lamp[None])
    assert np.array_equal(got.view(np.uint32), tri_b.view(np.uint32))
    # the package's own patch (Renderer.set_materials keeps scene.tri_enc in step with it) is the same function
    assert np.array_equal(apply_materials(tri_a, 1, lamp[None]).view(np.uint32), tri_b.view(np.uint32))
    # a range of two objects in one call, and back again
    white = materials_ref(tri_b, 0, np.stack([lamp, china]))
    assert np.array_equal(white[white[:, 42] == 0, 18:36], np.tile(lamp, (int((white[:, 42] == 0).sum()), 1)))
    assert np.array_equal(white[white[:, 42] == 1].view(np.uint32), tri_a[tri_a[:, 42] == 1].view(np.uint32))
    assert tri_a.dtype == got.dtype and tri_a.shape == got.shape
    assert np.array_equal(materials_ref(tri_a.reshape(-1), 1, lamp).reshape(-1, 45).view(np.uint32),
                          tri_b.view(np.uint32))  # flat in, flat out


def test_records_of_no_object_keep_their_bits():
    from ptsvgf.materials import apply_materials

    rng = np.random.default_rng(7)
    tri = rng.standard_normal((12, 45)).astype(np.float32)
    odd = np.float32([0.5, -1.0, np.nan, 1.0000001, 3.0, -0.0, 2.5, np.inf, 7.0, 1.0, 2.0, 0.0])
    tri[:, 42] = odd
    tri.view(np.uint32)[2, 42] = 0x7FC12345  # a NaN with a payload
    mats = rng.standard_normal((3, 18)).astype(np.float32)  # objects 0, 1, 2
    for fn in (materials_ref, apply_materials):
        out = fn(tri, 0, mats)
        named = {11: 0, 5: 0, 9: 1, 10: 2}  # -0.0 == float32(0); 1.0000001 is not 1
        for i in range(12):
            if i in named:
                assert np.array_equal(out[i, 18:36], mats[named[i]]), (fn.__name__, i)
                keep = np.r_[0:18, 36:45]
                assert np.array_equal(out.view(np.uint32)[i, keep], tri.view(np.uint32)[i, keep])
            else:
                assert np.array_equal(out.view(np.uint32)[i], tri.view(np.uint32)[i]), (fn.__name__, i)
        assert np.array_equal(tri[:, 42].view(np.uint32), out[:, 42].view(np.uint32))
    # first_obj offsets the table: objects 2 and 3
    out = materials_ref(tri, 2, mats[:2])
    assert np.array_equal(out[10, 18:36], mats[0]) and np.array_equal(out[4, 18:36], mats[1])
    assert np.array_equal(out.view(np.uint32)[9], tri.view(np.uint32)[9])

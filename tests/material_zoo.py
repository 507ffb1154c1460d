"""The material zoo: a Cornell box holding twelve small teapots, one per corner of the Disney BRDF's parameter space
(BRDF_Evaluate, path_tracing.frag:620-669; SampleBRDF :753-784; shade :948-968) that no other scene of the suite reaches:
a black base colour (the Cdlum <= 0 fallback of Ctint), metallic 1 (no diffuse lobe: p_diffuse = 0), roughness 0 (the
alpha = max(0.001, r^2) clamp) and 1, subsurface 1, full specular / sheen tints, clearcoatGloss at both ends of
mix(0.1, 0.001, gloss), and a black emitter (shade's BRDF-sampled emission term, with albedo 0 downstream in SVGF).

Built through the host scene library only, so the CPU tests use it too. TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

# object -> (name, material() keywords); unlisted parameters keep material()'s defaults
ZOO = {
    1: ("black_tint", dict(baseColor=(0.0, 0.0, 0.0), specular=1.0, specularTint=1.0, sheen=1.0, sheenTint=1.0)),
    2: ("mirror", dict(baseColor=(0.9, 0.8, 0.5), metallic=1.0, roughness=0.0)),
    3: ("metal_rough1", dict(baseColor=(0.9, 0.8, 0.5), metallic=1.0, roughness=1.0)),
    4: ("subsurface1", dict(baseColor=(0.8, 0.4, 0.3), subsurface=1.0, roughness=1.0)),
    5: ("ss_sheen", dict(baseColor=(0.3, 0.5, 0.8), subsurface=0.5, roughness=0.3, sheen=1.0, sheenTint=0.0)),
    6: ("spec_tint", dict(baseColor=(0.9, 0.1, 0.1), specular=1.0, specularTint=1.0, roughness=0.2)),
    7: ("coat_gloss0", dict(baseColor=(0.2, 0.6, 0.3), clearcoat=1.0, clearcoatGloss=0.0, roughness=0.6)),
    8: ("coat_metal", dict(baseColor=(0.7, 0.7, 0.2), clearcoat=1.0, clearcoatGloss=1.0, metallic=1.0, roughness=0.4)),
    9: ("emissive_black", dict(baseColor=(0.0, 0.0, 0.0), emissive=(2.0, 1.0, 0.5))),
    10: ("nospec_smooth", dict(baseColor=(0.6, 0.6, 0.6), specular=0.0, roughness=0.05)),
    11: ("blue", dict(baseColor=(0.0, 0.0, 1.0), specularTint=0.5, sheen=0.5, sheenTint=1.0)),
    12: ("mid", dict(baseColor=(0.5, 0.4, 0.3), subsurface=0.3, metallic=0.4, specular=0.6, specularTint=0.3,
                     roughness=0.45, sheen=0.4, sheenTint=0.6, clearcoat=0.5, clearcoatGloss=0.5)),
}
BOX = dict(baseColor=(0.73, 0.73, 0.73), roughness=0.8)  # object 0
OBJECTS = tuple(range(1, 13))
NAMES = {k: v[0] for k, v in ZOO.items()}
DEAD = dict(anisotropic=0.7, IOR=1.5, transmission=0.6)  # parameters the shader decodes and never reads


def zoo_params(k: int, ids: bool = False, override=None) -> dict:
    """material()'s keywords of object k (0: the box)."""
    kw = dict(BOX if k == 0 else ZOO[k][1])
    if ids:
        kw["baseColor"] = (k / 16.0, 1.0, 0.0)
        kw.pop("emissive", None)
    kw.update((override or {}).get(k, {}))
    return kw


def zoo_material(k: int, ids: bool = False, override=None) -> np.ndarray:
    from ptsvgf.scene import material

    return material(**zoo_params(k, ids, override))


def zoo_edges(ids: bool = False, override=None):
    """The scene. ids: object k has the base colour (k / 16, 1, 0) and no emission, so the albedo plane names the
    object (two of the zoo's base colours are black). override: {object: {parameter: value}} on top of the table."""
    from ptsvgf.scene import POINT_LIGHTS, Scene, SceneBuilder, env_map, gen_cornell, gen_teapot, hdr_cache, transform

    b = SceneBuilder()
    cpos, cidx = gen_cornell()
    b.add_mesh(cpos, cidx, zoo_material(0, ids, override), transform(), False, 0)
    tpos, tidx = gen_teapot(8)
    k = 1
    for i in range(4):
        for j in range(3):
            b.add_mesh(tpos, tidx, zoo_material(k, ids, override),
                       transform(trans=(-0.95 + 0.62 * i, -0.55 + 0.5 * j, 0.9), scale=(0.4, 0.4, 0.4)), True, k)
            k += 1
    b.build(8)
    tri, node, raster = b.encode()
    hdr = env_map(64, 32)
    return Scene("zoo_edges", tri, node, raster, POINT_LIGHTS.copy(), hdr, hdr_cache(hdr), b.counts(), None,
                 b.raster_objects())


def camera(W: int, H: int):
    """(eye, cameraRotate) of the default camera."""
    from ptsvgf.camera import Camera, rigid_inverse

    cam = Camera(W, H)
    cam.update()
    return cam.cam_position, rigid_inverse(cam.cam_view_mat)


def object_masks(W: int, H: int) -> np.ndarray:
    """(H, W) int: the object of each pixel's primary hit at the default camera (aspect-corrected ray), -1 on a miss:
    the oracle's albedo plane of the ids scene."""
    import oracle_ref as O

    eye, rot = camera(W, H)
    _, _, al = O.OracleScene(zoo_edges(ids=True)).path_trace(W, H, 0, eye, rot, aspect_corrected=True)
    obj = np.rint(al[..., 0].astype(np.float64) * 16.0).astype(np.int64)
    return np.where(al[..., 1] == 1.0, obj, -1)

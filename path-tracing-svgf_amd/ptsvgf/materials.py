"""Material edits on the host: what pt_materials_update does to Triangle_encoded rows (tests/materials_ref.py
restates the definition), and the hue turn render_cli --hue-cycle applies."""
from __future__ import annotations

import colorsys

import numpy as np

MATERIAL0, MATERIAL_FLOATS, OBJ_INDEX = 18, 18, 42  # floats 18 .. 35 of a 45-float row; the objIndex float


def apply_materials(tri_enc, first_obj: int, materials) -> np.ndarray:
    """A copy of `tri_enc` ((n, 45) float32, or flat) in which the rows of object first_obj + k hold materials[k]
    ((count, 18) float32). A row belongs to object o when its objIndex compares == float32(o); every other bit of the
    array is kept."""
    src = np.asarray(tri_enc, dtype=np.float32)
    out = np.array(src, dtype=np.float32, copy=True).reshape(-1, 45)
    mats = np.ascontiguousarray(materials, dtype=np.float32).reshape(-1, MATERIAL_FLOATS)
    obj = out[:, OBJ_INDEX].copy()
    for k in range(mats.shape[0]):
        out[obj == np.float32(first_obj + k), MATERIAL0:MATERIAL0 + MATERIAL_FLOATS] = mats[k]
    return out.reshape(src.shape)


def object_material(tri_enc, obj: int) -> np.ndarray:
    """The 18 material floats of object `obj`'s first row."""
    rows = np.asarray(tri_enc, dtype=np.float32).reshape(-1, 45)
    hit = np.nonzero(rows[:, OBJ_INDEX] == np.float32(obj))[0]
    if hit.size == 0:
        raise ValueError(f"no triangle of object {obj}")
    return rows[hit[0], MATERIAL0:MATERIAL0 + MATERIAL_FLOATS].copy()


def hue_turned(material18, degrees: float, base_color_at: int = 3) -> np.ndarray:
    """`material18` with the hue of its constant baseColor (floats base_color_at .. + 2) turned by `degrees`; a
    negative (texture-layer) or grey baseColor has no hue and gets a saturated one first."""
    m = np.array(material18, dtype=np.float32, copy=True)
    r, g, b = (float(max(v, 0.0)) for v in m[base_color_at:base_color_at + 3])
    h, s, v = colorsys.rgb_to_hsv(min(r, 1.0), min(g, 1.0), min(b, 1.0))
    if s < 0.25:
        s, v = 0.8, max(v, 0.6)
    m[base_color_at:base_color_at + 3] = colorsys.hsv_to_rgb((h + degrees / 360.0) % 1.0, s, v)
    return m

"""The definition of pt_materials_update (DESIGN.md "Material edits"), in numpy: what the call does to a buffer of
Triangle_encoded records. A record is 45 floats; floats 18 .. 35 are its material (ptsvgf_scene.h's order), float 42
its objIndex. The records of object first_obj + k take materials[k]; a record belongs to object o when its objIndex
compares == float32(o), so a fraction, a negative value or a NaN names no object. Every other bit stays."""
import numpy as np


def materials_ref(tri_enc, first_obj, materials):
    tri = np.array(tri_enc, dtype=np.float32, copy=True).reshape(-1, 45)
    mats = np.asarray(materials, dtype=np.float32).reshape(-1, 18)
    bits = tri.view(np.uint32)  # moved as bits: a NaN payload in a material survives
    obj = tri[:, 42].copy()
    with np.errstate(invalid="ignore"):
        for k in range(mats.shape[0]):
            bits[obj == np.float32(first_obj + k), 18:36] = mats[k].view(np.uint32)
    return tri.reshape(np.shape(tri_enc))

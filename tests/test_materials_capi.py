"""pt_materials_update at the drop-in boundary, on a host without a device: the entry points exist in the library,
the headers and the bindings, and the argument errors that need no device are reported."""
import ctypes as C
import os
import re

import pytest

from ptsvgf import _lib

NEW = {
    "ptsvgf.h": ["pt_materials_update"],
    "ptsvgf_debug_materials.h": ["pt_debug_materials_state"],
}


def _declared(header):
    txt = open(os.path.join(_lib.INCLUDE_DIR, header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(pt_\w+)\s*\(", txt))


@pytest.mark.parametrize("header", sorted(NEW))
def test_declared_exported_and_bound(header):
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    bound, _ = _lib.exported_symbols()
    declared = _declared(header)
    for name in NEW[header]:
        assert name in declared, (header, name)
        assert hasattr(lib, name), name
        assert name in bound, name
    if header == "ptsvgf_debug_materials.h":
        assert declared == set(NEW[header])


def test_argument_errors_need_no_device():
    L = _lib.pt()
    data = (C.c_float * 36)()
    assert L.pt_materials_update(1, 0, 0, 1, None) == -6  # PT_ERR_ARG: null data
    assert b"pt_materials_update" in L.pt_last_error()
    assert L.pt_materials_update(1, 0, 0, 0, data) == -6  # count in [1, 4096]
    assert L.pt_materials_update(1, 0, 0, -1, data) == -6
    assert L.pt_materials_update(1, 0, 0, 4097, data) == -6
    assert L.pt_materials_update(1, 0, -1, 1, data) == -6  # first_obj >= 0
    assert L.pt_materials_update(1, 0, 1 << 24, 1, data) == -6  # an object index no float encodes exactly
    assert L.pt_materials_update(1, 0, 2**31 - 1, 2, data) == -6


def test_update_before_init_fails_loudly():
    L = _lib.pt()
    h = C.c_uint32()
    if L.pt_texture2d_create(4, 4, C.byref(h)) == 0:
        pytest.skip("library already initialised in this process")
    data = (C.c_float * 18)()
    assert L.pt_materials_update(1, 0, 0, 1, data) == -9  # PT_ERR_STATE
    assert b"pt_init" in L.pt_last_error()
    n = C.c_int()
    assert L.pt_debug_materials_state(1, 2, None, C.byref(n), None) == -9

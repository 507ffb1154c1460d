"""pt_lights_update at the drop-in boundary, on a host without a device: the entry points exist in the library, the
headers and the bindings, and the argument errors that need no device are reported."""
import ctypes as C
import os
import re

import pytest

from ptsvgf import _lib

NEW = {
    "ptsvgf.h": ["pt_lights_update"],
    "ptsvgf_debug_lights.h": ["pt_debug_lights_moved_mask", "pt_debug_lights_settle", "pt_debug_lights_key_mode",
                              "pt_debug_lights_key_field", "pt_debug_lights_state"],
    "ptsvgf_debug_static.h": ["pt_debug_point_cache_forgotten"],
    "ptsvgf_debug_pointbins.h": ["pt_debug_point_bins_read"],
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
    # every entry point the debug header declares is exported and bound
    if header == "ptsvgf_debug_lights.h":
        assert declared == set(NEW[header])


def test_argument_errors_need_no_device():
    L = _lib.pt()
    data = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    assert L.pt_lights_update(1, 0, 1, None) == -6  # PT_ERR_ARG: null data
    assert b"pt_lights_update" in L.pt_last_error()
    assert L.pt_lights_update(1, -1, 1, data) == -6  # a range that starts before the buffer
    assert L.pt_lights_update(1, 0, -1, data) == -6


def test_update_before_init_fails_loudly():
    L = _lib.pt()
    h = C.c_uint32()
    if L.pt_texture2d_create(4, 4, C.byref(h)) == 0:
        pytest.skip("library already initialised in this process")
    data = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    assert L.pt_lights_update(1, 0, 1, data) == -9  # PT_ERR_STATE
    assert b"pt_init" in L.pt_last_error()
    m = C.c_uint32()
    assert L.pt_debug_point_cache_forgotten(1, C.byref(m)) == -1  # PT_ERR_INVALID_HANDLE: no such pass


def test_debug_entries_check_their_arguments():
    L = _lib.pt()
    m = C.c_uint32()
    assert L.pt_debug_lights_moved_mask(None, 4, 0, C.byref(m)) == -6
    assert L.pt_debug_lights_settle(None, 1, 0, None) == -6
    assert L.pt_debug_lights_key_field(5) == -6
    out = C.c_uint32()
    assert L.pt_debug_point_cache_word(6, 0, 0, C.byref(out)) == -6  # op 5 (forget) is the last
    assert L.pt_debug_point_cache_word(5, 0x0FF, 0xF, C.byref(out)) == 0 and out.value == 0

"""pt_environment_update at the drop-in boundary, on a host without a device: the entry points exist in the library,
the headers and the bindings, and the argument errors that need no device are reported."""
import ctypes as C
import os
import re

import pytest

from ptsvgf import _lib

NEW = {
    "ptsvgf.h": ["pt_environment_update"],
    "ptsvgf_debug_environment.h": ["pt_debug_environment_state"],
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
    if header == "ptsvgf_debug_environment.h":
        assert declared == set(NEW[header])


def test_python_surface():
    from ptsvgf import gl, render_cli
    from ptsvgf.renderer import Renderer

    assert callable(gl.environment_update) and callable(gl.environment_state)
    assert callable(Renderer.set_environment)
    assert render_cli.sky_shift(0, 30.0, 256) == 0
    assert render_cli.sky_shift(3, 30.0, 256) == 64
    assert render_cli.sky_shift(1, -45.0, 128) == -16


def test_argument_errors_need_no_device():
    L = _lib.pt()
    data = (C.c_float * 12)()
    assert L.pt_environment_update(1, 2, None, 2, 2, 0) == -6  # PT_ERR_ARG: null data
    assert b"pt_environment_update" in L.pt_last_error()
    assert L.pt_environment_update(1, 1, data, 2, 2, 0) == -6  # one texture for both
    for w, h in ((0, 2), (2, 0), (-1, 2), (8193, 2), (2, 8193)):
        assert L.pt_environment_update(1, 2, data, w, h, 0) == -6, (w, h)
        assert L.pt_environment_update(1, 2, data, w, h, 1) == -6, (w, h)


def test_update_before_init_fails_loudly():
    L = _lib.pt()
    h = C.c_uint32()
    if L.pt_texture2d_create(4, 4, C.byref(h)) == 0:
        pytest.skip("library already initialised in this process")
    data = (C.c_float * 12)()
    assert L.pt_environment_update(1, 2, data, 2, 2, 0) == -9  # PT_ERR_STATE
    assert b"pt_init" in L.pt_last_error()
    assert L.pt_debug_environment_state(1, None, None, None) == -9

"""The ray queries at the drop-in boundary, on a host without a device: the entry points exist in the library, the
headers and the bindings, and the argument errors that need no device are reported."""
import ctypes as C
import os
import re

import pytest

from ptsvgf import _lib

NEW = {
    "ptsvgf.h": ["pt_rays_closest", "pt_rays_occluded", "pt_rays_primary"],
    "ptsvgf_debug_rays.h": ["pt_debug_rays_variant", "pt_debug_rays_state"],
}
ARG, STATE = -6, -9


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
    if header == "ptsvgf_debug_rays.h":
        assert declared == set(NEW[header])


def test_header_states_the_section_and_the_refit_rule():
    txt = open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf.h")).read()
    assert "ray queries (no GL counterpart)" in txt
    sec = txt[txt.index("ray queries (no GL counterpart)"):txt.index("int pt_rays_primary(")]
    assert "no query in flight" in sec and "pt_bvh_refit" in sec and "pt_pose_apply" in sec


def test_argument_errors_need_no_device():
    L = _lib.pt()
    ok = C.c_void_p(4096)  # aligned, never dereferenced: every check below fails before the device is looked at
    for fn in (L.pt_rays_closest, L.pt_rays_occluded):
        name = fn.__name__.encode()
        assert fn(1, 2, None, 1, ok) == ARG  # null rays with n > 0
        assert name in L.pt_last_error()
        assert fn(1, 2, ok, 1, None) == ARG  # null output with n > 0
        assert fn(1, 2, ok, -1, ok) == ARG
        assert fn(1, 2, ok, (1 << 28) + 1, ok) == ARG
        assert fn(1, 2, C.c_void_p(4096 + 8), 1, ok) == ARG  # rays not 16-byte aligned
    assert L.pt_rays_closest(1, 2, ok, 1, C.c_void_p(4096 + 4)) == ARG  # hit records not 16-byte aligned
    eye = (C.c_float * 3)()
    rot = (C.c_float * 16)()
    assert L.pt_rays_primary(None, rot, 4, 4, 0, None, 16, ok) == ARG
    assert L.pt_rays_primary(eye, None, 4, 4, 0, None, 16, ok) == ARG
    assert L.pt_rays_primary(eye, rot, 0, 4, 0, None, 0, ok) == ARG  # width < 1
    assert L.pt_rays_primary(eye, rot, 4, -1, 0, None, 0, ok) == ARG
    assert L.pt_rays_primary(eye, rot, 4, 4, 0, None, -1, ok) == ARG
    assert L.pt_rays_primary(eye, rot, 4, 4, 0, ok, (1 << 28) + 1, ok) == ARG
    assert L.pt_rays_primary(eye, rot, 4, 4, 0, None, 16, None) == ARG  # null output with n > 0
    assert L.pt_rays_primary(eye, rot, 4, 4, 0, None, 16, C.c_void_p(4096 + 8)) == ARG  # alignment
    assert L.pt_rays_primary(eye, rot, 4, 4, 0, None, 15, ok) == ARG  # every pixel: n must be width * height
    assert b"pt_rays_primary" in L.pt_last_error()
    assert L.pt_debug_rays_variant(2) == ARG
    assert L.pt_debug_rays_variant(-1) == 0


def test_query_before_init_fails_loudly():
    L = _lib.pt()
    h = C.c_uint32()
    if L.pt_texture2d_create(4, 4, C.byref(h)) == 0:
        pytest.skip("library already initialised in this process")
    ok = C.c_void_p(4096)
    assert L.pt_rays_closest(1, 2, ok, 1, ok) == STATE
    assert b"pt_init" in L.pt_last_error()
    assert L.pt_rays_occluded(1, 2, ok, 1, ok) == STATE
    assert L.pt_rays_closest(1, 2, ok, 0, ok) == STATE  # n == 0 is PT_OK only on an initialised library
    eye, rot = (C.c_float * 3)(), (C.c_float * 16)()
    assert L.pt_rays_primary(eye, rot, 4, 4, 0, None, 16, ok) == STATE
    assert L.pt_debug_rays_state(None, None, None, None) == STATE

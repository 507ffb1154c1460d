"""The skin's entry points at the drop-in boundary: declared by include/ptsvgf.h, exported by the library, bound by
ptsvgf._lib."""
import ctypes as C
import os
import re

from ptsvgf import _lib

NAMES = ("pt_pose_set_skin", "pt_pose_apply_skin")


def test_header_declares_the_skin_entry_points():
    txt = open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name


def test_library_exports_the_skin_entry_points():
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    for name in NAMES:
        assert hasattr(lib, name), name


def test_bindings_list_the_skin_entry_points():
    pt_names, _ = _lib.exported_symbols()
    for name in NAMES:
        assert name in pt_names
    # and bind: eight arguments for the apply, as pt_pose_apply
    sigs = {n: args for n, _, args in _lib._PT_SIGS}
    assert len(sigs["pt_pose_apply_skin"]) == len(sigs["pt_pose_apply"]) == 8
    assert len(sigs["pt_pose_set_skin"]) == 5

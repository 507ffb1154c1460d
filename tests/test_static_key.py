"""The keys of the static-view reuse (csrc/static_key.h, DESIGN.md "Static view"), through the host-only entry points
of include/ptsvgf_debug_static.h: a key is one 64-bit word per field, a draw may reuse an earlier draw's work only when
every word is equal, and the switches that bypass the reuse do. No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ptsvgf import _lib

NAMES = ("pt_debug_stage_counts", "pt_debug_static_key_words", "pt_debug_static_key_diff", "pt_debug_static_key_hit")
KINDS = (0, 1)  # the primary stage's key, the G-buffer draw's


@pytest.fixture(scope="module")
def gl():
    from ptsvgf import gl

    return gl


def _key(gl, kind, seed=0):
    """A key with every word non-zero (a G-buffer key needs its compact planes present and valid to be reused)."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 2**63, gl.static_key_words(kind), dtype=np.uint64)


@pytest.mark.parametrize("kind", KINDS)
def test_equal_keys_hit(gl, kind):
    k = _key(gl, kind)
    assert len(k) > 30
    assert gl.static_key_diff(kind, k, k.copy()) == -1
    assert gl.static_key_hit(kind, k, True, k.copy(), True)


@pytest.mark.parametrize("kind", KINDS)
def test_every_field_enters_the_compare(gl, kind):
    """Each word flipped alone: in its lowest bit, in its highest, and to zero."""
    k = _key(gl, kind)
    for i in range(len(k)):
        for flip in (k[i] ^ np.uint64(1), k[i] ^ np.uint64(1 << 63), np.uint64(0)):
            q = k.copy()
            q[i] = flip
            assert gl.static_key_diff(kind, k, q) == i, i
            assert gl.static_key_diff(kind, q, k) == i, i
            assert not gl.static_key_hit(kind, k, True, q, True), i


@pytest.mark.parametrize("kind", KINDS)
def test_first_difference_is_reported(gl, kind):
    k = _key(gl, kind)
    q = k.copy()
    q[5] ^= np.uint64(2)
    q[len(k) - 1] ^= np.uint64(2)
    assert gl.static_key_diff(kind, k, q) == 5


@pytest.mark.parametrize("kind", KINDS)
def test_bypasses(gl, kind):
    """No completed draw behind the key, or the switch off (primary_cache = 0, trace statistics or row costs bound;
    reuse_static = 0, a motion bound bound): the work is done again whatever the keys say."""
    k = _key(gl, kind)
    assert not gl.static_key_hit(kind, k, False, k, True)
    assert not gl.static_key_hit(kind, k, True, k, False)


def test_gbuffer_needs_its_compact_planes(gl):
    """Equal keys are not enough for the G-buffer: the compact planes the draw writes must be there and valid. With
    bound_eye set that is four words (two pointers, two valid flags); with that one word zero (no bound_eye) only the
    fwidth attachment's two. The primary key has no such word."""
    def must_be_set(kind, also_zero=None):
        k = _key(gl, kind)
        if also_zero is not None:
            k[also_zero] = 0
        out = []
        for i in range(len(k)):
            q = k.copy()
            q[i] = 0
            if not gl.static_key_hit(kind, q, True, q, True):
                out.append(i)
        return out

    assert must_be_set(0) == []
    need = must_be_set(1)
    assert len(need) == 4
    fewer = {j: must_be_set(1, j) for j in range(gl.static_key_words(1)) if j not in need}
    switch = [j for j, n in fewer.items() if n != need]
    assert len(switch) == 1  # the word "bound_eye is set"
    assert len(fewer[switch[0]]) == 2 and set(fewer[switch[0]]) < set(need)


# ------------------------------------------------------------ the entry points' arguments ---
def test_header_declares_the_entry_points():
    txt = open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf_debug_static.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name


def test_library_exports_and_bindings_list_them():
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    pt_names, _ = _lib.exported_symbols()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in pt_names


def test_argument_checks(gl):
    pt = _lib.pt()
    ARG, HANDLE = -6, -1  # PT_ERR_ARG, PT_ERR_INVALID_HANDLE (include/ptsvgf.h)
    u64p = C.POINTER(C.c_uint64)
    for kind in (-1, 2):
        assert pt.pt_debug_static_key_words(kind) == ARG
    for kind in KINDS:
        n = gl.static_key_words(kind)
        k = _key(gl, kind)
        p = k.ctypes.data_as(u64p)
        f = C.c_int(7)
        assert pt.pt_debug_static_key_diff(kind, p, p, n, C.byref(f)) == 0 and f.value == -1
        assert pt.pt_debug_static_key_diff(kind, None, p, n, C.byref(f)) == ARG
        assert pt.pt_debug_static_key_diff(kind, p, None, n, C.byref(f)) == ARG
        assert pt.pt_debug_static_key_diff(kind, p, p, n, None) == ARG
        assert pt.pt_debug_static_key_diff(kind, p, p, n - 1, C.byref(f)) == ARG  # another kind's (or no kind's) size
        assert pt.pt_debug_static_key_diff(2, p, p, n, C.byref(f)) == ARG
        assert pt.pt_debug_static_key_hit(kind, p, 1, p, n, 1, None) == ARG
        assert pt.pt_debug_static_key_hit(kind, None, 1, p, n, 1, C.byref(f)) == ARG
        assert pt.pt_debug_static_key_hit(kind, p, 1, p, n + 1, 1, C.byref(f)) == ARG
        assert b"pt_debug_static_key_hit" in pt.pt_last_error()
    assert gl.static_key_words(0) != gl.static_key_words(1)
    r, u = C.c_uint64(), C.c_uint64()
    assert pt.pt_debug_stage_counts(0xFFFFFFF0, C.byref(r), C.byref(u)) == HANDLE

"""The bounce-0 point-light verdict cache's host side (DESIGN.md "Static view, part 2"), through the entry points of
include/ptsvgf_debug_static.h: the bit layout of the per-pixel word (csrc/point_cache.h: bits 0-3 verdict known for
light i, bits 4-7 light i occluded, bits 8-10 the pending light + 1) and the cache's key and mode rule
(csrc/static_key.h). No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ptsvgf import _lib

NAMES = ("pt_debug_point_cache_counts", "pt_debug_point_cache_read", "pt_debug_point_cache_write",
         "pt_debug_point_cache_mode", "pt_debug_point_cache_word", "pt_debug_point_cache_key_words",
         "pt_debug_point_cache_key_diff", "pt_debug_point_cache_key_mode")
LOOKUP, PENDING, MARK, RESOLVE = 0, 1, 2, 3
OFF, RESET, USE = 0, 1, 2


@pytest.fixture(scope="module")
def gl():
    from ptsvgf import gl

    return gl


# ------------------------------------------------------------ the word ---
def _words():
    """Every word the cache can hold: any set of known lights, any occluded subset of it, any pending light or none."""
    for known in range(16):
        for occ in range(16):
            if occ & ~known:
                continue
            for pend in range(5):  # 0: none, else light pend - 1
                yield known | (occ << 4) | (pend << 8), known, occ, pend - 1


def test_lookup_reports_only_known_lights(gl):
    n = 0
    for w, known, occ, _ in _words():
        for li in range(4):
            want = -1 if not (known >> li) & 1 else (occ >> li) & 1
            assert gl.point_cache_word(LOOKUP, w, li) == want, (hex(w), li)
        n += 1
    assert n == 81 * 5
    # an occluded bit without its known bit is not a verdict
    for li in range(4):
        assert gl.point_cache_word(LOOKUP, 1 << (4 + li), li) == -1


def test_mark_pending_touches_only_the_pending_field(gl):
    for w, known, occ, _ in _words():
        assert gl.point_cache_word(PENDING, w) == (w >> 8) - 1
        for li in range(4):
            m = gl.point_cache_word(MARK, w, li)
            assert m & 0xFF == w & 0xFF and m >> 8 == li + 1, (hex(w), li)
            assert gl.point_cache_word(PENDING, m) == li


def test_resolve_sets_exactly_the_pending_lights_bits(gl):
    for w, known, occ, pend in _words():
        for verdict in (0, 1):
            r = gl.point_cache_word(RESOLVE, w, verdict)
            assert r >> 8 == 0, hex(w)  # pending cleared
            assert gl.point_cache_word(PENDING, r) == -1
            if pend < 0:
                assert r == w & 0xFF
                continue
            kbit, obit = 1 << pend, 1 << (4 + pend)
            assert r & ~(kbit | obit) == w & 0xFF & ~(kbit | obit), (hex(w), verdict)  # every other light as it was
            assert r & kbit
            assert bool(r & obit) == bool(verdict)
            assert gl.point_cache_word(LOOKUP, r, pend) == verdict


def test_word_argument_checks():
    pt = _lib.pt()
    ARG = -6
    out = C.c_uint32()
    assert pt.pt_debug_point_cache_word(LOOKUP, 0, 0, None) == ARG
    assert pt.pt_debug_point_cache_word(4, 0, 0, C.byref(out)) == ARG
    for li in (-1, 4):
        assert pt.pt_debug_point_cache_word(LOOKUP, 0xFF, li, C.byref(out)) == ARG
        assert pt.pt_debug_point_cache_word(MARK, 0, li, C.byref(out)) == ARG


# ------------------------------------------------------------- the key ---
def _key(gl, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(1, 2**63, gl.point_cache_key_words(), dtype=np.uint64)


def test_key_extends_the_primary_key(gl):
    """The primary key's words and eight more: the lights texture (handle, pointer, version), pointLightSize, the
    lights in the buffer, who decides the ray (point_bins and the bins), and the plane."""
    assert gl.point_cache_key_words() == gl.static_key_words(0) + 8


def test_mode_rule(gl):
    k = _key(gl)
    assert gl.point_cache_key_diff(k, k.copy()) == -1
    assert gl.point_cache_key_mode(k, True, k.copy(), True, True) == USE
    assert gl.point_cache_key_mode(k, False, k, True, True) == RESET  # the plane is stale
    assert gl.point_cache_key_mode(k, True, k, False, True) == OFF    # the draw runs the primary stage
    assert gl.point_cache_key_mode(k, False, k, False, True) == OFF
    for valid in (False, True):
        for reused in (False, True):
            assert gl.point_cache_key_mode(k, valid, k, reused, False) == OFF  # bypassed


def test_every_field_enters_the_compare(gl):
    """Each word flipped alone (lowest bit, highest bit, zero): the keys differ there and the draw resets the plane."""
    k = _key(gl)
    for i in range(len(k)):
        for flip in (k[i] ^ np.uint64(1), k[i] ^ np.uint64(1 << 63), np.uint64(0)):
            q = k.copy()
            q[i] = flip
            assert gl.point_cache_key_diff(k, q) == i, i
            assert gl.point_cache_key_diff(q, k) == i, i
            assert gl.point_cache_key_mode(k, True, q, True, True) == RESET, i


def test_key_argument_checks(gl):
    pt = _lib.pt()
    ARG, HANDLE = -6, -1
    u64p = C.POINTER(C.c_uint64)
    k = _key(gl)
    n = len(k)
    p = k.ctypes.data_as(u64p)
    f = C.c_int(7)
    assert pt.pt_debug_point_cache_key_diff(p, p, n, C.byref(f)) == 0 and f.value == -1
    assert pt.pt_debug_point_cache_key_diff(None, p, n, C.byref(f)) == ARG
    assert pt.pt_debug_point_cache_key_diff(p, p, n, None) == ARG
    assert pt.pt_debug_point_cache_key_diff(p, p, n - 1, C.byref(f)) == ARG
    assert pt.pt_debug_point_cache_key_mode(p, 1, p, n + 1, 1, 1, C.byref(f)) == ARG
    assert pt.pt_debug_point_cache_key_mode(p, 1, None, n, 1, 1, C.byref(f)) == ARG
    assert pt.pt_debug_point_cache_key_mode(p, 1, p, n, 1, 1, None) == ARG
    a, b = C.c_uint64(), C.c_uint64()
    assert pt.pt_debug_point_cache_counts(0xFFFFFFF0, C.byref(a), C.byref(b)) == HANDLE
    assert pt.pt_debug_point_cache_mode(0xFFFFFFF0, C.byref(f), C.byref(f)) == HANDLE


def test_header_declares_and_library_exports_the_entry_points():
    txt = open(os.path.join(_lib.INCLUDE_DIR, "ptsvgf_debug_static.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = C.CDLL(os.path.join(_lib.LIB_DIR, "libptsvgf.so"))
    pt_names, _ = _lib.exported_symbols()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert hasattr(lib, name), name
        assert name in pt_names

"""The host side of the bounce-0 shade's keep mode (DESIGN.md "Static view, part 4"; csrc/static_key.h through
include/ptsvgf_debug_firsthit.h): the first-hit key, the rule that decides a draw's mode, and the schedule it gives over
the colour slots of frames in flight. No device.

The attachments are modelled here as the library keeps them: a colour texture carries a background stamp (id, scope),
an emission or albedo texture a first-hit record; every draw makes all three fresh / empty before it stores
(att_plane), and a draw that is not bypassed leaves the ids of its own keys on them."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ptsvgf._lib import pt

U64 = C.c_uint64
OFF, FULL, KEEP = 0, 1, 2
(R_NONE, R_UNIFORM, R_ENV, R_STATS, R_SPP, R_BATCH, R_MEGAKERNEL, R_TILES, R_ROWS, R_DEEP, R_UNFOLDED, R_DEPTH0,
 R_ACCUMULATE, R_STAGE, R_COLOUR, R_EMISSION, R_ALBEDO) = range(17)
BYPASSES = (R_UNIFORM, R_ENV, R_STATS, R_SPP, R_BATCH, R_MEGAKERNEL, R_TILES, R_ROWS, R_DEEP, R_UNFOLDED, R_DEPTH0,
            R_ACCUMULATE)


def _words():
    return pt().pt_debug_firsthit_key_words()


def _key(seed=1):
    return (np.arange(_words(), dtype=np.uint64) * np.uint64(7919) + np.uint64(seed)).copy()


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(U64))


def _id(key):
    i = U64()
    assert pt().pt_debug_firsthit_key_id(_ptr(key), key.size, C.byref(i)) == 0
    return i.value


def _decide(bypass=0, reused=True, colour=(0, 0), emission=0, albedo=0, miss=0, first=0):
    m, r = C.c_int(-1), C.c_int(-1)
    assert pt().pt_debug_firsthit_decide(bypass, int(reused), colour[0], colour[1], emission, albedo, miss, first,
                                         C.byref(m), C.byref(r)) == 0
    return m.value, r.value


def test_key_word_count_and_arguments():
    n = _words()
    assert n > pt().pt_debug_static_key_words(0) + 2  # the primary content and what decode_hit reads beyond it
    a = _key()
    f = C.c_int()
    assert pt().pt_debug_firsthit_key_diff(_ptr(a), _ptr(a), n - 1, C.byref(f)) != 0
    assert pt().pt_debug_firsthit_key_diff(_ptr(a), _ptr(a), n, None) != 0
    assert pt().pt_debug_firsthit_key_id(_ptr(a), n + 1, C.byref(U64())) != 0
    assert pt().pt_debug_firsthit_decide(0, 1, 0, 0, 0, 0, 0, 0, None, None) != 0


def test_every_field_of_the_key_changed_in_turn_gives_no_keep():
    """A draw whose key differs in any one word from the key of the draw that wrote the planes gets another content id,
    so neither record equals it: full. The same key again: keep."""
    n = _words()
    base = _key()
    first = _id(base)
    miss = 1 << 50
    assert first != 0
    assert _decide(colour=(miss, 0), emission=first, albedo=first, miss=miss, first=first) == (KEEP, R_NONE)
    seen = {first}
    for w in range(n):
        k = base.copy()
        k[w] ^= np.uint64(1)
        f = C.c_int(-2)
        assert pt().pt_debug_firsthit_key_diff(_ptr(base), _ptr(k), n, C.byref(f)) == 0 and f.value == w
        other = _id(k)
        assert other not in seen and other != 0, w
        seen.add(other)
        mode, reason = _decide(colour=(miss, 0), emission=first, albedo=first, miss=miss, first=other)
        assert (mode, reason) == (FULL, R_EMISSION), w
    f = C.c_int(-2)
    assert pt().pt_debug_firsthit_key_diff(_ptr(base), _ptr(base.copy()), n, C.byref(f)) == 0 and f.value == -1


def test_equal_keys_one_id():
    a = _key(5)
    assert _id(a) == _id(a.copy())
    assert _id(a) != _id(_key(6))


def test_every_bypass_reports_its_reason():
    miss, first = 11, 12
    proven = dict(colour=(miss, 0), emission=first, albedo=first, miss=miss, first=first)
    assert _decide(**proven) == (KEEP, R_NONE)
    for r in BYPASSES:
        assert _decide(bypass=1 << r, **proven) == (OFF, r), r
    # several at once: the lowest is reported; a bypass wins over everything else
    for a, b in itertools.combinations(BYPASSES, 2):
        assert _decide(bypass=(1 << a) | (1 << b), **proven) == (OFF, min(a, b))
    assert _decide(bypass=1 << R_ROWS, reused=False) == (OFF, R_ROWS)


def test_what_is_not_proven_draws_in_full():
    miss, first = 21, 22
    ok = dict(colour=(miss, 0), emission=first, albedo=first, miss=miss, first=first)
    assert _decide(reused=False, **ok) == (FULL, R_STAGE)
    assert _decide(**{**ok, "colour": (miss + 1, 0)}) == (FULL, R_COLOUR)
    assert _decide(**{**ok, "colour": (0, 0), "miss": 0}) == (FULL, R_COLOUR)       # nothing known is no proof
    assert _decide(**{**ok, "colour": (miss, 7)}) == (FULL, R_COLOUR)               # the stamp of an SVGF copy: a set only
    assert _decide(**{**ok, "colour": (miss | (1 << 63), 0)}) == (FULL, R_COLOUR)   # the modulate's form of the content
    assert _decide(**{**ok, "emission": 0}) == (FULL, R_EMISSION)
    assert _decide(**{**ok, "emission": first + 1}) == (FULL, R_EMISSION)
    assert _decide(**{**ok, "albedo": 0}) == (FULL, R_ALBEDO)
    assert _decide(**{**ok, "emission": 0, "albedo": 0, "first": 0}) == (FULL, R_EMISSION)


class Slot:
    """One path-tracing pass with its three attachments, as capi_draw_pt.hip's draw_pathtrace treats them."""

    def __init__(self):
        self.colour, self.emission, self.albedo = (0, 0), 0, 0
        self.stage_key = None  # the primary key of the stage that ran last
        self.fresh = itertools.count(1 << 40)

    def written(self, name):  # tex_written: an upload, a clear, a blit, any draw into it
        if name == "colour":
            self.colour = (next(self.fresh), 0)
        else:
            setattr(self, name, 0)

    def draw(self, view, miss, first, bypass=0, ok=True):
        before = (self.colour, self.emission, self.albedo)
        for name in ("colour", "emission", "albedo"):
            self.written(name)  # pt_params' att_plane
        reused = self.stage_key == view
        mode, reason = _decide(bypass, reused, before[0], before[1], before[2], miss, first)
        if ok:
            self.stage_key = view
            if not bypass:  # bg_note_colour's conditions are among the bypasses
                self.colour = (miss, 0)
            if mode != OFF:
                self.emission = self.albedo = first
        else:
            self.stage_key = None if not reused else self.stage_key
        return mode, reason


def test_schedule_over_four_slots():
    """K = 4 colour slots take the frames in turn. Each slot's first draw of a view runs the stage: full. Its second and
    later draws find the stamp and both records of its own first draw: keep. A new view: one full draw per slot."""
    slots = [Slot() for _ in range(4)]
    miss, first = 101, 102
    modes = [slots[f % 4].draw("view A", miss, first) for f in range(16)]
    assert modes[:4] == [(FULL, R_STAGE)] * 4
    assert modes[4:] == [(KEEP, R_NONE)] * 12
    modes = [slots[f % 4].draw("view B", miss + 2, first + 2) for f in range(8)]
    assert modes == [(FULL, R_STAGE)] * 4 + [(KEEP, R_NONE)] * 4
    # the same view with another environment: the stage is reused, the colour is not this draw's content
    modes = [slots[f % 4].draw("view B", miss + 4, first + 2) for f in range(8)]
    assert modes == [(FULL, R_COLOUR)] * 4 + [(KEEP, R_NONE)] * 4


@pytest.mark.parametrize("name,reason", [("colour", R_COLOUR), ("emission", R_EMISSION), ("albedo", R_ALBEDO)])
def test_a_write_to_an_attachment_costs_one_full_draw(name, reason):
    s = Slot()
    miss, first = 201, 202
    assert [s.draw("v", miss, first)[0] for _ in range(3)] == [FULL, KEEP, KEEP]
    s.written(name)
    assert s.draw("v", miss, first) == (FULL, reason)
    assert s.draw("v", miss, first) == (KEEP, R_NONE)


def test_bypassed_and_failed_draws_leave_nothing_trusted():
    s = Slot()
    miss, first = 301, 302
    assert [s.draw("v", miss, first)[0] for _ in range(2)] == [FULL, KEEP]
    assert s.draw("v", miss, first, bypass=1 << R_STATS) == (OFF, R_STATS)
    assert s.draw("v", miss, first)[0] == FULL  # the bypassed draw recorded nothing
    assert s.draw("v", miss, first)[0] == KEEP
    assert s.draw("v", miss, first, ok=False)[0] == KEEP  # it was proven, and failed
    assert s.draw("v", miss, first)[0] == FULL

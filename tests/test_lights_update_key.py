"""The staleness rules of moving point lights (csrc/lights_key.h, csrc/point_cache.h pc_forget) on the host, through
include/ptsvgf_debug_lights.h and pt_debug_point_cache_word: which lights moved between two versions, when a moved
light counts as settled, what the verdict word forgets, and when a draw forgets instead of resetting."""
import numpy as np
import pytest

from ptsvgf import gl

KEEP, MARK, WALK, REBUILD = 0, 1, 2, 3
LOOKUP, PENDING, MARK_PENDING, RESOLVE, FORGET = 0, 1, 2, 3, 5


# ------------------------------------------------------------------ moved mask ---
def test_moved_mask_between_versions():
    stamps = [0, 5, 3, 7]  # light 0 never moved; 1 at version 5, 2 at 3, 3 at 7
    assert gl.lights_moved_mask(stamps, 0) == 0b1110
    assert gl.lights_moved_mask(stamps, 2) == 0b1110
    assert gl.lights_moved_mask(stamps, 3) == 0b1010  # a stamp equal to `since` is not newer
    assert gl.lights_moved_mask(stamps, 5) == 0b1000
    assert gl.lights_moved_mask(stamps, 7) == 0
    assert gl.lights_moved_mask(stamps[:2], 0) == 0b10  # only the lights asked about
    assert gl.lights_moved_mask([9] * 40, 1) == 0xFFFFFFFF  # the first 32


# ---------------------------------------------------------------------- settle ---
def test_standing_light_keeps_its_bins():
    assert gl.lights_settle([0, 0, 0], 2) == [KEEP, KEEP, KEEP]


def test_settle_zero_rebuilds_at_the_first_draw_after_the_move():
    assert gl.lights_settle([0, 4, 4, 4], 0) == [KEEP, REBUILD, KEEP, KEEP]
    assert gl.lights_settle([0, 4, 5, 5], 0) == [KEEP, REBUILD, REBUILD, KEEP]


def test_settle_counts_consecutive_standing_draws():
    # moved at version 4: marked at the first draw, rebuilt once 2 further draws found the same stamp
    assert gl.lights_settle([0, 4, 4, 4, 4], 2) == [KEEP, MARK, WALK, REBUILD, KEEP]
    assert gl.lights_settle([0, 4, 4, 4, 4], 1) == [KEEP, MARK, REBUILD, KEEP, KEEP]


def test_a_light_that_keeps_moving_is_marked_once_and_never_rebuilt():
    assert gl.lights_settle([3, 4, 5, 6, 7, 8], 2) == [MARK, WALK, WALK, WALK, WALK, WALK]


def test_a_move_restarts_the_count():
    # stands one draw, moves again, then stands two
    assert gl.lights_settle([4, 4, 6, 6, 6, 6], 2) == [MARK, WALK, WALK, WALK, REBUILD, KEEP]
    # after the rebuild a new move is marked afresh
    assert gl.lights_settle([4, 4, 4, 9, 9, 9], 2) == [MARK, WALK, REBUILD, MARK, WALK, REBUILD]


def test_negative_settle_counts_as_zero():
    assert gl.lights_settle([0, 4], -3) == [KEEP, REBUILD]


# ------------------------------------------------------------------- pc_forget ---
def _word(known=0, occluded=0, pending=-1):
    return known | (occluded << 4) | ((pending + 1) << 8)


def test_forget_clears_the_masked_lights_only():
    w = _word(known=0b1111, occluded=0b0110)
    got = gl.point_cache_word(FORGET, w, 0b0100)
    assert got == _word(known=0b1011, occluded=0b0010)
    assert gl.point_cache_word(LOOKUP, got, 2) == -1
    assert [gl.point_cache_word(LOOKUP, got, li) for li in (0, 1, 3)] == [0, 1, 0]


def test_forget_with_the_pending_light_inside_the_mask():
    w = _word(known=0b0011, occluded=0b0001, pending=2)
    got = gl.point_cache_word(FORGET, w, 0b0100)
    assert gl.point_cache_word(PENDING, got, 0) == -1
    assert got == _word(known=0b0011, occluded=0b0001)
    # a resolve that arrives afterwards finds nothing pending and sets no verdict
    assert gl.point_cache_word(RESOLVE, got, 1) == got


def test_forget_with_the_pending_light_outside_the_mask():
    w = _word(known=0b0110, occluded=0b0100, pending=0)
    got = gl.point_cache_word(FORGET, w, 0b0100)
    assert gl.point_cache_word(PENDING, got, 0) == 0
    assert got == _word(known=0b0010, occluded=0, pending=0)


def test_forget_all_four_lights():
    for pending in (-1, 0, 3):
        w = _word(known=0b1111, occluded=0b1010, pending=pending)
        assert gl.point_cache_word(FORGET, w, 0b1111) == 0
    # bits past the word's four lights name no light
    w = _word(known=0b1111, occluded=0b1010, pending=1)
    assert gl.point_cache_word(FORGET, w, 0xF0) == w


def test_forget_nothing():
    w = _word(known=0b1001, occluded=0b1000, pending=3)
    assert gl.point_cache_word(FORGET, w, 0) == w


# ------------------------------------------------------------------- mode rule ---
@pytest.fixture(scope="module")
def fields():
    names = ("handle", "dev", "ver", "bins", "bins_dev")
    return dict(zip(names, (gl.lights_key_field(i) for i in range(5))))


def _key(fields):
    k = np.arange(1, gl.point_cache_key_words() + 1, dtype=np.uint64) * np.uint64(1000)
    k[fields["handle"]] = 17
    k[fields["ver"]] = 5
    return k


def test_lights_version_only_difference_forgets_and_uses(fields):
    last = _key(fields)
    now = last.copy()
    now[fields["ver"]] = 6
    assert gl.lights_key_mode(last, True, now, True, True) == (2, True)
    now[fields["dev"]] += np.uint64(256)  # the update's new device version
    assert gl.lights_key_mode(last, True, now, True, True) == (2, True)
    # the bins may change with the lights: who decides the ray does not change the verdict
    now[fields["bins_dev"]] += np.uint64(4096)
    assert gl.lights_key_mode(last, True, now, True, True) == (2, True)
    now[fields["bins"]] = last[fields["bins"]] + np.uint64(1)
    assert gl.lights_key_mode(last, True, now, True, True) == (2, True)


def test_equal_keys_use_without_forgetting(fields):
    last = _key(fields)
    assert gl.lights_key_mode(last, True, last.copy(), True, True) == (2, False)


def test_any_other_word_resets(fields):
    last = _key(fields)
    free = set(fields.values())
    for i in range(last.size):
        if i in free:
            continue
        now = last.copy()
        now[fields["ver"]] = 6
        now[i] += np.uint64(1)
        assert gl.lights_key_mode(last, True, now, True, True) == (1, False), i
    # another handle, even with a newer version
    now = last.copy()
    now[fields["handle"]] = 18
    now[fields["ver"]] = 6
    assert gl.lights_key_mode(last, True, now, True, True) == (1, False)


def test_without_a_newer_version_the_bins_fields_reset_as_before(fields):
    last = _key(fields)
    for name in ("dev", "bins", "bins_dev"):
        now = last.copy()
        now[fields[name]] += np.uint64(1)
        assert gl.lights_key_mode(last, True, now, True, True) == (1, False), name
        assert gl.point_cache_key_mode(last, True, now, True, True) == 1
    older = last.copy()
    older[fields["ver"]] = 4
    assert gl.lights_key_mode(last, True, older, True, True) == (1, False)
    unbound = last.copy()  # no lights texture bound: handle 0
    unbound[fields["handle"]] = 0
    newer = unbound.copy()
    newer[fields["ver"]] = 6
    assert gl.lights_key_mode(unbound, True, newer, True, True) == (1, False)


def test_stale_plane_resets_and_bypass_is_off(fields):
    last = _key(fields)
    now = last.copy()
    now[fields["ver"]] = 6
    assert gl.lights_key_mode(last, False, now, True, True) == (1, False)   # nothing to forget from
    assert gl.lights_key_mode(last, True, now, False, True) == (0, False)   # the draw ran the primary stage
    assert gl.lights_key_mode(last, True, now, True, False) == (0, False)   # bypass
    assert gl.lights_key_mode(last, True, last.copy(), True, False) == (0, False)

"""The host side of the static background of the SVGF chain (DESIGN.md "Static view, part 3"; csrc/static_key.h through
include/ptsvgf_debug_background.h): the stamp's three rules, the reproject draw's choice of a quiet-tile set, the
miss-colour key and the content of the primary and G-buffer keys. No device.

The last test walks the fast driver's chain by hand over K = 4 colour slots, five G-buffer sets, both history parities,
and checks that a draw becomes skippable on exactly the frames the rules predict (worked out in its docstring, not
taken from the library) and never on the frame after a key field changes, for every field of the key in turn."""
import ctypes as C

import numpy as np
import pytest

from ptsvgf import gl
from ptsvgf._lib import pt

U64 = C.c_uint64
MOD = 1 << 63


class Rules:
    """The rules with a serial of its own (ids and set ids come from one counter, as in the library)."""

    def __init__(self):
        # (far above the ids the library's own counter hands out for miss keys below: in the library both kinds come
        # from one counter, so they cannot meet)
        self.serial = U64(1 << 40)

    def fresh(self):
        i, s = U64(), U64()
        assert pt().pt_debug_bg_fresh(C.byref(self.serial), C.byref(i), C.byref(s)) == 0
        return i.value, s.value

    def copy(self, src, qset, modulated=False):
        i, s = U64(), U64()
        assert pt().pt_debug_bg_copy(src[0], src[1], qset, int(modulated), C.byref(self.serial), C.byref(i),
                                     C.byref(s)) == 0
        return i.value, s.value

    @staticmethod
    def quiet(src, dst, qset, modulated=False):
        q = C.c_int()
        assert pt().pt_debug_bg_pair_quiet(src[0], src[1], dst[0], dst[1], qset, int(modulated), C.byref(q)) == 0
        return bool(q.value)

    def choose(self, state, prim, gbuf):
        s, b = U64(), C.c_int()
        assert pt().pt_debug_bg_quiet_set(state, prim, gbuf, C.byref(self.serial), C.byref(s), C.byref(b)) == 0
        return s.value, bool(b.value)


def test_fresh_ids_are_new_and_whole():
    r = Rules()
    a, b = r.fresh(), r.fresh()
    assert a[0] != b[0] and a[0] != 0 and b[0] != 0
    assert a[1] == 0 and b[1] == 0  # scope: the whole texture


def test_copy_propagates_the_inputs_content_on_the_set():
    r = Rules()
    src = r.fresh()
    out = r.copy(src, 7)
    assert out == (src[0], 7)
    # a copy of the copy on the same set keeps the content; on another set it is fresh (nothing known there)
    assert r.copy(out, 7) == (src[0], 7)
    other = r.copy(out, 8)
    assert other[0] not in (src[0], 0) and other[1] == 0
    # a draw without a set leaves a fresh content
    none = r.copy(src, 0)
    assert none[0] not in (src[0], other[0], 0) and none[1] == 0
    # an input of which nothing is known (id 0) propagates nothing
    assert r.copy((0, 0), 7)[0] not in (0, src[0])


def test_reset_by_any_other_writer():
    r = Rules()
    src = r.fresh()
    dst = r.copy(src, 7)
    assert r.quiet(src, dst, 7)
    dst = r.fresh()  # an upload, a clear, a blit, a path-tracing draw ...
    assert not r.quiet(src, dst, 7)
    src2 = r.fresh()  # ... or one into the source
    assert not r.quiet(src2, r.copy(src, 7), 7)


def test_scope_whole_against_scope_set():
    r = Rules()
    x = r.fresh()[0]
    assert r.quiet((x, 0), (x, 7), 7)      # whole covers every set
    assert r.quiet((x, 7), (x, 0), 7)
    assert r.quiet((x, 0), (x, 0), 7)
    assert r.quiet((x, 7), (x, 7), 7)
    assert not r.quiet((x, 7), (x, 8), 7)  # the output holds it on another set only
    assert not r.quiet((x, 8), (x, 7), 7)
    assert not r.quiet((x, 0), (x, 0), 0)  # no set, no skip
    assert not r.quiet((0, 0), (0, 0), 7)  # id 0 is no content


def test_modulated_tag():
    r = Rules()
    src = r.fresh()
    mod = r.copy(src, 7, modulated=True)
    assert mod == (src[0] | MOD, 7)
    assert r.quiet(src, mod, 7, modulated=True)
    assert not r.quiet(src, mod, 7)                       # (c.xyz, 1) is not c
    assert not r.quiet(src, r.copy(src, 7), 7, modulated=True)


def test_quiet_set_is_built_by_the_second_draw_of_a_pair():
    r = Rules()
    st = (U64 * 3)(0, 0, 0)
    assert r.choose(st, 5, 9) == (0, False)   # first sight of the pair: no set
    s, build = r.choose(st, 5, 9)
    assert s != 0 and build                    # second: built
    assert r.choose(st, 5, 9) == (s, False)    # then kept
    assert r.choose(st, 6, 9) == (0, False)    # another view
    assert r.choose(st, 5, 9) == (0, False)    # and back: a new first sight
    s2, build = r.choose(st, 5, 9)
    assert build and s2 not in (0, s)
    assert r.choose(st, 0, 9) == (0, False)    # a draw without a content forgets the pair
    assert r.choose(st, 5, 9) == (0, False)
    # a camera that moves every frame never builds
    for v in range(20, 30):
        assert r.choose(st, v, 9) == (0, False)


def _miss_key(seed=1):
    n = pt().pt_debug_bg_miss_key_words()
    return np.arange(seed, seed + n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)


def _p(a):
    return a.ctypes.data_as(C.POINTER(U64))


def test_miss_key_compare_covers_every_field():
    n = pt().pt_debug_bg_miss_key_words()
    assert n == gl.static_key_words(0) + 14  # the primary content and the fourteen inputs beyond it
    a = _miss_key()
    f = C.c_int()
    assert pt().pt_debug_bg_miss_key_diff(_p(a), _p(a.copy()), n, C.byref(f)) == 0 and f.value == -1
    ia = U64()
    assert pt().pt_debug_bg_miss_key_id(_p(a), n, C.byref(ia)) == 0 and ia.value != 0
    for i in range(n):
        b = a.copy()
        b[i] ^= np.uint64(1)
        assert pt().pt_debug_bg_miss_key_diff(_p(a), _p(b), n, C.byref(f)) == 0 and f.value == i
        ib, again = U64(), U64()
        assert pt().pt_debug_bg_miss_key_id(_p(b), n, C.byref(ib)) == 0
        assert ib.value not in (0, ia.value), i   # another content
        assert pt().pt_debug_bg_miss_key_id(_p(a), n, C.byref(again)) == 0
        assert again.value == ia.value            # equal keys, one id, whichever draw asks
    assert pt().pt_debug_bg_miss_key_diff(_p(a), _p(a), n - 1, C.byref(f)) != 0


@pytest.mark.parametrize("kind", [0, 1])
def test_key_content_clears_where_and_keeps_what(kind):
    n = gl.static_key_words(kind)
    a = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    ca = np.zeros(n, np.uint64)
    assert pt().pt_debug_bg_key_content(kind, _p(a), n, 77, _p(ca)) == 0
    where, what = [], []
    for i in range(n):
        b = a.copy()
        b[i] ^= np.uint64(2)
        cb = np.zeros(n, np.uint64)
        assert pt().pt_debug_bg_key_content(kind, _p(b), n, 77, _p(cb)) == 0
        (where if np.array_equal(ca, cb) else what).append(i)
    if kind == 0:
        # hit0 and its allocation's generation, the tile-cost and tile-order buffers; of the spill columns only whether
        # there are any: kPkPlane, kPkPlaneGen, kPkTileCost, kPkTilePerm are the key's last four words
        # (n - 6 is kPkSpill: another address of the columns is the same content, their absence is not)
        assert where == [n - 6, n - 4, n - 3, n - 2, n - 1]
        assert ca[n - 6] == 1
        b = a.copy()
        b[n - 6] = 0
        cb = np.zeros(n, np.uint64)
        assert pt().pt_debug_bg_key_content(kind, _p(b), n, 77, _p(cb)) == 0
        assert cb[n - 6] == 0 and not np.array_equal(ca, cb)
    else:
        # the four attachments' (handle, pointer, version, stamp), both compact planes' pointers and the bound
        # plane's validity and eye, the tile flags' allocation, and kGkSource, which the caller's identity replaces
        assert len(where) == 16 + 2 + 1 + 3 + 5 + 1
        assert ca[n - 2] == 77
        cb = np.zeros(n, np.uint64)
        assert pt().pt_debug_bg_key_content(kind, _p(a), n, 78, _p(cb)) == 0
        assert not np.array_equal(ca, cb)
    assert len(what) == n - len(where)


K, NG, FRAMES = 4, 5, 12
DRAWS = ("reproject", "variance", "atrous0", "atrous1", "atrous2", "atrous3", "atrous4")


def _walk(r, change_at=None, field=None, gbuf_change_at=None):
    """The fast driver's chain (ptsvgf/renderer.py _back_fast) on stamps alone. Per frame: which draws may skip.

    change_at: the frame from which word `field` of the miss key differs (a view, an environment, a uniform).
    gbuf_change_at: the frame from which the G-buffer key's content differs (the raster triangles) while the miss key
    stays. Frame f draws into colour slot f % K and G-buffer set f % NG; a set keeps the content id of the draw that
    wrote it last, as Texture::bg_gbuf does."""
    n, npk = pt().pt_debug_bg_miss_key_words(), gl.static_key_words(0)
    key = _miss_key(3)
    ids = {}

    def content(kind, words):  # equal keys, one id (the library's ContentIds, here for the two keys it is not asked for)
        return ids.setdefault((kind, tuple(int(w) for w in words)), r.fresh()[0])

    tex = {k: r.fresh() for k in ("illum", "var", "ping", "pong", "mod", "m0", "m1", "h0", "h1")}
    colour = [r.fresh() for _ in range(K)]
    colour_prim = [0] * K
    gset = [0] * NG
    geometry = 0
    set_gbuf = {}
    st = (U64 * 3)(0, 0, 0)
    out = []
    for f in range(FRAMES):
        if change_at is not None and f == change_at:
            key = key.copy()
            key[field] ^= np.uint64(4)
        if gbuf_change_at is not None and f == gbuf_change_at:
            geometry += 1
        cid = U64()
        assert pt().pt_debug_bg_miss_key_id(_p(key), n, C.byref(cid)) == 0
        # the G-buffer draw into set f % NG: its content is the view (the key's primary words) and the geometry
        g = f % NG
        gset[g] = content("gbuf", list(key[:npk]) + [geometry])
        # the path tracer's draw into slot f % K: the miss key's content, whole texture, and its primary content
        colour[f % K] = (cid.value, 0)
        colour_prim[f % K] = content("prim", key[:npk])
        b, pb = f & 1, 1 - (f & 1)
        qset, build = r.choose(st, colour_prim[f % K], gset[g])
        if build:
            set_gbuf[qset] = gset[g]
        skips = {}
        # reproject: colour -> illum, moments[pb] -> moments[b]; both pairs or none
        pairs = [(colour[f % K], "illum"), (tex[f"m{pb}"], f"m{b}")]
        skips["reproject"] = all(r.quiet(s, tex[d], qset) for s, d in pairs)
        for s, d in pairs:
            tex[d] = r.copy(s, qset)

        # variance and a-trous take the set their input's stamp holds for, if it was built for this set's content
        def draw(name, src, dst, mod=None):
            s = tex[src]
            q = s[1] if s[0] and set_gbuf.get(s[1]) == gset[g] else 0
            ok = r.quiet(s, tex[dst], q) and (mod is None or r.quiet(s, tex[mod], q, True))
            new = r.copy(s, q)
            new_mod = r.copy(s, q, True) if mod else None
            tex[dst] = new
            if mod:
                tex[mod] = new_mod
            skips[name] = ok

        draw("variance", "illum", "var")
        draw("atrous0", "var", "ping")
        draw("atrous1", "ping", f"h{b}")
        draw("atrous2", f"h{b}", "ping")
        draw("atrous3", "ping", "pong")
        draw("atrous4", "pong", "ping", mod="mod")
        out.append(skips)
    return out


def test_sequence_becomes_skippable_when_the_rules_say():
    """Frame 0 meets the view's pair for the first time: no set, every output fresh. Frame 1 builds the set Q and
    stamps every output of the chain with (content, Q), none of which was there before: nothing skips but iteration 2
    (history -> ping), whose output iteration 0 of the same frame has just stamped. Frame 2:
    the single planes (illum, variance, ping, pong, modulate) hold the miss colour on Q, and moments[0] still holds,
    whole, the content frame 0 left in it, which frame 1 copied into moments[1] on Q: reproject, variance and the
    a-trous iterations 0, 2, 3, 4 skip. Iteration 1 writes hist[0], last written at frame 0 without a set: it copies,
    once. From frame 3 on hist[1] (frame 1) and hist[0] (frame 2) both hold the colour on Q: every draw skips."""
    got = _walk(Rules())
    none = dict.fromkeys(DRAWS, False)
    assert got[0] == none and got[1] == {**none, "atrous2": True}
    assert got[2] == {**dict.fromkeys(DRAWS, True), "atrous1": False}
    for f in range(3, FRAMES):
        assert got[f] == dict.fromkeys(DRAWS, True), f


def test_no_skip_on_the_frames_after_a_key_field_changes():
    """Every field of the miss key in turn, from frame 6 on. A field of its primary part (the view, the scene, the
    rows) is another primary and G-buffer content: a new pair at frame 6, a new set at frame 7, and the schedule of
    a fresh start. A field beyond it (the environment, a miss-path uniform) leaves the pair and the set: the colour is
    another content, so at frame 6 its copies all run (iteration 2 alone stores into ping what iteration 0 has just
    put there), at frame 7 only the history plane frame 5 wrote still holds the old colour, from frame 8 on all skip."""
    none, every = dict.fromkeys(DRAWS, False), dict.fromkeys(DRAWS, True)
    npk = gl.static_key_words(0)
    for field in range(pt().pt_debug_bg_miss_key_words()):
        got = _walk(Rules(), change_at=6, field=field)
        assert got[5] == every, field
        if field < npk:
            assert got[6] == none and got[7] == {**none, "atrous2": True}, field
            assert got[8] == {**every, "atrous1": False}, field
        else:
            assert got[6] == {**none, "atrous2": True}, field
            assert got[7] == {**every, "atrous1": False}, field
            assert got[8] == every, field
        assert got[9] == every, field


def test_no_skip_after_the_gbuffer_content_alone_changes():
    """The raster triangles change at frame 6 and the miss key stays (geometry that moves where no primary ray
    goes): the colour keeps its content id, but the pair is new, the old set was built for another G-buffer content
    and no stamp covers the new one. Nothing skips at frame 6; frame 7 builds the set; then as from a fresh start.
    Each of the five sets is redrawn when its turn comes, so a frame never pairs a set of the old content."""
    none, every = dict.fromkeys(DRAWS, False), dict.fromkeys(DRAWS, True)
    got = _walk(Rules(), gbuf_change_at=6)
    assert got[5] == every
    assert got[6] == none and got[7] == {**none, "atrous2": True}
    assert got[8] == {**every, "atrous1": False}
    for f in range(9, FRAMES):
        assert got[f] == every, f

/* ptsvgf_debug_static.h — diagnostics of the static-view reuse (DESIGN.md "Static view"): the primary-hit cache of a
 * path-tracing pass (pass uniform primary_cache) and the G-buffer draw elision of a rasterize pass (pass uniform
 * reuse_static). Beside ptsvgf_debug.h and with its conventions: entry points tests and tools use to look inside the
 * library, no part of the drop-in boundary. */
#ifndef PTSVGF_DEBUG_STATIC_H
#define PTSVGF_DEBUG_STATIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* How many draws of `pass` did the work and how many reused an earlier draw's, since the pass was created.
 *   a path-tracing pass: *runs counts the draws that ran the primary stage (a pt_pass_draw_batch counts one for each of
 *     its passes), *reuses those that read the cached primary hit instead; megakernel draws (pt_kernel = 1) count in
 *     neither;
 *   a rasterize pass: *runs counts the G-buffer draws that launched, *reuses those that were elided.
 * PT_ERR_ARG for a pass of any other program. Either pointer may be NULL. */
int pt_debug_stage_counts(uint32_t pass, uint64_t* runs, uint64_t* reuses);

/* The keys behind both (csrc/static_key.h), for tests of the compare; needs no device. kind 0: the primary stage's
 * key, 1: the G-buffer draw's. A key is pt_debug_static_key_words(kind) 64-bit words, one per field. */
int pt_debug_static_key_words(int kind);
/* *field receives the index of the first word in which keys a and b differ, -1 when they are equal. */
int pt_debug_static_key_diff(int kind, const uint64_t* a, const uint64_t* b, int words, int* field);
/* The decision itself: *hit receives 1 when a draw with key `now` may reuse the work of the draw that left `last`
 * (last_valid: that key describes a completed draw). enabled: for kind 0, no trace statistics or row costs are bound
 * and primary_cache is not 0; for kind 1, reuse_static is on and no motion bound is bound. Kind 1 also needs the
 * compact planes the draw writes present and valid in `now`: the fwidth attachment's, and with bound_eye set the world
 * attachment's. */
int pt_debug_static_key_hit(int kind, const uint64_t* last, int last_valid, const uint64_t* now, int words, int enabled,
                            int* hit);

/* ---- The bounce-0 point-light verdict cache of a path-tracing pass (DESIGN.md "Static view, part 2"; pass uniform
 * point_cache, default 1; csrc/point_cache.h for the word's layout).
 *
 * Of the pass's last draw: the bounce-0 point-light verdicts served from the cache and those queued as rays. Device
 * counters; the call synchronises the device. PT_ERR_STATE before the pass's first wavefront draw. */
int pt_debug_point_cache_counts(uint32_t pass, uint64_t* served, uint64_t* queued);
/* The verdict plane itself, one 16-bit word per pixel of the rows the pass last drew (n: that pixel count, row-major
 * from the first row drawn). Both synchronise the device. */
int pt_debug_point_cache_read(uint32_t pass, uint16_t* words, size_t n);
int pt_debug_point_cache_write(uint32_t pass, const uint16_t* words, size_t n);
/* The mode of the pass's last draw (0 off, 1 reset, 2 use) and whether the plane holds verdicts now (1) or is stale. */
int pt_debug_point_cache_mode(uint32_t pass, int* mode, int* valid);
/* The lights (bit i: light i) the cache forgot at the top of the pass's last draw, because pt_lights_update had moved
 * them since the cache's key; 0 for a draw that forgot nothing. */
int pt_debug_point_cache_forgotten(uint32_t pass, uint32_t* mask);
/* The word's bit operations on the host, no device: op 0 look-up of light arg (*out: -1 as 0xFFFFFFFF not known, 0 lit,
 * 1 occluded), 1 the pending light (-1 none), 2 mark light arg pending, 3 resolve the pending light with verdict arg,
 * 5 forget the lights of the bit mask arg (moved lights, pt_lights_update). Op 4 is none and stays PT_ERR_ARG. */
int pt_debug_point_cache_word(int op, uint32_t word, int arg, uint32_t* out);
/* The cache's key (csrc/static_key.h LightsKey), as pt_debug_static_key_* for the other two: the word count, the first
 * differing word (-1: equal), and the mode a draw with key `now` gets after the draw that left `last` (last_valid: the
 * plane holds that draw's verdicts; stage_reused: this draw reads the cached primary hit; enabled: nothing bypasses). */
int pt_debug_point_cache_key_words(void);
int pt_debug_point_cache_key_diff(const uint64_t* a, const uint64_t* b, int words, int* field);
int pt_debug_point_cache_key_mode(const uint64_t* last, int last_valid, const uint64_t* now, int words, int stage_reused,
                                  int enabled, int* mode);

#ifdef __cplusplus
}
#endif
#endif

/* ptsvgf_debug_firsthit.h — diagnostics of the bounce-0 shade's keep mode (DESIGN.md "Static view, part 4"; int uniform
 * reuse_static on a path-tracing pass). Beside ptsvgf_debug_background.h and with its conventions: entry points tests
 * and tools use to look inside the library, no part of the drop-in boundary. */
#ifndef PTSVGF_DEBUG_FIRSTHIT_H
#define PTSVGF_DEBUG_FIRSTHIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The mode of a path-tracing pass's last draw. */
enum {
  PT_FH_OFF = 0,  /* bypassed: *reason says why; the draw records nothing on its attachments */
  PT_FH_FULL = 1, /* the draw qualifies and stored every texel: *reason names what was not proven */
  PT_FH_KEEP = 2  /* miss pixels untouched, no emission or albedo store, all-miss tiles not visited */
};
enum {
  PT_FH_R_NONE = 0,
  /* bypasses (mode off); bit (1 << reason) of pt_debug_firsthit_decide's `bypass` */
  PT_FH_R_UNIFORM = 1,    /* reuse_static is 0 (the default) */
  PT_FH_R_ENV = 2,        /* PTSVGF_STATIC_REUSE=0 in the environment */
  PT_FH_R_STATS = 3,      /* trace statistics or a row-cost buffer are bound */
  PT_FH_R_SPP = 4,        /* spp > 1 */
  PT_FH_R_BATCH = 5,      /* a draw of pt_pass_draw_batch */
  PT_FH_R_MEGAKERNEL = 6, /* pt_kernel = 1 */
  PT_FH_R_TILES = 7,      /* a tile subset (tile_stride > 1) */
  PT_FH_R_ROWS = 8,       /* a row subset, a band, or an attachment that does not store the whole frame */
  PT_FH_R_DEEP = 9,       /* a tree deeper than the LDS stack (spill columns) */
  PT_FH_R_UNFOLDED = 10,  /* shade_fold = 0 */
  PT_FH_R_DEPTH0 = 11,    /* max_tracing_depth = 0: no shade runs */
  PT_FH_R_ACCUMULATE = 12,/* accumulate != 0: a miss texel depends on the frame */
  /* full draws */
  PT_FH_R_STAGE = 13,     /* the primary stage ran (a new view, scene or plane; primary_cache = 0) */
  PT_FH_R_COLOUR = 14,    /* the colour attachment does not hold this draw's miss content on the whole frame */
  PT_FH_R_EMISSION = 15,  /* the emission attachment carries no first-hit record of this draw's content */
  PT_FH_R_ALBEDO = 16     /* nor does the albedo attachment */
};

/* Of `pass`'s last draw: mode and reason; *kept counts the pass's kept draws so far. Any pointer may be NULL. */
int pt_debug_firsthit_last(uint32_t pass, int* mode, int* reason, uint64_t* kept);

/* The pass's busy-tile list: *busy tiles hold a primary hit, of *tiles in the frame; *busy is -1 when no list stands
 * for the primary stage that ran last (no kept draw since). Reads a device word: the call synchronises the device. */
int pt_debug_firsthit_busy(uint32_t pass, int* busy, int* tiles);

/* A texture's first-hit record: the content id a qualifying draw left on its emission / albedo attachment, 0: none. */
int pt_debug_firsthit_record(uint32_t tex, uint64_t* id);

/* ---- The rule on the host (csrc/static_key.h), no device. */
/* The first-hit key (FirstHitKey): its word count, the first word in which a and b differ (-1: equal), and the content
 * id the library gives a key (equal keys: one id; the library's own table and counter, as pt_debug_bg_miss_key_id). */
int pt_debug_firsthit_key_words(void);
int pt_debug_firsthit_key_diff(const uint64_t* a, const uint64_t* b, int words, int* field);
int pt_debug_firsthit_key_id(const uint64_t* key, int words, uint64_t* id);
/* The mode of a draw. bypass: the bypass reasons that hold, one bit each; stage_reused: the draw reads the cached
 * primary hit; (colour_id, colour_scope): the colour attachment's background stamp and emission, albedo: the two
 * first-hit records, all as the draw finds them; miss, first: the content ids of the draw's two keys. */
int pt_debug_firsthit_decide(uint32_t bypass, int stage_reused, uint64_t colour_id, uint64_t colour_scope,
                             uint64_t emission, uint64_t albedo, uint64_t miss, uint64_t first, int* mode, int* reason);

#ifdef __cplusplus
}
#endif
#endif

/* ptsvgf_debug_background.h — diagnostics of the static background of the SVGF chain (DESIGN.md "Static view, part 3";
 * pass uniform static_background on the reproject, variance and a-trous passes). Beside ptsvgf_debug_static.h and with
 * its conventions: entry points tests and tools use to look inside the library, no part of the drop-in boundary. */
#ifndef PTSVGF_DEBUG_BACKGROUND_H
#define PTSVGF_DEBUG_BACKGROUND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The mode of an SVGF pass's last draw. */
enum {
  PT_BG_OFF = 0,   /* bypassed: *reason says why; the outputs' stamps are fresh */
  PT_BG_ARMED = 1, /* on, nothing skipped: no quiet-tile set yet, or a stamp does not agree (*reason) */
  PT_BG_SKIP = 2   /* the draw skipped its quiet tiles */
};
enum {
  PT_BG_R_NONE = 0,
  PT_BG_R_UNIFORM = 1,        /* static_background is 0 (the default) */
  PT_BG_R_ENV = 2,            /* PTSVGF_STATIC_BACKGROUND=0 in the environment */
  PT_BG_R_ROWS = 3,           /* a row subset, a band, or a texture that does not store the whole frame */
  PT_BG_R_SAMPLE_MOMENTS = 4, /* gSampleMoments is bound */
  PT_BG_R_NO_CONTENT = 5,     /* the colour plane or the G-buffer carries no content id: an spp or batched draw, a row
                                 subset, accumulation, the megakernel; a G-buffer no full-frame draw_raster wrote */
  PT_BG_R_KERNEL = 6,         /* the a-trous draw does not run the tiled kernel with tile flags */
  PT_BG_R_NO_PLANE = 7,       /* no compact depth-fwidth plane, no primary plane, or gNormalAndLinearZ and
                                 gNormalDepthFwidth are not one G-buffer draw's */
  PT_BG_R_NO_SET = 8,         /* armed: no quiet-tile set for this content yet (built by the second draw that meets it) */
  PT_BG_R_STAMPS = 9          /* armed: an output does not hold its input's content on the set */
};

/* A variance or a-trous draw whose input was written by a bypassed draw of the chain is bypassed with that draw's
 * reason (the reproject draw of an spp frame reports PT_BG_R_NO_CONTENT, and so do the six draws after it).
 *
 * Stream order: a quiet-tile set is built on the stream of the reproject draw that first needs it, and the library
 * orders nothing else. static_background therefore also states that the chain's draws are issued in stream order
 * after that reproject draw (one stream, or events), which the data dependency of the chain demands anyway.
 *
 * The reproject draws' choice of a set is one per process: the pair of the last reproject draw with the switch on.
 * Passes with the switch on that alternate between different views reset each other's pair, build no set and report
 * PT_BG_ARMED / PT_BG_R_NO_SET: safe, and nothing is gained. */

/* Of `pass`'s last draw: its mode and reason, and with PT_BG_SKIP the tiles it skipped out of those it has (16 x 16 blocks
 * for reproject and variance, the step's a-trous tiles otherwise); *skipped is 0 in the other modes, *total is 0 in
 * mode PT_BG_OFF. The skipped count is a device counter of the quiet-tile set: the call synchronises the device.
 * Any pointer may be NULL. */
int pt_debug_bg_counts(uint32_t pass, int* mode, int* reason, uint64_t* skipped, uint64_t* total);

/* A texture's background stamp: the content id (bit 63: the modulate's form of it) and the scope, 0 for the whole
 * texture or the id of the quiet-tile set the stamp holds for. */
int pt_debug_bg_stamp(uint32_t tex, uint64_t* id, uint64_t* scope);

/* Writes (tri, t) into the primary plane of path-tracing pass `pass` at pixel (x, y) of the rows it last drew, as
 * if the primary stage had hit triangle `tri` there at distance t (tri < 0: a miss). For tests of a G-buffer-background
 * pixel that is a primary hit. Synchronises the device. */
int pt_debug_bg_poke_hit0(uint32_t pass, int x, int y, int tri, float t);

/* ---- The rules on the host (csrc/static_key.h), no device. A stamp is (id, scope); *serial is the caller's counter of
 * ids (fresh ids and set ids are taken from it). */
/* rule 1, any other writer: a fresh id for the whole texture */
int pt_debug_bg_fresh(uint64_t* serial, uint64_t* id, uint64_t* scope);
/* rule 2, an SVGF draw's output after the draw: the input's content on the draw's set (modulated: under the modulate's
 * tag), or fresh when the input says nothing about `set` (set 0: the draw has none) */
int pt_debug_bg_copy(uint64_t in_id, uint64_t in_scope, uint64_t set, int modulated, uint64_t* serial, uint64_t* id,
                     uint64_t* scope);
/* rule 3: *quiet is 1 when a draw with quiet-tile set `set` would store on it what the output already holds */
int pt_debug_bg_pair_quiet(uint64_t in_id, uint64_t in_scope, uint64_t out_id, uint64_t out_scope, uint64_t set,
                           int modulated, int* quiet);
/* The reproject draw's choice of a set. state[3]: (primary content, G-buffer content, set) of the draw before, all 0
 * at first; updated. *set: the draw's set, 0 for none; *build: 1 when this draw builds it. */
int pt_debug_bg_quiet_set(uint64_t* state, uint64_t prim, uint64_t gbuf, uint64_t* serial, uint64_t* set, int* build);

/* The miss-colour key (csrc/static_key.h MissKey): its word count; the first word in which a and b differ (-1: equal);
 * and the content id the library gives a key (equal keys: one id; the library's own table, so ids are comparable with
 * pt_debug_bg_stamp's). */
int pt_debug_bg_miss_key_words(void);
int pt_debug_bg_miss_key_diff(const uint64_t* a, const uint64_t* b, int words, int* field);
int pt_debug_bg_miss_key_id(const uint64_t* key, int words, uint64_t* id);
/* The content of a primary key (kind 0) or a G-buffer key (kind 1; source: the identity of the pass whose triangles the
 * draw reads), pt_debug_static_key_words(kind) words in and out: the fields that name planes and scratch cleared. */
int pt_debug_bg_key_content(int kind, const uint64_t* key, int words, uint64_t source, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif

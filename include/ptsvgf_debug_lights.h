/* ptsvgf_debug_lights.h — diagnostics of moving point lights (pt_lights_update, ptsvgf.h; DESIGN.md "Moving point
 * lights"), beside ptsvgf_debug_static.h and with its conventions: entry points tests and tools use to look inside the
 * library, no part of the drop-in boundary. The staleness rules (csrc/lights_key.h) are plain host logic: the first
 * four calls need no device. */
#ifndef PTSVGF_DEBUG_LIGHTS_H
#define PTSVGF_DEBUG_LIGHTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Which lights moved between two versions: pos_stamps[l] is the version of the lights texture at which light l's
 * position last changed bitwise (0: never); *mask receives bit l for every l < nl (the first 32) whose stamp is newer
 * than `since`. */
int pt_debug_lights_moved_mask(const uint64_t* pos_stamps, int nl, uint64_t since, uint32_t* mask);
/* When a light counts as settled: one light's bins, built at stamp 0, meet the stamps[0 .. ndraws) in ndraws
 * consecutive path-tracing draws with point_bins_settle = settle. actions[i] receives what draw i does: 0 the lists
 * are this position's, 1 the light is marked "moved, bins pending" (its rays walk), 2 it is still marked, 3 its lists
 * are rebuilt (it has stood for `settle` draws after the one that first found its stamp). */
int pt_debug_lights_settle(const uint64_t* stamps, int ndraws, int settle, int* actions);
/* The verdict cache's mode rule with moved lights, as pt_debug_point_cache_key_mode: *mode 0 off, 1 reset, 2 use;
 * *forget 1 when the draw first forgets the moved lights' bits: it reuses the primary stage, the cache is valid, and
 * the keys differ only in the lights' version (newer) or device pointer and in the bins fields, under one non-zero
 * lights handle. */
int pt_debug_lights_key_mode(const uint64_t* last, int last_valid, const uint64_t* now, int words, int stage_reused,
                             int enabled, int* mode, int* forget);
/* The index of a word of that key: which 0 the lights handle, 1 their device pointer, 2 their version, 3 whether the
 * bins decide the rays, 4 the bins' device pointer. */
int pt_debug_lights_key_field(int which);
/* A lights texture buffer's state: its version, the position stamps of its first `cap` lights (0 past its lights),
 * and the device buffers it owns (1 until the first update; an update that finds an idle one allocates none). Any
 * output may be NULL. */
int pt_debug_lights_state(uint32_t lights_tex, uint64_t* version, uint64_t* pos_stamps, int cap, int* device_versions);

#ifdef __cplusplus
}
#endif
#endif

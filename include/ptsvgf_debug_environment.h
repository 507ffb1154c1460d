/* ptsvgf_debug_environment.h — diagnostics of pt_environment_update (ptsvgf.h; DESIGN.md "Environment edits"), beside
 * ptsvgf_debug_lights.h and with its conventions: for tests and tools, no part of the drop-in boundary. */
#ifndef PTSVGF_DEBUG_ENVIRONMENT_H
#define PTSVGF_DEBUG_ENVIRONMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* An hdrMap texture's state: its version; the device buffers the pair's texels hold (1 until the first update: the
 * texture's own; afterwards that one set aside, the current version and the retired ones; an update that finds an idle
 * one allocates none); the pinned host slots host sources were copied through (at most one per version). Either
 * texture of an updated pair may be named. Any output may be NULL. */
int pt_debug_environment_state(uint32_t hdr_tex, uint64_t* version, int* device_versions, int* staging_slots);

#ifdef __cplusplus
}
#endif
#endif

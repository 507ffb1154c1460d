/* ptsvgf_debug_rays.h — diagnostics of the ray queries (DESIGN.md "Ray queries"), for tests and tools/ray_query_prof.py. */
#ifndef PTSVGF_DEBUG_RAYS_H
#define PTSVGF_DEBUG_RAYS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The kernels pt_rays_closest and pt_rays_occluded launch from now on: 0 one ray per lane, 1 waves that refill their
 * idle lanes, -1 the library's default. Same bits either way. Needs no device. PT_ERR_ARG for another value. */
int pt_debug_rays_variant(int variant);
/* Of the last query that launched: its traversal stack (0 small, 1 full, 2 deep: entries past the LDS stack spill to
 * scratch) and its variant (-1 each before any); the allocations of the spill scratch so far and its size now. Any
 * pointer may be null. */
int pt_debug_rays_state(int* stack_kind, int* variant, uint64_t* scratch_allocs, size_t* scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif

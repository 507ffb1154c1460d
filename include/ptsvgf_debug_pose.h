/* ptsvgf_debug_pose.h — diagnostics of pt_pose_apply (ptsvgf.h), beside ptsvgf_debug_refit.h and with its
 * conventions: an entry point tests and tools use to look inside the library, no part of the drop-in boundary. */
#ifndef PTSVGF_DEBUG_POSE_H
#define PTSVGF_DEBUG_POSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* A posed raster vertex list of `pose`: which = 0 the current list (what the last pt_pose_apply wrote, the rest list
 * before the first), 1 the previous one (what the call before wrote; unspecified before the first pt_pose_apply).
 * *n receives the list's size in floats (0 for a pose without a raster list); the floats are copied to host_out
 * when host_out is not NULL (cap: its room in floats). Synchronises the device. */
int pt_debug_pose_raster(uint32_t pose, int which, float* host_out, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif

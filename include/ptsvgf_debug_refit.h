/* ptsvgf_debug_refit.h — diagnostics of pt_bvh_refit (ptsvgf.h), beside ptsvgf_debug.h and with its conventions:
 * entry points tests and tools use to look inside the library, no part of the drop-in boundary. (A header of its
 * own: tests/test_lbvh_trees_ref.py pins the declarations of ptsvgf_debug.h to the one it was written for.) */
#ifndef PTSVGF_DEBUG_REFIT_H
#define PTSVGF_DEBUG_REFIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The leaf order of the pt_bvh_build that wrote node_tex (PT_ERR_STATE for any other buffer): order[p] = the index
 * in that build's tri_in of the triangle at position p of its tri_out; pt_bvh_refit permutes by it. *n receives the
 * triangle count; the ints are copied to host_out when host_out is not NULL (cap: its room in ints). */
int pt_debug_lbvh_order(uint32_t node_tex, int* host_out, size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif
#endif

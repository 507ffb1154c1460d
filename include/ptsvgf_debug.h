/* ptsvgf_debug.h — diagnostics of libptsvgf.so that are no part of the drop-in boundary (ptsvgf.h): entry points
 * tests and tools use to look inside the library. Same conventions as ptsvgf.h (int status, pt_last_error()). */
#ifndef PTSVGF_DEBUG_H
#define PTSVGF_DEBUG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The walk trees of a node buffer pt_bvh_build wrote (PT_ERR_STATE for any other buffer).
 *   source 0: the buffers the device stage derived during pt_bvh_build (what draws read);
 *   source 1: the host functions that define them, run now on the host mirror of the node texels.
 *   which  0: packed binary tree, 4 float4 per interior node in depth-first preorder (left first):
 *             (L.AA.xyz, L.BB.x) (L.BB.yz, R.AA.xy) (R.AA.z, R.BB.xyz) (bits rl, bits rr, 0, 0); rl / rr is a child's
 *             packed index, or -(first * 16 + n) - 1 for a leaf;
 *          1: leaf list, 2 float4 per leaf in node order: (AA.xyz, bits ref) (BB.xyz, 0);
 *          2: 4-wide tree, 7 float4 per node (PT_WIDE_STRIDE): lo.x[4] hi.x[4] lo.y[4] hi.y[4] lo.z[4] hi.z[4] refs[4];
 *             refs >= 0 a 4-wide node, < 0 a leaf ref, 0x80000000 an empty slot (lo = +inf, hi = -inf).
 * *bytes receives the size of that buffer; it is copied to host_out when host_out is not NULL (cap: its room).
 * info8: root_ref, need (deepest interior level, root = 1), leaves, root4, need4 (most stack entries a 4-wide walk
 * holds), 4-wide nodes, NaN flag (a child box of the 4-wide tree has a NaN coordinate), device time of the stage in
 * microseconds (source 0; 0 for source 1). */
int pt_debug_lbvh_trees(uint32_t node_tex, int source, int which, void* host_out, size_t cap, size_t* bytes,
                        int* info8);

#ifdef __cplusplus
}
#endif
#endif

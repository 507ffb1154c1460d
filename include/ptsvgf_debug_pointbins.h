/* ptsvgf_debug_pointbins.h — diagnostics of the point-light triangle bins (pass uniform point_bins, ptsvgf.h), beside
 * ptsvgf_debug_refit.h and with its conventions: an entry point tests and tools use to look inside the library, no
 * part of the drop-in boundary. */
#ifndef PTSVGF_DEBUG_POINTBINS_H
#define PTSVGF_DEBUG_POINTBINS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The bins' build decides with this predicate (run here on the host, the same code) in which cells of one cube-map
 * face a triangle is listed (point_bins_tight = 1): (px, py)[0..n) is the face's clipped, projected polygon in cell
 * coordinates (n <= 8), fw the widening in cells, R the cells per face edge, [cx0, cx1] x [cy0, cy1] the cell box the
 * build found first (within [0, R - 1]). kept[(cy - cy0) * (cx1 - cx0 + 1) + (cx - cx0)] receives 1 for a cell that
 * lists the triangle, 0 for one dropped (cap: kept's room in bytes). A cell is dropped only if its square widened by
 * fw lies wholly beyond one edge line of the polygon; every cell is kept when the box has at most two cells or the
 * polygon is degenerate (*degenerate then receives 1; may be NULL). Needs no device. */
int pt_debug_point_bins_overlap(const float* px, const float* py, int n, float fw, int R, int cx0, int cy0, int cx1,
                                int cy1, uint8_t* kept, size_t cap, int* degenerate);

/* The lists of one light of the scene's bins (pt_point_bins_info), as they lie on the device: hdr receives the
 * 6 R R + 1 cell headers (first entry, entries), two ints each (hdr_cap: ints of room), ent the light's used entries,
 * two 32-bit words each (ent_cap: words of room), *entries their count (-1: the light has no usable lists, and ent
 * is left alone). Synchronises the device. hdr, ent, entries may be NULL. */
int pt_debug_point_bins_read(uint32_t tri_tex, uint32_t node_tex, int light, int32_t* hdr, size_t hdr_cap,
                             uint32_t* ent, size_t ent_cap, int* entries);

#ifdef __cplusplus
}
#endif
#endif

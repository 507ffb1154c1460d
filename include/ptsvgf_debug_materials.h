/* ptsvgf_debug_materials.h — diagnostics of pt_materials_update (DESIGN.md "Material edits"), for tests. */
#ifndef PTSVGF_DEBUG_MATERIALS_H
#define PTSVGF_DEBUG_MATERIALS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The scene decoded from (tri_tex, node_tex); PT_ERR_STATE when no draw has decoded one. shade_version: the
 * pt_materials_update calls that wrote its shading records; device_versions: the device buffers those records hold
 * (1 before the first update; then the current one, the retired ones and the decode's, set aside); staging_slots:
 * the material tables the library holds in all. Any pointer may be null. */
int pt_debug_materials_state(uint32_t tri_tex, uint32_t node_tex, uint64_t* shade_version, int* device_versions,
                             int* staging_slots);

#ifdef __cplusplus
}
#endif
#endif

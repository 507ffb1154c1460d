// materials_host.h — the host side of a material edit (DESIGN.md "Material edits", tests/materials_ref.py): the
// records of a texture buffer's host mirror patched by the rule of kernels_materials.hip. Plain C++, no HIP header:
// tools/materials_host_check.cpp builds it alone, with the sanitizers if wanted.
#pragma once
#include <cstddef>
#include <cstring>

namespace ptapi {

constexpr int kTriRecordFloats = 45, kTriMaterial0 = 18, kTriMaterialFloats = 18, kTriObjIndex = 42;

// n Triangle_encoded records: floats 18 .. 35 of the records of object first + k (objIndex == (float)(first + k),
// k < count, first + count <= 2^24) become table[18 k ..]; every other bit stays
inline void patch_records_host(float* rec, size_t n, const float* table, int first, int count) {
  for (size_t i = 0; i < n; ++i) {
    float* f = rec + i * kTriRecordFloats;
    const float o = f[kTriObjIndex];
    if (!(o >= (float)first && o < (float)(first + count))) continue;  // false for a NaN
    const int k = (int)o;
    if ((float)k != o) continue;
    memcpy(f + kTriMaterial0, table + (size_t)(k - first) * kTriMaterialFloats, kTriMaterialFloats * sizeof(float));
  }
}

}  // namespace ptapi

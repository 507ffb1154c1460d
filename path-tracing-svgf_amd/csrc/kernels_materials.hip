// kernels_materials.hip — material edits in place (DESIGN.md "Material edits", tests/materials_ref.py): the records of
// the objects first .. first + count - 1 take the 18 material floats of a small device table, every other bit is kept.
// A record belongs to object o when its objIndex compares == (float)o (pose_tris's rule: a fraction, a negative
// value or a NaN names no object). The only index read from memory is that objIndex, checked before it is used.
#include <hip/hip_runtime.h>

#include "pt_device.h"

namespace ptk {

namespace {

// k with objIndex == (float)(first + k) and k < count, or -1. first + count <= 2^24 (the caller's check), so every
// object index is exact as a float and no two objects claim one record.
__device__ __forceinline__ int material_slot(float f, int first, int count) {
  if (!(f >= (float)first && f < (float)(first + count))) return -1;  // false for a NaN
  const int o = (int)f;
  return (float)o == f ? o - first : -1;
}

// One thread per triangle: the old version's tri_shade record with the material floats (record floats 9 .. 26:
// s[2].y .. s[6].z) of a named object replaced, into the new version. Copy and patch are one pass. out may be old
// (a retired version taken again at once): a thread writes only the record it read.
__global__ void __launch_bounds__(256) materials_shade_kernel(const float4* old, float4* out, int n,
                                                              const float* __restrict__ table, int first, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4* s = old + 9 * (size_t)i;
  // (named registers: the compiler placed an array of nine in LDS, 8 KiB per block)
  const float4 r0 = s[0], r1 = s[1], r7 = s[7], r8 = s[8];
  float4 r2 = s[2], r3 = s[3], r4 = s[4], r5 = s[5], r6 = s[6];
  const int k = material_slot(r6.w, first, count);
  if (k >= 0) {
    const float* m = table + (size_t)k * kMaterialFloats;
    r2 = float4{r2.x, m[0], m[1], m[2]};
    r3 = float4{m[3], m[4], m[5], m[6]};
    r4 = float4{m[7], m[8], m[9], m[10]};
    r5 = float4{m[11], m[12], m[13], m[14]};
    r6 = float4{m[15], m[16], m[17], r6.w};
  }
  float4* d = out + 9 * (size_t)i;
  d[0] = r0;
  d[1] = r1;
  d[2] = r2;
  d[3] = r3;
  d[4] = r4;
  d[5] = r5;
  d[6] = r6;
  d[7] = r7;
  d[8] = r8;
}

// One thread per Triangle_encoded record, patched where it lies: floats 18 .. 35 of a named object's record.
__global__ void __launch_bounds__(256) materials_records_kernel(float* rec, int n, const float* __restrict__ table,
                                                                int first, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float* f = rec + (size_t)i * 45;
  const int k = material_slot(f[42], first, count);
  if (k < 0) return;
  const float* m = table + (size_t)k * kMaterialFloats;
#pragma unroll
  for (int j = 0; j < kMaterialFloats; ++j) f[18 + j] = m[j];
}

}  // namespace

int materials_shade_launch(const float4* old_shade, float4* new_shade, int n, const float* table, int first, int count,
                           hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(materials_shade_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, old_shade, new_shade,
                     n, table, first, count);
  return (int)hipGetLastError();
}

int materials_records_launch(float* records, int n, const float* table, int first, int count, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(materials_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, records, n, table,
                     first, count);
  return (int)hipGetLastError();
}

}  // namespace ptk

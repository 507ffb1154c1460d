// kernels_lights.hip — moving point lights (DESIGN.md "Moving point lights"): the verdict cache forgets the lights
// that moved. One pass over a path-tracing pass's verdict plane (WFState::pcache, point_cache.h), 2 bytes read and
// written per pixel, on the draw's stream before its bounce-0 shade looks anything up.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "point_cache.h"
#include "pt_device.h"

namespace ptk {

namespace {

// two words per thread: the plane is 256-byte aligned (wf_alloc), so a pair is one aligned 4-byte access; an odd
// count's last word is taken alone
__global__ void __launch_bounds__(256) pc_forget_kernel(uint16_t* plane, size_t n, uint32_t mask) {
  const size_t pairs = n >> 1;
  uint32_t* p2 = (uint32_t*)plane;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (size_t)gridDim.x * 256) {
    const uint32_t v = p2[i];
    const uint32_t r = pc_forget(v & 0xffffu, mask) | (pc_forget(v >> 16, mask) << 16);
    if (r != v) p2[i] = r;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) plane[n - 1] = (uint16_t)pc_forget(plane[n - 1], mask);
}

}  // namespace

int launch_point_cache_forget(uint16_t* plane, size_t n, uint32_t mask, hipStream_t s) {
  if (!plane || ((uintptr_t)plane & 3u)) return (int)hipErrorInvalidValue;
  if (n == 0 || !(mask & ((1u << kPcLights) - 1u))) return (int)hipSuccess;
  const size_t blocks = std::min<size_t>(((n >> 1) + 255) / 256 + 1, 4096);
  hipLaunchKernelGGL(pc_forget_kernel, dim3((unsigned)blocks), dim3(256), 0, s, plane, n, mask);
  return (int)hipGetLastError();
}

}  // namespace ptk

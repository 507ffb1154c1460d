// rays_device.h — what capi_rays.hip hands to the ray-query kernels (kernels_rays.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_device.h"

namespace ptk {

// The kernel variants of a query: one ray per lane, or waves that refill their idle lanes (same bits).
constexpr int kRaysLane = 0, kRaysRefill = 1;

struct RayQuery {
  SceneDev scene;       // tri_geom, tri_shade, bvh / root_ref (the reference tree); with sah: bvh_any / root_any; with
                        // wide: bvh4 / root4 / root4c
  const float4* rays;   // 2 per ray: (origin, -), (direction, tmax)
  long long n;
  int sah;              // rays from within fine_limit walk the SAH tree over the reference leaves (ties: the reference's)
  int wide;             // and, where the kernel has a 4-wide walk, its 4-wide form
  float fine_limit;     // SceneGPU::fine_eye_limit: the reach of those trees' fine boxes, per origin coordinate
  int stack_need;       // the most stack entries a binary walk of these trees holds
  int* spill;           // deep trees: entry kSpillKS + j of the lane in column c at spill[j * spill_stride + c]
  size_t spill_stride;  // columns: the grid's threads (ray_query_blocks(n) * 128)
};

int ray_query_blocks(long long n);
int launch_rays_closest(const RayQuery& q, void* hits, int variant, hipStream_t s);
int launch_rays_occluded(const RayQuery& q, void* verdicts, int variant, hipStream_t s);
// xy: n int32 pairs, or null for every pixel of p.W x p.H row-major (n = W * H). p: W, H, eye, camRot, aspect_corrected.
int launch_rays_primary(const PTParams& p, const void* xy, long long n, void* rays_out, hipStream_t s);

}  // namespace ptk

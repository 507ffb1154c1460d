// kernels_rays.hip — ray queries over a caller's ray list (include/ptsvgf.h "ray queries", DESIGN.md "Ray queries";
// capi_rays.hip has the entry points): the closest hit of every ray as hitBVH (path_tracing.frag:372-424) returns it,
// the occlusion verdict derived from it, and the path-tracing pass's primary rays written out as ray records. The
// walks are pt_shading.h's; tests/ray_query_ref.py is the definition.
//
// A ray is two float4 (origin, -) (direction, tmax); a hit two float4 (t, tri, obj, inside) (P, 0). One ray per lane
// in 128-thread blocks with a per-lane LDS stack column as in wf_trace_closest, a bounded grid striding over the list;
// or (the *_refill kernels) waves that hand the next rays of their chunk to lanes whose rays ended, as
// wf_trace_closest_refill does. Both give the same bits: per ray the candidate triangles and the tie rule are the same.
#include <hip/hip_runtime.h>

#include "glsl_builtins.h"
#include "pt_device.h"
#include "pt_shading.h"
#include "rays_device.h"
#include "wf_common.h"

using namespace glsl;

namespace ptk {

namespace {

// the SAH / 4-wide trees' fine boxes hold for origins within q.fine_limit per coordinate (host_trees.cpp
// refine_leaves); a ray from further out (or from a NaN) walks the reference tree
__device__ __forceinline__ bool origin_near(const RayQuery& q, v3 S) {
  return fabsf(S.x) <= q.fine_limit && fabsf(S.y) <= q.fine_limit && fabsf(S.z) <= q.fine_limit;
}

// this lane's stack: its LDS column and, DEEP, column `col` of the spill scratch
template <int KS, bool DEEP>
__device__ __forceinline__ auto query_stack(int* lds_column, const RayQuery& q, size_t col) {
  if constexpr (DEEP) return SpillStack<kTB, KS>{lds_column, q.spill + col, q.spill_stride};
  else return LdsStack<kTB>{lds_column};
}

__device__ __forceinline__ int obj_of(const SceneDev& sc, int tri) {
  const float f = sc.tri_shade[9 * tri + 6].w;  // objIndex (float 42 of the record)
  return (__builtin_isfinite(f) && fabsf(f) <= 16777216.0f) ? (int)f : -1;
}

__device__ __forceinline__ void store_hit(const RayQuery& q, float4* __restrict__ hits, long long i, int tri, float t,
                                          v3 S, v3 d) {
  float4 a, b;
  if (tri >= 0) {
    const bool inside = dot(xyz(q.scene.tri_geom[4 * tri + 3]), d) > 0.0f;  // hitTriangle's isInside (:230)
    const v3 P = add(S, muls(d, t));
    a = f4(t, __int_as_float(tri), __int_as_float(obj_of(q.scene, tri)), __int_as_float(inside ? 1 : 0));
    b = f4(P.x, P.y, P.z, 0.0f);
  } else {
    a = f4(PT_INF, __int_as_float(-1), __int_as_float(-1), __int_as_float(0));
    b = f4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  stnt(hits + 2 * i, a);
  stnt(hits + 2 * i + 1, b);
}

// Any triangle the reference's walk tests that hitTriangle accepts with t < PT_INF and t < tmax (the occlusion
// query's predicate: in units of t, the direction is not normalised). Binary walk, anyhit2's shape; boxes entered
// beyond tmax are pruned with the point-light walks' margin.
template <class Stk>
__device__ bool occluded2(const SceneDev& sc, Stk& stk, v3 S, v3 d, float tmax) {
  const v3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const float lim = tmax * 1.0002f + 2.0e-4f;
  int sp = 0;
  int node = sc.root_ref;
  int leaf = kNone;
  if (node < 0) { leaf = node; node = kNone; }
  while (node != kNone || leaf != kNone) {
    while (node >= 0) {
      const float4* nd = sc.bvh + 4 * node;
      const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
      float t0l, t0r;
      const float dl = slab(S, inv, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, &t0l);
      const float dr = slab(S, inv, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, &t0r);
      const bool hl = dl > 0.0f && !(t0l > lim), hr = dr > 0.0f && !(t0r > lim);
      const int cl = __float_as_int(q3.x), cr = __float_as_int(q3.y);
      if (hl && hr) {
        const bool lnear = dl < dr;
        stk.put(sp++, lnear ? cr : cl);
        node = lnear ? cl : cr;
      } else if (hl) {
        node = cl;
      } else if (hr) {
        node = cr;
      } else {
        node = sp > 0 ? stk.get(--sp) : kNone;
      }
      if (node < 0 && node != kNone && leaf == kNone) {
        leaf = node;
        node = sp > 0 ? stk.get(--sp) : kNone;
      }
      if (!__any(leaf == kNone)) break;
    }
    while (leaf != kNone) {
      if (leaf_scan(sc.tri_geom, ref_leaf_first(leaf), ref_leaf_count(leaf), S, d,
                    [&](int, float t) { return t < PT_INF && t < tmax; }))
        return true;
      leaf = kNone;
      if (node < 0 && node != kNone) {
        leaf = node;
        node = sp > 0 ? stk.get(--sp) : kNone;
      }
    }
  }
  return false;
}

// The same verdict on the 4-wide tree (anyhit4's shape): 1 occluded, 0 not, -1 when the KS-entry stack would
// overflow (the caller walks the binary tree then).
template <int KS>
__device__ int occluded4(const SceneDev& sc, int* __restrict__ stk, v3 S, v3 d, float tmax) {
  const v3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const float lim = tmax * 1.0002f + 2.0e-4f;
  int sp = 0;
  int node = sc.root4;
  int leaf = kNone;
  if (node < 0) { leaf = node; node = kNone; }
  while (node != kNone || leaf != kNone) {
    while (node >= 0) {
      const float4* q = sc.bvh4 + kWideStride * node;
      const float4 lx = q[0], hx = q[1], ly = q[2], hy = q[3], lz = q[4], hz = q[5], rf = q[6];
      const float alx[4] = {lx.x, lx.y, lx.z, lx.w}, ahx[4] = {hx.x, hx.y, hx.z, hx.w};
      const float aly[4] = {ly.x, ly.y, ly.z, ly.w}, ahy[4] = {hy.x, hy.y, hy.z, hy.w};
      const float alz[4] = {lz.x, lz.y, lz.z, lz.w}, ahz[4] = {hz.x, hz.y, hz.z, hz.w};
      const int ref[4] = {__float_as_int(rf.x), __float_as_int(rf.y), __float_as_int(rf.z), __float_as_int(rf.w)};
      int next = kNone;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float t0;
        const float dist = slab(S, inv, alx[c], aly[c], alz[c], ahx[c], ahy[c], ahz[c], &t0);
        if (ref[c] != kNone && dist > 0.0f && !(t0 > lim)) {
          if (next == kNone) {
            next = ref[c];
          } else {
            if (sp == KS) return -1;
            stk[sp++ * kTB] = ref[c];
          }
        }
      }
      node = next != kNone ? next : (sp > 0 ? stk[--sp * kTB] : kNone);
      if (node < 0 && node != kNone && leaf == kNone) {
        leaf = node;
        node = sp > 0 ? stk[--sp * kTB] : kNone;
      }
      if (!__any(leaf == kNone)) break;
    }
    while (leaf != kNone) {
      if (leaf_scan(sc.tri_geom, ref_leaf_first(leaf), ref_leaf_count(leaf), S, d,
                    [&](int, float t) { return t < PT_INF && t < tmax; }))
        return 1;
      leaf = kNone;
      if (node < 0 && node != kNone) {
        leaf = node;
        node = sp > 0 ? stk[--sp * kTB] : kNone;
      }
    }
  }
  return 0;
}

// ------------------------------------------------------------ one ray per lane ---
template <int KS, bool DEEP>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR rays_closest_lane(RayQuery q, float4* __restrict__ hits) {
  __shared__ int stk[KS * kTB];
  const size_t col = (size_t)blockIdx.x * kTB + threadIdx.x;
  for (long long i = (long long)col; i < q.n; i += (long long)gridDim.x * kTB) {
    const float4 o = ldnt(q.rays + 2 * i), dd = ldnt(q.rays + 2 * i + 1);
    const v3 S = xyz(o), d = xyz(dd);
    auto st = query_stack<KS, DEEP>(stk + threadIdx.x, q, col);
    float t;
    const int tri = closest_hit(q.scene, q.sah && origin_near(q, S), st, S, d, 1, &t, nullptr);
    store_hit(q, hits, i, tri, t, S, d);
  }
}

template <int KS, bool DEEP, bool WIDE>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR rays_occluded_lane(RayQuery q, uint8_t* __restrict__ out) {
  __shared__ int stk[KS * kTB];
  const size_t col = (size_t)blockIdx.x * kTB + threadIdx.x;
  for (long long i = (long long)col; i < q.n; i += (long long)gridDim.x * kTB) {
    const float4 o = ldnt(q.rays + 2 * i), dd = ldnt(q.rays + 2 * i + 1);
    const v3 S = xyz(o), d = xyz(dd);
    const bool near = q.sah && origin_near(q, S);
    int occ = (WIDE && near) ? occluded4<KS>(q.scene, stk + threadIdx.x, S, d, dd.w) : -1;
    if (occ < 0) {  // no 4-wide tree for this ray, or its stack overflowed: the binary walk
      auto st = query_stack<KS, DEEP>(stk + threadIdx.x, q, col);
      occ = occluded2(near ? anyhit_scene(q.scene) : q.scene, st, S, d, dd.w);
    }
    out[i] = (uint8_t)occ;
  }
}

// ------------------------------------------------------------------ lane refill ---
// A wave owns the chunks vw, vw + gw, .. of kRayChunk consecutive rays (vw: its index in the grid, gw: the grid's
// waves) and hands a chunk's next rays to its idle lanes in lane order, between two leaf phases of the while-while
// walk, once at least kRayRefillMin lanes idle (a refill stalls the wave for the new rays' loads).
constexpr int kRayChunk = 256;
constexpr int kRayRefillMin = 16;
struct RayChunks {
  long long n, next, end;
  long long vw, gw;
  __device__ __forceinline__ void chunk() {
    next = min(vw * kRayChunk, n);
    end = min(next + kRayChunk, n);
  }
  __device__ __forceinline__ bool grab() {
    vw += gw;
    chunk();
    return next < end;
  }
};
__device__ __forceinline__ RayChunks ray_chunks(long long n) {
  RayChunks c{n, 0, 0, (long long)blockIdx.x * (kTB / 64) + (threadIdx.x >> 6), (long long)gridDim.x * (kTB / 64)};
  c.chunk();
  return c;
}

// One step of a binary walk (traverse's descent): both child boxes tested, the nearer hit child entered, the other
// pushed. `lim`: boxes entered beyond it are pruned.
template <class Stk>
__device__ __forceinline__ void binary_step(const float4* __restrict__ tree, int& node, Stk& st, int& sp, v3 S, v3 inv,
                                            float lim) {
  const float4* nd = tree + 4 * node;
  const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
  float t0l, t0r;
  const float dl = slab(S, inv, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, &t0l);
  const float dr = slab(S, inv, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, &t0r);
  const bool hl = dl > 0.0f && !(t0l > lim), hr = dr > 0.0f && !(t0r > lim);
  const int cl = __float_as_int(q3.x), cr = __float_as_int(q3.y);
  if (hl && hr) {
    const bool lnear = dl < dr;
    st.put(sp++, lnear ? cr : cl);
    node = lnear ? cl : cr;
  } else if (hl) {
    node = cl;
  } else if (hr) {
    node = cr;
  } else {
    node = sp > 0 ? st.get(--sp) : kNone;
  }
}

// Closest hits with lane refill. Per ray closest_hit's walk: on the SAH tree over the reference leaves (WIDE: on its
// 4-wide form, the same candidate triangles), and for a ray whose best t a second triangle met exactly the walk again
// on the reference tree in the reference's order, by the same lane before it takes a new ray. A 4-wide walk whose
// pushes would overflow the stack, or whose ray is axis-parallel (wide_step's signed planes need finite inverses),
// restarts on the reference tree too, as does a ray from beyond the fine boxes' reach.
template <int KS, bool DEEP, bool WIDE>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR rays_closest_refill(RayQuery q, float4* __restrict__ hits) {
  __shared__ int stk[KS * kTB];
  const int lane = threadIdx.x & 63;
  RayChunks c = ray_chunks(q.n);
  if (c.next >= c.end) return;
  const unsigned long long below = (1ull << lane) - 1ull;
  auto st = query_stack<KS, DEEP>(stk + threadIdx.x, q, (size_t)blockIdx.x * kTB + threadIdx.x);
  bool have = false, ref = false, tied = false, ovf = false;  // ref: this lane walks the reference tree
  long long i = 0;
  int sp = 0, node = kNone, leaf = kNone, best = -1;
  v3 S = splat(0.0f), d = splat(0.0f), inv = splat(0.0f);
  float tbest = PT_INF;
  auto start = [&](bool on_ref) {
    ref = on_ref;
    node = on_ref ? q.scene.root_ref : (WIDE ? q.scene.root4c : q.scene.root_any);
    tbest = PT_INF;
    best = -1;
    tied = ovf = false;
    sp = 0;
    leaf = kNone;
    if (node < 0) { leaf = node; node = kNone; }
  };
  while (true) {
    const unsigned long long idle = __ballot(!have);
    if (__popcll(idle) >= (__ballot(have) ? kRayRefillMin : 1) && (c.next < c.end || c.grab())) {
      const long long k = c.next + __popcll(idle & below);
      if (!have && k < c.end) {
        i = k;
        const float4 o = ldnt(q.rays + 2 * i), dd = ldnt(q.rays + 2 * i + 1);
        S = xyz(o);
        d = xyz(dd);
        inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        start(!(q.sah && origin_near(q, S)) || (WIDE && PT_WIDE_SIGNED && !finite3(inv)));
        have = true;
      }
      c.next = min(c.next + (long long)__popcll(idle), c.end);
    }
    if (!__any(have)) break;
    while (node >= 0) {  // traverse<0>'s descent, pruned by the current best t
      const float lim = tbest * 1.0002f + 2.0e-4f;
      if (WIDE && !ref) {
        if (!wide_step<KS, true>(q.scene.bvh4, node, st, sp, S, inv, lim)) {
          ovf = true;
          node = leaf = kNone;
        }
      } else {
        binary_step(ref ? q.scene.bvh : q.scene.bvh_any, node, st, sp, S, inv, lim);
      }
      if (node < 0 && node != kNone && leaf == kNone) {
        leaf = node;
        node = sp > 0 ? st.get(--sp) : kNone;
      }
      if (!__any(leaf == kNone)) break;
    }
    while (leaf != kNone) {  // traverse<0>'s leaf phase: strict '<' keeps the first triangle at a given t
      leaf_scan(q.scene.tri_geom, ref_leaf_first(leaf), ref_leaf_count(leaf), S, d, [&](int j, float t) {
        if (t < tbest) {
          tbest = t;
          best = j;
          tied = false;
        } else if (t == tbest && best >= 0) {
          tied = true;
        }
        return false;
      });
      leaf = kNone;
      if (node < 0 && node != kNone) {
        leaf = node;
        node = sp > 0 ? st.get(--sp) : kNone;
      }
    }
    if (have && node == kNone && leaf == kNone) {  // this lane's walk is complete (or gave up: ovf)
      if (!ref && (tied || ovf)) {
        start(true);  // in the reference's order
      } else {
        store_hit(q, hits, i, best, tbest, S, d);
        have = false;
      }
    }
  }
}

// Occlusion verdicts with lane refill: occluded2's walk (WIDE: on the 4-wide tree, children in slot order; a walk
// whose stack would overflow, an axis-parallel ray and a ray from beyond the fine boxes' reach walk the reference tree).
template <int KS, bool DEEP, bool WIDE>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR rays_occluded_refill(RayQuery q, uint8_t* __restrict__ out) {
  __shared__ int stk[KS * kTB];
  const int lane = threadIdx.x & 63;
  RayChunks c = ray_chunks(q.n);
  if (c.next >= c.end) return;
  const unsigned long long below = (1ull << lane) - 1ull;
  auto st = query_stack<KS, DEEP>(stk + threadIdx.x, q, (size_t)blockIdx.x * kTB + threadIdx.x);
  bool have = false, ref = false, ovf = false;
  long long i = 0;
  int sp = 0, node = kNone, leaf = kNone;
  v3 S = splat(0.0f), d = splat(0.0f), inv = splat(0.0f);
  float tmax = 0.0f, lim = 0.0f;
  auto start = [&](bool on_ref) {
    ref = on_ref;
    node = on_ref ? q.scene.root_ref : (WIDE ? q.scene.root4 : q.scene.root_any);
    ovf = false;
    sp = 0;
    leaf = kNone;
    if (node < 0) { leaf = node; node = kNone; }
  };
  while (true) {
    const unsigned long long idle = __ballot(!have);
    if (__popcll(idle) >= (__ballot(have) ? kRayRefillMin : 1) && (c.next < c.end || c.grab())) {
      const long long k = c.next + __popcll(idle & below);
      if (!have && k < c.end) {
        i = k;
        const float4 o = ldnt(q.rays + 2 * i), dd = ldnt(q.rays + 2 * i + 1);
        S = xyz(o);
        d = xyz(dd);
        inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        tmax = dd.w;
        lim = tmax * 1.0002f + 2.0e-4f;
        start(!(q.sah && origin_near(q, S)) || (WIDE && PT_WIDE_SIGNED && !finite3(inv)));
        have = true;
      }
      c.next = min(c.next + (long long)__popcll(idle), c.end);
    }
    if (!__any(have)) break;
    while (node >= 0) {
      if (WIDE && !ref) {
        if (!wide_step<KS, false>(q.scene.bvh4, node, st, sp, S, inv, lim)) {
          ovf = true;
          node = leaf = kNone;
        }
      } else {
        binary_step(ref ? q.scene.bvh : q.scene.bvh_any, node, st, sp, S, inv, lim);
      }
      if (node < 0 && node != kNone && leaf == kNone) {
        leaf = node;
        node = sp > 0 ? st.get(--sp) : kNone;
      }
      if (!__any(leaf == kNone)) break;
    }
    bool hit = false;
    while (leaf != kNone) {
      if (leaf_scan(q.scene.tri_geom, ref_leaf_first(leaf), ref_leaf_count(leaf), S, d,
                    [&](int, float t) { return t < PT_INF && t < tmax; })) {
        hit = true;
        break;
      }
      leaf = kNone;
      if (node < 0 && node != kNone) {
        leaf = node;
        node = sp > 0 ? st.get(--sp) : kNone;
      }
    }
    if (have && (hit || (node == kNone && leaf == kNone))) {
      if (!hit && !ref && ovf) {
        start(true);
      } else {
        out[i] = hit ? 1 : 0;
        have = false;
        node = leaf = kNone;
      }
    }
  }
}

// ----------------------------------------------------------------- primary rays ---
// The ray records of pixels (x, y): the path-tracing pass's origin and primary_dir, tmax = +inf. A pixel outside the
// frame gets the direction 0, which misses everything (hitTriangle's parallel test rejects every triangle).
__global__ void __launch_bounds__(256) rays_primary_k(PTParams p, const int2* __restrict__ xy, long long n,
                                                      float4* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    int x, y;
    if (xy) {
      const int2 c = xy[i];
      x = c.x;
      y = c.y;
    } else {
      x = (int)(i % p.W);
      y = (int)(i / p.W);
    }
    const bool in = x >= 0 && x < p.W && y >= 0 && y < p.H;
    const v3 d = in ? primary_dir(p, x, y) : splat(0.0f);
    stnt(out + 2 * i, f4(p.eye[0], p.eye[1], p.eye[2], 0.0f));
    stnt(out + 2 * i + 1, f4(d.x, d.y, d.z, __builtin_inff()));
  }
}

// The blocks of a query: a block per kTB rays, at most the waves the chip holds twice over (256 CUs x 28 waves); each
// lane (each wave, with refill) strides over the list.
constexpr int kRayBlocksMax = 256 * 28;
WfStack stack_of(const RayQuery& q) {
  if (q.spill) return WfStack::kDeep;
  return q.stack_need <= kStackSmall ? WfStack::kSmall : WfStack::kFull;
}

}  // namespace

int ray_query_blocks(long long n) { return (int)std::min<long long>((n + kTB - 1) / kTB, kRayBlocksMax); }

int launch_rays_closest(const RayQuery& q, void* hits, int variant, hipStream_t s) {
  if (q.n <= 0) return 0;
  const dim3 grid(ray_query_blocks(q.n)), block(kTB);
  const WfStack kind = stack_of(q);
  const bool wide = variant == kRaysRefill && q.wide && kind != WfStack::kDeep;
  with_stack(kind, [&](auto ks, auto deep) {
    if (variant != kRaysRefill)
      hipLaunchKernelGGL((rays_closest_lane<ks(), deep()>), grid, block, 0, s, q, (float4*)hits);
    else if (wide)
      hipLaunchKernelGGL((rays_closest_refill<ks(), false, true>), grid, block, 0, s, q, (float4*)hits);
    else
      hipLaunchKernelGGL((rays_closest_refill<ks(), deep(), false>), grid, block, 0, s, q, (float4*)hits);
  });
  return (int)hipGetLastError();
}

int launch_rays_occluded(const RayQuery& q, void* out, int variant, hipStream_t s) {
  if (q.n <= 0) return 0;
  const dim3 grid(ray_query_blocks(q.n)), block(kTB);
  const WfStack kind = stack_of(q);
  const bool refill = variant == kRaysRefill;
  const bool wide = q.wide && !(refill && kind == WfStack::kDeep);
  with_stack(kind, [&](auto ks, auto deep) {
    if (!refill) {
      const auto kernel = wide ? rays_occluded_lane<ks(), deep(), true> : rays_occluded_lane<ks(), deep(), false>;
      hipLaunchKernelGGL(kernel, grid, block, 0, s, q, (uint8_t*)out);
    } else if (wide) {
      hipLaunchKernelGGL((rays_occluded_refill<ks(), false, true>), grid, block, 0, s, q, (uint8_t*)out);
    } else {
      hipLaunchKernelGGL((rays_occluded_refill<ks(), deep(), false>), grid, block, 0, s, q, (uint8_t*)out);
    }
  });
  return (int)hipGetLastError();
}

int launch_rays_primary(const PTParams& p, const void* xy, long long n, void* rays_out, hipStream_t s) {
  if (n <= 0) return 0;
  const int blocks = (int)std::min<long long>((n + 255) / 256, 256 * 8);
  hipLaunchKernelGGL(rays_primary_k, dim3(blocks), dim3(256), 0, s, p, (const int2*)xy, n, (float4*)rays_out);
  return (int)hipGetLastError();
}

}  // namespace ptk

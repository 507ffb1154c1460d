// kernels_bvh.hip — GPU LBVH builder for dynamic scenes.
//
// The reference builds its BVH once, on the host, with a recursive SAH sweep (buildBVHwithSAH, Utils/BVH.h:42-173,
// called at main.cpp:88-96 with leaf size 8) and uploads it as BVHNode_encoded texels (main.cpp:122-151). A scene
// whose triangles move every frame cannot afford that (a recursive sort per node). This builder produces the SAME
// buffer formats on the device — triangles in leaf order (Triangle_encoded, 15 RGB32F texels each) and
// BVHNode_encoded nodes with the dummy node 0 and the root at node 1 — so every consumer of the reference's buffers
// (the path tracer, the host decode in capi_draw_pt.hip, the CPU oracle) takes them unchanged. It is a different tree than
// the SAH builder's (no GPU builder can reproduce a host sort-and-sweep bit for bit); rendering over it is checked
// against the oracle walking the same buffers (tests/test_gpu_bvh.py).
//
// Algorithm: Karras, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees" (HPG 2012):
//   1. centroid c = (p1 + p2 + p3) / 3 (cmpx's centre, BVH.h:25-29) and the centroid bounds (wave max/min, one
//      ordered-int atomic per wave);
//   2. 30-bit Morton code of the centroid quantised to 1024 cells per axis, key = code << b | index (b bits of
//      index: keys are unique, so the radix tree is fully determined and the build deterministic);
//   3. rocPRIM radix sort of the keys (30 + b bits);
//   4. one thread per internal node finds its key range and split (the highest differing key bit);
//   5. bottom-up refit: each primitive walks towards the root; the second child to arrive (one acq_rel atomic per
//      node) computes the box as the union of its children — min/max are exact, so a node box equals the
//      reference's per-triangle min/max loop (BVH.h:52-67) over the same triangles;
//   6. nodes whose range holds <= leaf_n triangles become leaves (their subtrees are dropped); a scan over
//      "reachable" flags (internal nodes first, in Karras order, then single-triangle leaves) numbers the output
//      nodes from 1 (the root), and the emit kernel writes BVHNode_encoded texels and the triangles in key order.
// HBM traffic is a few passes over 16-64 B per triangle: for the 30.6 k-triangle bench scene the build is bound
// by launch latency and the sort's passes, not bytes.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdint>

#include "glsl_builtins.h"
#include "pt_device.h"

namespace ptk {

namespace {

constexpr int kTriFloats = 45;   // Triangle_encoded (Utils/Triangle.h:12-24)
constexpr int kNodeFloats = 12;  // BVHNode_encoded (Utils/BVH.h:18-22)

__device__ __forceinline__ unsigned ordered(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
// glm::min / glm::max (a < b ? ... as the reference evaluates them)
__device__ __forceinline__ float gmin(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float gmax(float a, float b) { return a < b ? b : a; }

// p1 at t[0..2], p2 at t[o2..], p3 at t[o3..] (Triangle_encoded: 3, 6; the raster vertex list: 6, 12)
__device__ __forceinline__ float3 centroid(const float* t, int o2, int o3) {
  return float3{((t[0] + t[o2]) + t[o3]) / 3.0f, ((t[1] + t[o2 + 1]) + t[o3 + 1]) / 3.0f,
                ((t[2] + t[o2 + 2]) + t[o3 + 2]) / 3.0f};
}

// 1. centroids and their bounds. bounds[0..2] = ordered min, bounds[3..5] = ordered max (pre-set by the host).
__global__ void __launch_bounds__(256) lbvh_centroids(const float* __restrict__ tri, int n, TriLayout lay,
                                                       float4* __restrict__ cen, unsigned* __restrict__ bounds) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (i < n) {
    const float3 c = centroid(tri + (size_t)i * lay.stride, lay.o2, lay.o3);
    cen[i] = float4{c.x, c.y, c.z, 0.0f};
    const float cc[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int a = 0; a < 3; ++a)  // NaN centroids (NaN vertices) stay out of the bounds
      if (cc[a] == cc[a]) lo[a] = hi[a] = ordered(cc[a]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], o));
      hi[a] = max(hi[a], (unsigned)__shfl_xor((int)hi[a], o));
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&bounds[a], lo[a]);
      atomicMax(&bounds[3 + a], hi[a]);
    }
  }
}

__device__ __forceinline__ uint64_t spread10(uint32_t v) {  // 10 bits -> every third bit of 30
  uint64_t x = v & 0x3ffu;
  x = (x | (x << 16)) & 0x030000FFull;
  x = (x | (x << 8)) & 0x0300F00Full;
  x = (x | (x << 4)) & 0x030C30C3ull;
  x = (x | (x << 2)) & 0x09249249ull;
  return x;
}

__device__ __forceinline__ uint32_t cell(float c, float lo, float hi) {
  const float ext = hi - lo;
  const float q = ext > 0.0f ? (c - lo) / ext : 0.0f;
  const float v = floorf(q * 1024.0f);
  return !(v == v) || v < 0.0f ? 0u : (v > 1023.0f ? 1023u : (uint32_t)v);  // NaN -> cell 0
}

// 2. keys: Morton code (x in the highest of each bit triple) above b index bits
__global__ void __launch_bounds__(256) lbvh_keys(const float4* __restrict__ cen, int n, const unsigned* bounds,
                                                  int ibits, uint64_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 c = cen[i];
  const float lx = unordered(bounds[0]), ly = unordered(bounds[1]), lz = unordered(bounds[2]);
  const float hx = unordered(bounds[3]), hy = unordered(bounds[4]), hz = unordered(bounds[5]);
  const uint64_t m = (spread10(cell(c.x, lx, hx)) << 2) | (spread10(cell(c.y, ly, hy)) << 1) |
                     spread10(cell(c.z, lz, hz));
  keys[i] = (m << ibits) | (uint64_t)i;
}

__device__ __forceinline__ int delta(const uint64_t* __restrict__ k, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  return __clzll(k[i] ^ k[j]);
}

// 4. internal node i of n-1: its range [first, last] and children. child refs: >= 0 internal node, < 0 primitive
// (~sorted position). parent[] indexes internal nodes 0..n-2, then primitives at n-1+p.
__global__ void __launch_bounds__(256) lbvh_karras(const uint64_t* __restrict__ k, int n, int2* __restrict__ child,
                                                    int2* __restrict__ range, int* __restrict__ parent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n - 1) return;
  const int d = delta(k, n, i, i + 1) - delta(k, n, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = delta(k, n, i, i - d);
  int lmax = 2;
  while (delta(k, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(k, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(k, n, i, j);
  int s = 0;
  for (int div = 2;; div <<= 1) {
    const int t = (l + div - 1) / div;
    if (delta(k, n, i, i + (s + t) * d) > dnode) s += t;
    if (t == 1) break;
  }
  const int gamma = i + s * d + min(d, 0);
  const int first = min(i, j), last = max(i, j);
  const int left = first == gamma ? ~gamma : gamma;
  const int right = last == gamma + 1 ? ~(gamma + 1) : gamma + 1;
  child[i] = int2{left, right};
  range[i] = int2{first, last};
  parent[left >= 0 ? left : n - 1 + ~left] = i;
  parent[right >= 0 ? right : n - 1 + ~right] = i;
  if (i == 0) parent[0] = -1;
}

// 5. bottom-up boxes. box[e] (e: internal 0..n-2, primitive n-1+p) = lo.xyz, hi.xyz as 2 float4.
__global__ void __launch_bounds__(256) lbvh_refit(const float* __restrict__ tri, TriLayout lay,
                                                   const uint64_t* __restrict__ k, int n, int ibits,
                                                   const int2* __restrict__ child, const int* __restrict__ parent,
                                                   float4* box, int* flags, int* __restrict__ order) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint64_t mask = (ibits >= 64) ? ~0ull : ((1ull << ibits) - 1ull);
  const int orig = (int)(k[p] & mask);
  if (order) order[p] = orig;
  const float* t = tri + (size_t)orig * lay.stride;
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {  // BVH.h:54-66: min(p1, min(p2, p3)) per axis
    lo[a] = gmin(t[a], gmin(t[lay.o2 + a], t[lay.o3 + a]));
    hi[a] = gmax(t[a], gmax(t[lay.o2 + a], t[lay.o3 + a]));
  }
  int e = n - 1 + p;
  box[2 * e] = float4{lo[0], lo[1], lo[2], 0.0f};
  box[2 * e + 1] = float4{hi[0], hi[1], hi[2], 0.0f};
  int node = parent[e];
  while (node >= 0) {
    // the first child to arrive stops; the second sees both boxes (acq_rel orders the box stores and loads)
    if (__hip_atomic_fetch_add(&flags[node], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const int2 c = child[node];
    const int a = c.x >= 0 ? c.x : n - 1 + ~c.x, b = c.y >= 0 ? c.y : n - 1 + ~c.y;
    const float4 al = box[2 * a], ah = box[2 * a + 1], bl = box[2 * b], bh = box[2 * b + 1];
    box[2 * node] = float4{gmin(al.x, bl.x), gmin(al.y, bl.y), gmin(al.z, bl.z), 0.0f};
    box[2 * node + 1] = float4{gmax(ah.x, bh.x), gmax(ah.y, bh.y), gmax(ah.z, bh.z), 0.0f};
    node = parent[node];
  }
}

// 6a. reachable output nodes: internal node i unless its parent's range fits a leaf; primitive p only when its
// parent is an interior output node (a range > leaf_n). n == 1: the single primitive is the root leaf.
__global__ void __launch_bounds__(256) lbvh_mark(int n, int leaf_n, const int2* __restrict__ range,
                                                  const int* __restrict__ parent, int* __restrict__ keep) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * n - 1) return;
  const int par = parent[e];
  int k;
  if (par < 0) k = 1;  // the root (internal 0, or the lone primitive when n == 1)
  else {
    const int2 r = range[par];
    k = r.y - r.x + 1 > leaf_n;
  }
  keep[e] = k;
}

// 6b. BVHNode_encoded texels (childs, leafInfo, AA, BB) and the dummy node 0 (main.cpp:88-94).
__global__ void __launch_bounds__(256) lbvh_emit(int n, int leaf_n, const int2* __restrict__ child,
                                                  const int2* __restrict__ range, const int* __restrict__ keep,
                                                  const int* __restrict__ id, const float4* __restrict__ box,
                                                  float* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) {
    const float dummy[kNodeFloats] = {255, 128, 0, 30, 0, 0, 1, 1, 0, 0, 1, 0};
    for (int q = 0; q < kNodeFloats; ++q) out[q] = dummy[q];
  }
  if (e >= 2 * n - 1 || !keep[e]) return;
  float* o = out + (size_t)(1 + id[e]) * kNodeFloats;
  int first, count;
  bool leaf;
  if (e < n - 1) {
    const int2 r = range[e];
    first = r.x;
    count = r.y - r.x + 1;
    leaf = count <= leaf_n;
  } else {
    first = e - (n - 1);
    count = 1;
    leaf = true;
  }
  if (leaf) {
    o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
    o[3] = (float)count; o[4] = (float)first; o[5] = 0.0f;
  } else {
    const int2 c = child[e];
    const int a = c.x >= 0 ? c.x : n - 1 + ~c.x, b = c.y >= 0 ? c.y : n - 1 + ~c.y;
    o[0] = (float)(1 + id[a]); o[1] = (float)(1 + id[b]); o[2] = 0.0f;
    o[3] = 0.0f; o[4] = 0.0f; o[5] = 0.0f;
  }
  const float4 lo = box[2 * e], hi = box[2 * e + 1];
  o[6] = lo.x; o[7] = lo.y; o[8] = lo.z;
  o[9] = hi.x; o[10] = hi.y; o[11] = hi.z;
}

// 6c. triangles in key (leaf) order
__global__ void __launch_bounds__(256) lbvh_reorder(const float* __restrict__ tri, const uint64_t* __restrict__ k,
                                                     int n, int ibits, float* __restrict__ out) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)n * kTriFloats) return;
  const int p = (int)(f / kTriFloats), q = (int)(f - (size_t)p * kTriFloats);
  const uint64_t mask = (1ull << ibits) - 1ull;
  out[f] = tri[(size_t)(k[p] & mask) * kTriFloats + q];
}

// Triangle_encoded texels -> the path tracer's tri_geom / tri_shade records (capi_draw_pt.hip get_scene's host decode,
// same built-ins, so the same bits): the device decode of GPU-built scenes, whose triangles never leave the device.
__global__ void __launch_bounds__(256) decode_tris_kernel(const float* __restrict__ te, int n, float4* __restrict__ geom,
                                                           float4* __restrict__ shade) {
  using namespace glsl;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* f = te + (size_t)i * kTriFloats;
  const v3 p1 = mk(f[0], f[1], f[2]), p2 = mk(f[3], f[4], f[5]), p3 = mk(f[6], f[7], f[8]);
  const v3 N = normalize(cross(sub(p2, p1), sub(p3, p1)));  // hitTriangle (path_tracing.frag:227)
  geom[4 * i + 0] = float4{p1.x, p1.y, p1.z, dot(N, p1)};
  geom[4 * i + 1] = float4{p2.x, p2.y, p2.z, 0.0f};
  geom[4 * i + 2] = float4{p3.x, p3.y, p3.z, 0.0f};
  geom[4 * i + 3] = float4{N.x, N.y, N.z, 0.0f};
  float4* s = shade + 9 * (size_t)i;
  s[0] = float4{f[9], f[10], f[11], f[12]};
  s[1] = float4{f[13], f[14], f[15], f[16]};
  s[2] = float4{f[17], f[18], f[19], f[20]};
  s[3] = float4{f[21], f[22], f[23], f[24]};
  s[4] = float4{f[25], f[26], f[27], f[28]};
  s[5] = float4{f[29], f[30], f[31], f[32]};
  s[6] = float4{f[33], f[34], f[35], f[42]};
  s[7] = float4{f[36], f[37], f[38], f[39]};
  s[8] = float4{f[40], f[41], 0.0f, 0.0f};
}


// ---------------------------------------------------------------------------------------------------------------
// PLOC top (quality > 0): the LBVH's leaves (ranges of <= leaf_n Morton-ordered triangles, their boxes exact) are
// kept, and the tree above them is rebuilt by Parallel Locally-Ordered Clustering (Meister & Bittner, 2018): every
// cluster in Morton order finds, within r positions, the neighbour whose merged box has the smallest surface area
// (ties: the nearer-indexed pair, a total order on pairs, so the globally best pair is always mutual and every
// iteration merges at least once); mutual pairs merge into a new node at the lower position, the array is
// compacted, until one cluster is left. Clusters: >= 0 PLOC node (creation order), < 0 leaf ~L (Morton rank).
__device__ __forceinline__ float half_area(float4 lo, float4 hi) {
  const float dx = hi.x - lo.x, dy = hi.y - lo.y, dz = hi.z - lo.z;
  return (dx * dy + dy * dz) + dz * dx;
}

// leaves in Morton order: start[first] = 1 for every reachable LBVH leaf
__global__ void __launch_bounds__(256) ploc_leafstart(int n, int leaf_n, const int2* __restrict__ range,
                                                       const int* __restrict__ keep, int* __restrict__ start) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * n - 1 || !keep[e]) return;
  if (e < n - 1) {
    const int2 r = range[e];
    if (r.y - r.x + 1 <= leaf_n) start[r.x] = 1;
  } else {
    start[e - (n - 1)] = 1;
  }
}

__global__ void __launch_bounds__(256) ploc_init(int n, int leaf_n, const int2* __restrict__ range,
                                                  const int* __restrict__ keep, const int* __restrict__ rank,
                                                  const int* __restrict__ start, const float4* __restrict__ box,
                                                  int2* __restrict__ leaf, float4* __restrict__ leafbox,
                                                  int* __restrict__ C, float4* __restrict__ cbox, int* __restrict__ cnt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) {
    cnt[0] = rank[n - 1] + start[n - 1];  // clusters (= leaves, M)
    cnt[1] = 0;                           // PLOC nodes created
    cnt[4] = cnt[0];
  }
  if (e >= 2 * n - 1 || !keep[e]) return;
  int first, count;
  if (e < n - 1) {
    const int2 r = range[e];
    count = r.y - r.x + 1;
    if (count > leaf_n) return;
    first = r.x;
  } else {
    first = e - (n - 1);
    count = 1;
  }
  const int L = rank[first];
  leaf[L] = int2{first, count};
  C[L] = ~L;
  cbox[2 * L] = leafbox[2 * L] = box[2 * e];
  cbox[2 * L + 1] = leafbox[2 * L + 1] = box[2 * e + 1];
}

__global__ void __launch_bounds__(256) ploc_nn(const int* __restrict__ cnt, const float4* __restrict__ cbox, int r,
                                                int* __restrict__ nn) {
  const int n = cnt[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 lo = cbox[2 * i], hi = cbox[2 * i + 1];
  float best = __builtin_inff();
  int bj = -1, bs = 1;
  const int j0 = max(0, i - r), j1 = min(n - 1, i + r);
  // Pairs are ranked by (area, j != (i ^ 1), min(i, j), max(i, j)): a total order on pairs, so the globally best pair
  // is mutual and every iteration merges; on runs of equal areas (coincident points, NaN boxes) the sibling pairs
  // (2k, 2k + 1) rank first and are all mutual, so such a run halves per iteration instead of losing one cluster.
  for (int j = j0; j <= j1; ++j) {  // ascending j: for equal (area, sibling flag) the smaller pair comes first
    if (j == i) continue;
    // the union in position order (lower position first), as ploc_compact merges: with NaN coordinates glm's
    // min/max depend on the operand order, and the area must be the same seen from either end of the pair
    const float4 l2 = cbox[2 * j], h2 = cbox[2 * j + 1];
    const float4 la = j < i ? l2 : lo, lb = j < i ? lo : l2, ha = j < i ? h2 : hi, hb = j < i ? hi : h2;
    float a = half_area(float4{gmin(la.x, lb.x), gmin(la.y, lb.y), gmin(la.z, lb.z), 0.0f},
                        float4{gmax(ha.x, hb.x), gmax(ha.y, hb.y), gmax(ha.z, hb.z), 0.0f});
    a = a == a ? a : __builtin_inff();  // NaN boxes rank last: the pair order stays total, so PLOC ends
    const int sj = j != (i ^ 1);
    if (bj < 0 || a < best || (a == best && sj < bs)) {
      best = a;
      bj = j;
      bs = sj;
    }
  }
  nn[i] = bj < 0 ? i : bj;
}

// f[i] = (merges here << 32) | survives, for i < N (zero past the live clusters)
__global__ void __launch_bounds__(256) ploc_flags(const int* __restrict__ cnt, const int* __restrict__ nn, int N,
                                                   uint64_t* __restrict__ f) {
  const int n = cnt[0];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  if (i >= n) {
    f[i] = 0;
    return;
  }
  const int j = nn[i];
  const bool mutual = j != i && nn[j] == i;
  f[i] = ((uint64_t)(mutual && i < j) << 32) | (uint64_t)!(mutual && i > j);
}

__global__ void __launch_bounds__(256) ploc_compact(const int* __restrict__ cin, int* __restrict__ cout,
                                                     const int* __restrict__ C, const float4* __restrict__ cbox,
                                                     const int* __restrict__ nn, const uint64_t* __restrict__ f,
                                                     const uint64_t* __restrict__ pf, int* __restrict__ C2,
                                                     float4* __restrict__ cbox2, int2* __restrict__ nchild,
                                                     float4* __restrict__ nbox) {
  const int n = cin[0], created = cin[1];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t fi = f[i], pi = pf[i];
  if (i == n - 1) {
    const uint64_t tot = pi + fi;
    cout[0] = (int)(tot & 0xffffffffu);
    cout[1] = created + (int)(tot >> 32);
  }
  if (!(fi & 1u)) return;
  const int p = (int)(pi & 0xffffffffu);
  if (fi >> 32) {
    const int j = nn[i], k = created + (int)(pi >> 32);
    const float4 al = cbox[2 * i], ah = cbox[2 * i + 1], bl = cbox[2 * j], bh = cbox[2 * j + 1];
    const float4 lo = float4{gmin(al.x, bl.x), gmin(al.y, bl.y), gmin(al.z, bl.z), 0.0f};
    const float4 hi = float4{gmax(ah.x, bh.x), gmax(ah.y, bh.y), gmax(ah.z, bh.z), 0.0f};
    nchild[k] = int2{C[i], C[j]};
    nbox[2 * k] = lo;
    nbox[2 * k + 1] = hi;
    C2[p] = k;
    cbox2[2 * p] = lo;
    cbox2[2 * p + 1] = hi;
  } else {
    C2[p] = C[i];
    cbox2[2 * p] = cbox[2 * i];
    cbox2[2 * p + 1] = cbox[2 * i + 1];
  }
}

// BVHNode_encoded: PLOC node k -> node 1 + (M - 2 - k) (the root, created last, is node 1); leaf L -> node M + L
__global__ void __launch_bounds__(256) ploc_emit(const int* __restrict__ cnt, int N, const int2* __restrict__ nchild,
                                                  const float4* __restrict__ nbox, const int2* __restrict__ leaf,
                                                  const float4* __restrict__ cbox_leaf, float* __restrict__ out) {
  const int M = cnt[4];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) {
    const float dummy[kNodeFloats] = {255, 128, 0, 30, 0, 0, 1, 1, 0, 0, 1, 0};
    for (int q = 0; q < kNodeFloats; ++q) out[q] = dummy[q];
  }
  auto id = [&](int ref) { return ref >= 0 ? 1 + (M - 2 - ref) : M + ~ref; };
  if (e < M - 1) {
    float* o = out + (size_t)id(e) * kNodeFloats;
    const int2 c = nchild[e];
    const float4 lo = nbox[2 * e], hi = nbox[2 * e + 1];
    o[0] = (float)id(c.x); o[1] = (float)id(c.y); o[2] = 0.0f;
    o[3] = 0.0f; o[4] = 0.0f; o[5] = 0.0f;
    o[6] = lo.x; o[7] = lo.y; o[8] = lo.z;
    o[9] = hi.x; o[10] = hi.y; o[11] = hi.z;
  }
  if (e < M) {
    float* o = out + (size_t)(M + e) * kNodeFloats;
    const int2 l = leaf[e];
    const float4 lo = cbox_leaf[2 * e], hi = cbox_leaf[2 * e + 1];
    o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
    o[3] = (float)l.y; o[4] = (float)l.x; o[5] = 0.0f;
    o[6] = lo.x; o[7] = lo.y; o[8] = lo.z;
    o[9] = hi.x; o[10] = hi.y; o[11] = hi.z;
  }
}

// Raster vertex list (pos3 + nrm3 per vertex, obj_loader.h:143-160) -> the G-buffer's records in leaf order, as
// pt_raster_pass_bind writes them on the host: (p1, original index bits), e1, e2, cross(e1, e2); the three normals.
__global__ void __launch_bounds__(256) decode_raster_kernel(const float* __restrict__ verts,
                                                             const int* __restrict__ order, int n,
                                                             float4* __restrict__ geom, float4* __restrict__ nrm) {
  using namespace glsl;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int oi = order[k];
  const float* f = verts + (size_t)oi * 18;
  const v3 p1 = mk(f[0], f[1], f[2]), p2 = mk(f[6], f[7], f[8]), p3 = mk(f[12], f[13], f[14]);
  const v3 e1 = sub(p2, p1), e2 = sub(p3, p1), ng = cross(e1, e2);
  geom[4 * k + 0] = float4{p1.x, p1.y, p1.z, __int_as_float(oi)};
  geom[4 * k + 1] = float4{e1.x, e1.y, e1.z, 0.0f};
  geom[4 * k + 2] = float4{e2.x, e2.y, e2.z, 0.0f};
  geom[4 * k + 3] = float4{ng.x, ng.y, ng.z, 0.0f};
  nrm[3 * k + 0] = float4{f[3], f[4], f[5], 0.0f};
  nrm[3 * k + 1] = float4{f[9], f[10], f[11], 0.0f};
  nrm[3 * k + 2] = float4{f[15], f[16], f[17], 0.0f};
}

// Displacement records of a bound rasterize pass (pt_raster_pass_set_prev_vertices): per triangle in leaf order, its
// three vertices' prev - cur of the two vertex lists (original order, geom[4k].w = the original index); .w = 1 when
// any of the nine components is non-zero (the moved flag gb_finish branches on). An index outside the lists (not
// written by either bind) leaves a zero record.
__global__ void __launch_bounds__(256) raster_disp_kernel(const float4* __restrict__ geom,
                                                           const float* __restrict__ prev,
                                                           const float* __restrict__ cur, int n,
                                                           float4* __restrict__ disp) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int oi = __float_as_int(geom[4 * k].w);
  float d[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool moved = false;
  if (oi >= 0 && oi < n) {
    const float *a = prev + (size_t)oi * 18, *b = cur + (size_t)oi * 18;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        d[3 * j + c] = a[6 * j + c] - b[6 * j + c];
        moved = moved || d[3 * j + c] != 0.0f;
      }
  }
  const float w = moved ? 1.0f : 0.0f;
#pragma unroll
  for (int j = 0; j < 3; ++j) disp[3 * k + j] = float4{d[3 * j], d[3 * j + 1], d[3 * j + 2], w};
}

// ---------------------------------------------------------------------------------------------------------------
// Walk trees of a built tree (lbvh_trees_launch): the packed binary tree, the leaf list and the 4-wide tree the
// traversal kernels read, derived from the BVHNode_encoded texels without a trip through the host. Their content is
// defined by pack_bvh and pack_wide (host_trees.cpp) and upload_leaves (capi_draw_pt.hip) (greedy collapse, no keep / direct nodes); every
// float32 operation below is spelled as those evaluate it (-ffp-contract=off).
//   trees_local   per node: parent links; per interior node the child list of the 4-wide node it would root (local:
//                 at most two nodes are opened, so only nodes up to three levels below are read)
//   trees_sizes   bottom-up, lbvh_refit's arrive-second pattern: interior nodes and 4-wide nodes below each node
//   trees_index   per interior node: walk up; its preorder index is the sum of 1 + (left sibling's size) on the way
//   trees_emit    per leaf its list entry; per interior node its packed record, and a walk down from the root
//                 through the child lists (preorder index + size = an O(1) ancestor test) that finds whether it is
//                 a 4-wide node, which one, and the stack entries held above it
// Every loop is bounded by the tree's depth (and by the node count, should the texels be no tree) or by 4; no
// thread waits on another.
enum { kInfoRoot = 0, kInfoNeed, kInfoLeaves, kInfoRoot4, kInfoNeed4, kInfoWide, kInfoNan, kInfoSpare, kInfoBin,
       kInfoErr, kInfoInts };

struct NodeTex {
  int left, right, n, first;
};
__device__ __forceinline__ NodeTex node_tex(const float* __restrict__ nodes, int i) {
  const float* f = nodes + (size_t)i * kNodeFloats;
  return NodeTex{(int)f[0], (int)f[1], (int)f[3], (int)f[4]};
}
__device__ __forceinline__ bool node_ok(int i, int nn) { return i >= 1 && i < nn; }
__device__ __forceinline__ int leaf_ref_of(const NodeTex& t) { return -(t.first * 16 + t.n) - 1; }

// host_trees.cpp sah_area: extents clamped as std::max(d, 0.0f) evaluates ((d < 0) ? 0 : d, so NaN stays NaN)
__device__ __forceinline__ float tex_area(const float* __restrict__ nodes, int i) {
  const float* f = nodes + (size_t)i * kNodeFloats;
  float dx = f[9] - f[6], dy = f[10] - f[7], dz = f[11] - f[8];
  dx = dx < 0.0f ? 0.0f : dx;
  dy = dy < 0.0f ? 0.0f : dy;
  dz = dz < 0.0f ? 0.0f : dz;
  return (dx * dy + dy * dz) + dz * dx;
}

__global__ void __launch_bounds__(256) trees_local(const float* __restrict__ nodes, int nn, int* __restrict__ parent,
                                                    int4* __restrict__ ch, int2* __restrict__ sz,
                                                    int* __restrict__ leaf, int* __restrict__ info,
                                                    const int* __restrict__ refit_err) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nn) return;
  sz[i] = int2{0, 0};
  ch[i] = int4{-1, -1, -1, -1};
  if (i == 0) {
    leaf[0] = 0;
    if (refit_err && *refit_err) atomicOr(&info[kInfoErr], 4);  // a refit before this stage met a bad index
    return;
  }
  const NodeTex t = node_tex(nodes, i);
  leaf[i] = t.n > 0;
  if (t.n > 0) return;
  if (!node_ok(t.left, nn) || !node_ok(t.right, nn) || t.left == t.right) {
    atomicOr(&info[kInfoErr], 1);
    return;
  }
  parent[t.left] = i;
  parent[t.right] = i;
  // pack_wide's greedy collapse: open the interior child of the greatest area (strict >, from -1: the first in the
  // current order wins ties, area 0 qualifies, NaN never does) until four slots are used
  int c[4] = {t.left, t.right, -1, -1};
  float a[4] = {tex_area(nodes, t.left), tex_area(nodes, t.right), 0.0f, 0.0f};
  int nc = 2;
  for (int round = 0; round < 2; ++round) {
    int best = -1;
    float ba = -1.0f;
    for (int k = 0; k < 4; ++k)
      if (k < nc && node_tex(nodes, c[k]).n <= 0 && a[k] > ba) {
        ba = a[k];
        best = k;
      }
    if (best < 0) break;
    const NodeTex b = node_tex(nodes, c[best]);
    if (!node_ok(b.left, nn) || !node_ok(b.right, nn)) {
      atomicOr(&info[kInfoErr], 1);
      return;
    }
    for (int k = 3; k > 0; --k)
      if (k > best + 1 && k <= nc) {
        c[k] = c[k - 1];
        a[k] = a[k - 1];
      }
    c[best] = b.left;
    a[best] = tex_area(nodes, b.left);
    c[best + 1] = b.right;
    a[best + 1] = tex_area(nodes, b.right);
    ++nc;
  }
  // PT_WIDE_ORDER: a stable sort by area, descending (std::stable_sort's insertion sort of so few elements)
  for (int k = 1; k < 4; ++k) {
    if (k >= nc) break;
    const int cv = c[k];
    const float av = a[k];
    if (av > a[0]) {
      for (int j = k; j > 0; --j) {
        c[j] = c[j - 1];
        a[j] = a[j - 1];
      }
      c[0] = cv;
      a[0] = av;
    } else {
      int j = k;
      while (j > 0 && av > a[j - 1]) {
        c[j] = c[j - 1];
        a[j] = a[j - 1];
        --j;
      }
      c[j] = cv;
      a[j] = av;
    }
  }
  ch[i] = int4{c[0], c[1], c[2], c[3]};
}

__global__ void __launch_bounds__(256) trees_sizes(const float* __restrict__ nodes, int nn,
                                                    const int* __restrict__ parent, const int4* __restrict__ ch,
                                                    const int* __restrict__ leaf, int2* sz, int* flags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 1 || i >= nn || !leaf[i]) return;
  int node = parent[i];
  for (int step = 0; step < nn && node_ok(node, nn); ++step) {
    // the first child to arrive stops; the second sees every size below (acq_rel orders the stores and loads)
    if (__hip_atomic_fetch_add(&flags[node], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const NodeTex t = node_tex(nodes, node);
    const int4 c4 = ch[node];
    const int c[4] = {c4.x, c4.y, c4.z, c4.w};
    int wide = 1;
    for (int k = 0; k < 4; ++k)
      if (c[k] >= 0) wide += sz[c[k]].y;  // a leaf's sizes are 0
    sz[node] = int2{1 + sz[t.left].x + sz[t.right].x, wide};
    node = parent[node];
  }
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

__global__ void __launch_bounds__(256) trees_index(const float* __restrict__ nodes, int nn,
                                                    const int* __restrict__ parent, const int* __restrict__ leaf,
                                                    const int2* __restrict__ sz, int* __restrict__ idx,
                                                    int* __restrict__ info) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  int depth = 0;
  if (v >= 1 && v < nn && !leaf[v]) {
    int k = 0, x = v;
    depth = 1;
    for (int step = 0; step < nn; ++step) {
      const int p = parent[x];
      if (!node_ok(p, nn)) break;
      const int l = node_tex(nodes, p).left;
      k += 1 + (x != l && node_ok(l, nn) ? sz[l].x : 0);
      ++depth;
      x = p;
    }
    idx[v] = k;
  }
  depth = wave_max(depth);
  if ((threadIdx.x & 63) == 0 && depth) atomicMax(&info[kInfoNeed], depth);
}

__global__ void __launch_bounds__(256) trees_emit(const float* __restrict__ nodes, int nn, const int4* __restrict__ ch,
                                                   const int* __restrict__ leaf, const int* __restrict__ leafpos,
                                                   const int2* __restrict__ sz, const int* __restrict__ idx,
                                                   float4* __restrict__ bin, int cap_bin, float4* __restrict__ leaves,
                                                   int cap_leaves, float4* __restrict__ wide, int cap_wide,
                                                   int* __restrict__ info) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  int need4 = 0, bits = 0;  // bits: 1 NaN child box, 2 child index out of range, 4 a record past its part's room
  if (v >= 1 && v < nn) {
    const NodeTex t = node_tex(nodes, v);
    const float* f = nodes + (size_t)v * kNodeFloats;
    if (v == 1) {
      info[kInfoRoot] = info[kInfoRoot4] = t.n > 0 ? leaf_ref_of(t) : 0;
      info[kInfoBin] = sz[1].x;
      info[kInfoWide] = sz[1].y;
    }
    if (v == nn - 1) info[kInfoLeaves] = leafpos[v] + leaf[v];
    if (t.n > 0) {
      const int p = leafpos[v];
      if (p < cap_leaves) {
        leaves[2 * p] = float4{f[6], f[7], f[8], __int_as_float(leaf_ref_of(t))};
        leaves[2 * p + 1] = float4{f[9], f[10], f[11], 0.0f};
      } else {
        bits |= 4;
      }
    } else if (node_ok(t.left, nn) && node_ok(t.right, nn)) {
      const int k = idx[v];
      {  // pack_bvh's record
        const NodeTex L = node_tex(nodes, t.left), R = node_tex(nodes, t.right);
        const float* l = nodes + (size_t)t.left * kNodeFloats;
        const float* r = nodes + (size_t)t.right * kNodeFloats;
        const int rl = L.n > 0 ? leaf_ref_of(L) : k + 1;
        const int rr = R.n > 0 ? leaf_ref_of(R) : k + 1 + sz[t.left].x;
        if (k >= 0 && k < cap_bin) {
          bin[4 * k + 0] = float4{l[6], l[7], l[8], l[9]};
          bin[4 * k + 1] = float4{l[10], l[11], r[6], r[7]};
          bin[4 * k + 2] = float4{r[8], r[9], r[10], r[11]};
          bin[4 * k + 3] = float4{__int_as_float(rl), __int_as_float(rr), 0.0f, 0.0f};
        } else {
          bits |= 4;
        }
      }
      // down from the root through the 4-wide child lists: w = the 4-wide node's preorder index, acc = pack_wide's
      int x = 1, w = 0, acc = 0;
      bool is_wide = false;
      for (int step = 0; step < nn; ++step) {
        if (x == v) {
          is_wide = true;
          break;
        }
        const int4 c4 = ch[x];
        const int c[4] = {c4.x, c4.y, c4.z, c4.w};
        int nc = 0, next = -1, wn = w + 1;
        for (int s = 0; s < 4; ++s) {
          if (c[s] < 0) continue;
          ++nc;
          if (next >= 0 || leaf[c[s]]) continue;
          const int2 cs = sz[c[s]];
          const int ci = idx[c[s]];
          if (ci <= k && k < ci + cs.x) next = c[s];
          else wn += cs.y;
        }
        if (next < 0 || nc < 2) break;  // v was opened into a 4-wide node above it
        x = next;
        w = wn;
        acc += nc - 1;
      }
      if (is_wide) {
        const int4 c4 = ch[v];
        const int c[4] = {c4.x, c4.y, c4.z, c4.w};
        int nc = 0;
        for (int s = 0; s < 4; ++s) nc += c[s] >= 0;
        need4 = acc + nc;  // here = acc + nc - 1; need = max(need, here + 1)
        if (w >= 0 && w < cap_wide) {
          float q[28];
          int wn = w + 1;
          for (int s = 0; s < 4; ++s) {
            int ref = kNoneRef;
            float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
            float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
            if (c[s] >= 0) {
              const float* b = nodes + (size_t)c[s] * kNodeFloats;
              for (int a = 0; a < 3; ++a) {
                lo[a] = b[6 + a];
                hi[a] = b[9 + a];
                if (lo[a] != lo[a] || hi[a] != hi[a]) bits |= 1;
              }
              const NodeTex ct = node_tex(nodes, c[s]);
              if (ct.n > 0) {
                ref = leaf_ref_of(ct);
              } else {
                ref = wn;
                wn += sz[c[s]].y;
              }
            }
            for (int a = 0; a < 3; ++a) {
              q[8 * a + s] = lo[a];
              q[8 * a + 4 + s] = hi[a];
            }
            q[24 + s] = __int_as_float(ref);
          }
          float4* o = wide + (size_t)kWideStride * w;
          for (int j = 0; j < 7; ++j) o[j] = float4{q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]};
          for (int j = 7; j < kWideStride; ++j) o[j] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        } else {
          bits |= 4;
        }
      }
    } else {
      bits |= 2;
    }
  }
  need4 = wave_max(need4);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) bits |= __shfl_xor(bits, o);
  if ((threadIdx.x & 63) == 0) {
    if (need4) atomicMax(&info[kInfoNeed4], need4);
    if (bits & 1) atomicOr(&info[kInfoNan], 1);
    if (bits & 6) atomicOr(&info[kInfoErr], bits >> 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Refit (lbvh_refit_nodes): geometry that moved but kept its triangles and their order keeps the tree's topology;
// only the boxes are recomputed, in the node texels where they lie. Defined by tests/lbvh_refit_ref.py.

// parent[child] = node for every interior node of a built tree (parent pre-set to -1: the root keeps it)
__global__ void __launch_bounds__(256) refit_link(const float* __restrict__ nodes, int nn, int* __restrict__ parent,
                                                   int* __restrict__ err) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 1 || i >= nn) return;
  const NodeTex t = node_tex(nodes, i);
  if (t.n > 0) return;
  if (!node_ok(t.left, nn) || !node_ok(t.right, nn) || t.left == t.right) {
    atomicOr(err, 1);
    return;
  }
  parent[t.left] = i;
  parent[t.right] = i;
}

// One thread per output node. A leaf folds its triangles' boxes in leaf order, starting from the first, stores AA / BB
// and climbs: lbvh_refit's arrive-second pattern over flags (zeroed by the host), the second child to arrive at a node
// storing gmin / gmax (left, right) of its children's texels. Interior nodes do nothing at entry. Every index read from
// a texel or a kept array is checked before it is followed; the climb is bounded by the depth (and by nn).
__global__ void __launch_bounds__(256) refit_nodes(float* nodes, int nn, const float* __restrict__ tri, int ntris,
                                                    TriLayout lay, const int* __restrict__ order,
                                                    const int* __restrict__ parent, int* flags, int* __restrict__ err) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 1 || i >= nn) return;
  float* f = nodes + (size_t)i * kNodeFloats;
  const int count = (int)f[3], first = (int)f[4];
  if (count <= 0) return;
  if (first < 0 || count > ntris || first > ntris - count) {
    atomicOr(err, 1);
    return;
  }
  float lo[3], hi[3];
  for (int j = 0; j < count; ++j) {
    const int o = order[first + j];
    if (o < 0 || o >= ntris) {
      atomicOr(err, 1);
      return;
    }
    const float* t = tri + (size_t)o * lay.stride;
#pragma unroll
    for (int a = 0; a < 3; ++a) {  // BVH.h:54-66: min(p1, min(p2, p3)) per axis
      const float tl = gmin(t[a], gmin(t[lay.o2 + a], t[lay.o3 + a]));
      const float th = gmax(t[a], gmax(t[lay.o2 + a], t[lay.o3 + a]));
      lo[a] = j == 0 ? tl : gmin(lo[a], tl);
      hi[a] = j == 0 ? th : gmax(hi[a], th);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    f[6 + a] = lo[a];
    f[9 + a] = hi[a];
  }
  int node = parent[i];
  for (int step = 0; step < nn && node_ok(node, nn); ++step) {
    // the first child to arrive stops; the second sees both boxes (acq_rel orders the box stores and loads)
    if (__hip_atomic_fetch_add(&flags[node], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    float* p = nodes + (size_t)node * kNodeFloats;
    const int l = (int)p[0], r = (int)p[1];
    if (!node_ok(l, nn) || !node_ok(r, nn)) {
      atomicOr(err, 1);
      return;
    }
    const float* lf = nodes + (size_t)l * kNodeFloats;
    const float* rf = nodes + (size_t)r * kNodeFloats;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = gmin(lf[6 + a], rf[6 + a]);
      hi[a] = gmax(lf[9 + a], rf[9 + a]);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p[6 + a] = lo[a];
      p[9 + a] = hi[a];
    }
    node = parent[node];
  }
}

// the moved triangles in the build's leaf order
__global__ void __launch_bounds__(256) refit_reorder(const float* __restrict__ tri, const int* __restrict__ order,
                                                      int n, float* __restrict__ out) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)n * kTriFloats) return;
  const int p = (int)(f / kTriFloats), q = (int)(f - (size_t)p * kTriFloats);
  const int o = order[p];
  if (o >= 0 && o < n) out[f] = tri[(size_t)o * kTriFloats + q];
}

// ---------------------------------------------------------------------------------------------------------------
// Posed objects (pose_tris, pose_raster): rest-pose records placed by one matrix per object, defined by
// tests/pose_ref.py. The table holds kPoseMatFloats per object: the glm column-major mat4, then the cofactor columns
// a0, a1, a2 of its upper 3x3 (computed once per object by the caller). Every float32 operation is spelled as the
// definition evaluates it (-ffp-contract=off); a record of no object, or of an object whose matrix is the identity,
// is copied bit for bit. The only index read from memory is the record's object, checked before it is used.

// the object of a record's objIndex among n_obj, or -1 (a NaN compares false throughout)
__device__ __forceinline__ int pose_object(float f, int n_obj) {
  return (f >= 0.0f && f < (float)n_obj && f == floorf(f)) ? (int)f : -1;
}

// all 16 floats compare == to the identity's (pts_transform_matrix's I)
__device__ __forceinline__ bool pose_identity(const float* __restrict__ m) {
  bool id = true;
#pragma unroll
  for (int j = 0; j < 16; ++j) id = id && m[j] == (j % 5 == 0 ? 1.0f : 0.0f);
  return id;
}

// glm mat4 * vec4(p, 1) (scene_prep.cpp xform_point): (m0 x + m1 y) + (m2 z + m3 1)
__device__ __forceinline__ glsl::v3 pose_point(const float* __restrict__ m, glsl::v3 p) {
  float r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mul0 = m[0 + k] * p.x, mul1 = m[4 + k] * p.y, mul2 = m[8 + k] * p.z, mul3 = m[12 + k] * 1.0f;
    const float add0 = mul0 + mul1, add1 = mul2 + mul3;
    r[k] = add0 + add1;
  }
  return glsl::mk(r[0], r[1], r[2]);
}

// normalize(cofactor matrix * n): the inverse transpose up to a scale of either sign; a = the 9 cofactor floats
__device__ __forceinline__ glsl::v3 pose_normal(const float* __restrict__ a, glsl::v3 n) {
  float v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = (a[0 + k] * n.x + a[3 + k] * n.y) + a[6 + k] * n.z;
  return glsl::normalize(glsl::mk(v[0], v[1], v[2]));
}

// One thread per 12-byte texel of a Triangle_encoded record (15 per record), so a wave loads and stores 768
// contiguous bytes: texels 0-2 are p1-p3, 3-5 n1-n3, the rest is copied; the object comes from texel 14 of the record.
__global__ void __launch_bounds__(256) pose_tris(const float* __restrict__ rest, int n, const float* __restrict__ mats,
                                                  int n_obj, float* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * 15) return;
  const size_t rec = t / 15;
  const int tex = (int)(t - rec * 15);
  glsl::v3 v = glsl::mk(rest[3 * t], rest[3 * t + 1], rest[3 * t + 2]);
  if (tex < 6) {
    const int k = pose_object(rest[rec * kTriFloats + 42], n_obj);
    if (k >= 0) {
      const float* m = mats + (size_t)k * kPoseMatFloats;
      if (!pose_identity(m)) v = tex < 3 ? pose_point(m, v) : pose_normal(m + 16, v);
    }
  }
  out[3 * t] = v.x;
  out[3 * t + 1] = v.y;
  out[3 * t + 2] = v.z;
}

// One thread per vertex of the raster list (pos3 + nrm3, 24 bytes); obj holds one int per triangle.
__global__ void __launch_bounds__(256) pose_raster(const float* __restrict__ rest, const int* __restrict__ obj,
                                                    int ntris, const float* __restrict__ mats, int n_obj,
                                                    float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)ntris * 3) return;
  const float* f = rest + 6 * i;
  glsl::v3 p = glsl::mk(f[0], f[1], f[2]), nv = glsl::mk(f[3], f[4], f[5]);
  const int k = obj[i / 3];
  if (k >= 0 && k < n_obj) {
    const float* m = mats + (size_t)k * kPoseMatFloats;
    if (!pose_identity(m)) {
      p = pose_point(m, p);
      nv = pose_normal(m + 16, nv);
    }
  }
  float* o = out + 6 * i;
  o[0] = p.x; o[1] = p.y; o[2] = p.z;
  o[3] = nv.x; o[4] = nv.y; o[5] = nv.z;
}

// ---------------------------------------------------------------------------------------------------------------
// Skinned objects (skin_tris, skin_raster): rest-pose corners placed by a blend of up to four bone matrices, defined
// by tests/skin_ref.py. A corner carries four bone indices (uint16, 8 bytes) and four weights (float, 16 bytes). The
// table holds kSkinBoneFloats per bone: three float4 rows (m[k], m[4+k], m[8+k], m[12+k]), k = 0..2, of the glm
// column-major mat4, so an influence is three 16-byte loads through the cache. Every float32 operation is spelled as
// the definition evaluates it; a corner whose four weights all compare == 0, or that names a bone >= n_bones (checked
// before the table is read), is copied bit for bit.

struct SkinBlend {
  float4 r[3];  // row k: M[k], M[4+k], M[8+k], M[12+k]
};

// the corner's influences; false: the corner is kept
__device__ __forceinline__ bool skin_influences(const uint16_t* __restrict__ bones, const float* __restrict__ weights,
                                                size_t corner, int n_bones, int b[4], float w[4]) {
  const float4 wv = *reinterpret_cast<const float4*>(weights + 4 * corner);
  w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
  if (w[0] == 0.0f && w[1] == 0.0f && w[2] == 0.0f && w[3] == 0.0f) return false;
  const uint2 bv = *reinterpret_cast<const uint2*>(bones + 4 * corner);
  b[0] = (int)(bv.x & 0xffffu); b[1] = (int)(bv.x >> 16);
  b[2] = (int)(bv.y & 0xffffu); b[3] = (int)(bv.y >> 16);
  return b[0] < n_bones && b[1] < n_bones && b[2] < n_bones && b[3] < n_bones;
}

// M[j] = ((w0 B0[j] + w1 B1[j]) + w2 B2[j]) + w3 B3[j]: all four terms, whatever the weights
__device__ __forceinline__ float skin_mix(const float w[4], float b0, float b1, float b2, float b3) {
  const float mul0 = w[0] * b0, mul1 = w[1] * b1, mul2 = w[2] * b2, mul3 = w[3] * b3;
  const float add0 = mul0 + mul1, add1 = add0 + mul2;
  return add1 + mul3;
}

__device__ __forceinline__ SkinBlend skin_blend(const float4* __restrict__ table, const int b[4], const float w[4]) {
  SkinBlend m;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float4 b0 = table[3 * b[0] + k], b1 = table[3 * b[1] + k], b2 = table[3 * b[2] + k],
                 b3 = table[3 * b[3] + k];
    m.r[k] = make_float4(skin_mix(w, b0.x, b1.x, b2.x, b3.x), skin_mix(w, b0.y, b1.y, b2.y, b3.y),
                         skin_mix(w, b0.z, b1.z, b2.z, b3.z), skin_mix(w, b0.w, b1.w, b2.w, b3.w));
  }
  return m;
}

// pose_point's expression with the blended matrix
__device__ __forceinline__ glsl::v3 skin_point(const SkinBlend& m, glsl::v3 p) {
  float r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mul0 = m.r[k].x * p.x, mul1 = m.r[k].y * p.y, mul2 = m.r[k].z * p.z, mul3 = m.r[k].w * 1.0f;
    const float add0 = mul0 + mul1, add1 = mul2 + mul3;
    r[k] = add0 + add1;
  }
  return glsl::mk(r[0], r[1], r[2]);
}

// pose_normal with the cofactor columns of the blended matrix, computed per corner
__device__ __forceinline__ glsl::v3 skin_normal(const SkinBlend& m, glsl::v3 n) {
  const glsl::v3 c0 = glsl::mk(m.r[0].x, m.r[1].x, m.r[2].x), c1 = glsl::mk(m.r[0].y, m.r[1].y, m.r[2].y),
                 c2 = glsl::mk(m.r[0].z, m.r[1].z, m.r[2].z);
  const glsl::v3 a0 = glsl::cross(c1, c2), a1 = glsl::cross(c2, c0), a2 = glsl::cross(c0, c1);
  const float a[9] = {a0.x, a0.y, a0.z, a1.x, a1.y, a1.z, a2.x, a2.y, a2.z};
  return pose_normal(a, n);
}

// pose_tris's mapping: one thread per 12-byte texel, 15 per record; texels 0-2 are p1-p3, 3-5 n1-n3, the rest is
// copied. A position or normal texel reads the influences of its corner (3 rec + tex % 3) and blends.
__global__ void __launch_bounds__(256) skin_tris(const float* __restrict__ rest, int n,
                                                  const uint16_t* __restrict__ bones,
                                                  const float* __restrict__ weights,
                                                  const float4* __restrict__ table, int n_bones,
                                                  float* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * 15) return;
  const size_t rec = t / 15;
  const int tex = (int)(t - rec * 15);
  glsl::v3 v = glsl::mk(rest[3 * t], rest[3 * t + 1], rest[3 * t + 2]);
  if (tex < 6) {
    int b[4];
    float w[4];
    if (skin_influences(bones, weights, rec * 3 + (size_t)(tex < 3 ? tex : tex - 3), n_bones, b, w)) {
      const SkinBlend m = skin_blend(table, b, w);
      v = tex < 3 ? skin_point(m, v) : skin_normal(m, v);
    }
  }
  out[3 * t] = v.x;
  out[3 * t + 1] = v.y;
  out[3 * t + 2] = v.z;
}

// pose_raster's mapping: one thread per vertex of the raster list (pos3 + nrm3), one blend for both.
__global__ void __launch_bounds__(256) skin_raster(const float* __restrict__ rest, int ntris,
                                                    const uint16_t* __restrict__ bones,
                                                    const float* __restrict__ weights,
                                                    const float4* __restrict__ table, int n_bones,
                                                    float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)ntris * 3) return;
  const float* f = rest + 6 * i;
  glsl::v3 p = glsl::mk(f[0], f[1], f[2]), nv = glsl::mk(f[3], f[4], f[5]);
  int b[4];
  float w[4];
  if (skin_influences(bones, weights, i, n_bones, b, w)) {
    const SkinBlend m = skin_blend(table, b, w);
    p = skin_point(m, p);
    nv = skin_normal(m, nv);
  }
  float* o = out + 6 * i;
  o[0] = p.x; o[1] = p.y; o[2] = p.z;
  o[3] = nv.x; o[4] = nv.y; o[5] = nv.z;
}

}  // namespace

int skin_tris_launch(const float* rest, int n, const uint16_t* bones, const float* weights, const float* table,
                     int n_bones, float* out, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(skin_tris, dim3((unsigned)(((size_t)n * 15 + 255) / 256)), dim3(256), 0, s, rest, n, bones,
                     weights, reinterpret_cast<const float4*>(table), n_bones, out);
  return (int)hipGetLastError();
}

int skin_raster_launch(const float* rest, int ntris, const uint16_t* bones, const float* weights, const float* table,
                       int n_bones, float* out, hipStream_t s) {
  if (ntris <= 0) return 0;
  hipLaunchKernelGGL(skin_raster, dim3((unsigned)(((size_t)ntris * 3 + 255) / 256)), dim3(256), 0, s, rest, ntris,
                     bones, weights, reinterpret_cast<const float4*>(table), n_bones, out);
  return (int)hipGetLastError();
}

int pose_tris_launch(const float* rest, int n, const float* mats, int n_obj, float* out, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(pose_tris, dim3((unsigned)(((size_t)n * 15 + 255) / 256)), dim3(256), 0, s, rest, n, mats, n_obj,
                     out);
  return (int)hipGetLastError();
}

int pose_raster_launch(const float* rest, const int* obj, int ntris, const float* mats, int n_obj, float* out,
                       hipStream_t s) {
  if (ntris <= 0) return 0;
  hipLaunchKernelGGL(pose_raster, dim3((unsigned)(((size_t)ntris * 3 + 255) / 256)), dim3(256), 0, s, rest, obj, ntris,
                     mats, n_obj, out);
  return (int)hipGetLastError();
}

int decode_raster(const float* verts, const int* order, int n, float4* geom, float4* nrm, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(decode_raster_kernel, dim3((n + 255) / 256), dim3(256), 0, s, verts, order, n, geom, nrm);
  return (int)hipGetLastError();
}

int raster_disp(const float4* geom, const float* prev, const float* cur, int n, float4* disp, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(raster_disp_kernel, dim3((n + 255) / 256), dim3(256), 0, s, geom, prev, cur, n, disp);
  return (int)hipGetLastError();
}

int decode_tris(const float* te, int n, float4* geom, float4* shade, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(decode_tris_kernel, dim3((n + 255) / 256), dim3(256), 0, s, te, n, geom, shade);
  return (int)hipGetLastError();
}

size_t LbvhWork::need(int n) {
  size_t b = 0;
  auto add = [&](size_t bytes) { b += (bytes + 255) & ~(size_t)255; };
  add(2 * sizeof(uint64_t) * n);            // keys in / out
  add(sizeof(float4) * n);                  // centroids
  add(sizeof(int2) * n);                    // child
  add(sizeof(int2) * n);                    // range
  add(sizeof(int) * 2 * n);                 // parent
  add(sizeof(float4) * 2 * 2 * n);          // boxes
  add(sizeof(int) * n);                     // flags
  add(sizeof(int) * 2 * n * 2);             // keep, id
  add(64);                                  // bounds + count
  // PLOC top: start, rank, nn, cluster ids x2 | leaf ranges | cluster boxes x2, leaf boxes, node boxes | flags,
  // scanned flags | node children | counters
  add(sizeof(int) * n * 5);
  add(sizeof(int2) * n);
  add(sizeof(float4) * 2 * n * 4);
  add(sizeof(uint64_t) * n * 2);
  add(sizeof(int2) * n);
  add(64);
  return b;
}

int lbvh_build(LbvhWork& w, const float* tri, TriLayout lay, int n, int leaf_n, int ploc_r, float* tri_out,
               float* node_out, int* order, int* nnodes, hipStream_t s) {
  if (n < 1) return (int)hipErrorInvalidValue;
  int ibits = 1;
  while ((1ll << ibits) < n) ++ibits;
  const size_t need = LbvhWork::need(n);
  // rocPRIM scratch: sort of 30 + ibits key bits, scan of 2n - 1 flags
  size_t sort_bytes = 0, scan_bytes = 0;
  hipError_t e = rocprim::radix_sort_keys(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)n, 0,
                                          30 + ibits, s);
  if (e != hipSuccess) return (int)e;
  e = rocprim::exclusive_scan(nullptr, scan_bytes, (int*)nullptr, (int*)nullptr, 0, (size_t)(2 * n - 1),
                              rocprim::plus<int>(), s);
  if (e != hipSuccess) return (int)e;
  size_t scan64_bytes = 0;
  e = rocprim::exclusive_scan(nullptr, scan64_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)n,
                              rocprim::plus<uint64_t>(), s);
  if (e != hipSuccess) return (int)e;
  const size_t temp = std::max(sort_bytes, std::max(scan_bytes, scan64_bytes));
  if (w.bytes < need + temp) {
    if (w.base) (void)hipFree(w.base);
    w.base = nullptr;
    w.bytes = 0;
    if ((e = hipMalloc(&w.base, need + temp)) != hipSuccess) return (int)e;
    w.bytes = need + temp;
  }
  char* p = (char*)w.base;
  auto take = [&](size_t bytes) { char* q = p; p += (bytes + 255) & ~(size_t)255; return (void*)q; };
  uint64_t* kin = (uint64_t*)take(sizeof(uint64_t) * n);
  uint64_t* kout = (uint64_t*)take(sizeof(uint64_t) * n);
  float4* cen = (float4*)take(sizeof(float4) * n);
  int2* child = (int2*)take(sizeof(int2) * n);
  int2* range = (int2*)take(sizeof(int2) * n);
  int* parent = (int*)take(sizeof(int) * 2 * n);
  float4* box = (float4*)take(sizeof(float4) * 2 * 2 * n);
  int* flags = (int*)take(sizeof(int) * n);
  int* keep = (int*)take(sizeof(int) * 2 * n);
  int* id = (int*)take(sizeof(int) * 2 * n);
  unsigned* bounds = (unsigned*)take(64);
  int* start = (int*)take(sizeof(int) * n * 5);
  int *rank = start + n, *nn = start + 2 * n, *C0 = start + 3 * n, *C1 = start + 4 * n;
  int2* leaf = (int2*)take(sizeof(int2) * n);
  float4* cb0 = (float4*)take(sizeof(float4) * 2 * n * 4);
  float4 *cb1 = cb0 + 2 * n, *leafbox = cb0 + 4 * n, *nbox = cb0 + 6 * n;
  uint64_t* f = (uint64_t*)take(sizeof(uint64_t) * n * 2);
  uint64_t* pf = f + n;
  int2* nchild = (int2*)take(sizeof(int2) * n);
  int* cnt = (int*)take(64);
  void* scratch = (void*)(p);
  // bounds: ordered min words start at 0xffffffff, max words at 0 (no host buffer involved)
  if ((e = hipMemsetAsync(bounds, 0xff, 3 * sizeof(unsigned), s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(bounds + 3, 0, 3 * sizeof(unsigned), s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(flags, 0, sizeof(int) * n, s)) != hipSuccess) return (int)e;
  const int gb = (n + 255) / 256, ge = (2 * n - 1 + 255) / 256;
  hipLaunchKernelGGL(lbvh_centroids, dim3(gb), dim3(256), 0, s, tri, n, lay, cen, bounds);
  hipLaunchKernelGGL(lbvh_keys, dim3(gb), dim3(256), 0, s, cen, n, bounds, ibits, kin);
  size_t sb = sort_bytes;
  if ((e = rocprim::radix_sort_keys(scratch, sb, kin, kout, (size_t)n, 0, 30 + ibits, s)) != hipSuccess) return (int)e;
  if (n > 1) hipLaunchKernelGGL(lbvh_karras, dim3((n - 1 + 255) / 256), dim3(256), 0, s, kout, n, child, range, parent);
  else if ((e = hipMemsetAsync(parent, 0xff, sizeof(int), s)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(lbvh_refit, dim3(gb), dim3(256), 0, s, tri, lay, kout, n, ibits, child, parent, box, flags, order);
  hipLaunchKernelGGL(lbvh_mark, dim3(ge), dim3(256), 0, s, n, leaf_n, range, parent, keep);
  size_t cb = scan_bytes;
  if ((e = rocprim::exclusive_scan(scratch, cb, keep, id, 0, (size_t)(2 * n - 1), rocprim::plus<int>(), s)) !=
      hipSuccess)
    return (int)e;
  if (ploc_r <= 0 || n == 1) {
    hipLaunchKernelGGL(lbvh_emit, dim3(ge), dim3(256), 0, s, n, leaf_n, child, range, keep, id, box, node_out);
  } else {
    if ((e = hipMemsetAsync(start, 0, sizeof(int) * n, s)) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(ploc_leafstart, dim3(ge), dim3(256), 0, s, n, leaf_n, range, keep, start);
    size_t rb = scan_bytes;
    if ((e = rocprim::exclusive_scan(scratch, rb, start, rank, 0, (size_t)n, rocprim::plus<int>(), s)) != hipSuccess)
      return (int)e;
    hipLaunchKernelGGL(ploc_init, dim3(ge), dim3(256), 0, s, n, leaf_n, range, keep, rank, start, box, leaf, leafbox, C0,
                       cb0, cnt);
    // iterations in batches; a converged array (one cluster) makes further iterations no-ops
    int host_cnt[5] = {0, 0, 0, 0, 0};
    bool converged = false;
    for (int it = 0; it < 4096 && !converged;) {
      for (int b = 0; b < 8; ++b, ++it) {
        int* cin = cnt + 2 * (it & 1);
        int* cout = cnt + 2 * ((it + 1) & 1);
        int* Ci = (it & 1) ? C1 : C0;
        int* Co = (it & 1) ? C0 : C1;
        float4* bi = (it & 1) ? cb1 : cb0;
        float4* bo = (it & 1) ? cb0 : cb1;
        hipLaunchKernelGGL(ploc_nn, dim3(gb), dim3(256), 0, s, cin, bi, ploc_r, nn);
        hipLaunchKernelGGL(ploc_flags, dim3(gb), dim3(256), 0, s, cin, nn, n, f);
        size_t fb = scan64_bytes;
        if ((e = rocprim::exclusive_scan(scratch, fb, f, pf, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), s)) !=
            hipSuccess)
          return (int)e;
        hipLaunchKernelGGL(ploc_compact, dim3(gb), dim3(256), 0, s, cin, cout, Ci, bi, nn, f, pf, Co, bo, nchild, nbox);
      }
      if ((e = hipMemcpyAsync(host_cnt, cnt, sizeof(host_cnt), hipMemcpyDeviceToHost, s)) != hipSuccess) return (int)e;
      if ((e = hipStreamSynchronize(s)) != hipSuccess) return (int)e;
      converged = host_cnt[2 * (it & 1)] <= 1;
    }
    if (converged) {
      hipLaunchKernelGGL(ploc_emit, dim3(gb), dim3(256), 0, s, cnt, n, nchild, nbox, leaf, leafbox, node_out);
      if (tri_out)
        hipLaunchKernelGGL(lbvh_reorder, dim3((unsigned)(((size_t)n * kTriFloats + 255) / 256)), dim3(256), 0, s, tri,
                           kout, n, ibits, tri_out);
      if ((e = hipStreamSynchronize(s)) != hipSuccess) return (int)e;
      *nnodes = 2 * host_cnt[4];  // dummy + (M - 1) PLOC nodes + M leaves
      return (int)hipGetLastError();
    }
    // past the iteration cap (every iteration merges at least one pair, and runs of equal areas halve, so only a
    // pathological input gets here): the plain LBVH top over the same leaves, whose buffers PLOC left untouched
    hipLaunchKernelGGL(lbvh_emit, dim3(ge), dim3(256), 0, s, n, leaf_n, child, range, keep, id, box, node_out);
  }
  if (tri_out)
    hipLaunchKernelGGL(lbvh_reorder, dim3((unsigned)(((size_t)n * kTriFloats + 255) / 256)), dim3(256), 0, s, tri,
                       kout, n, ibits, tri_out);
  // output node count = 1 (dummy) + id[last] + keep[last]
  int tail[2];
  if ((e = hipMemcpyAsync(&tail[0], id + 2 * n - 2, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(&tail[1], keep + 2 * n - 2, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return (int)e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return (int)e;
  *nnodes = 1 + tail[0] + tail[1];
  return (int)hipGetLastError();
}

void lbvh_trees_free(LbvhTrees& t) {
  if (t.base) (void)hipFree(t.base);
  if (t.e0) (void)hipEventDestroy(t.e0);
  if (t.e1) (void)hipEventDestroy(t.e1);
  t = LbvhTrees{};
}

int lbvh_trees_launch(LbvhWork& w, const float* nodes, int nnodes, LbvhTrees& out, hipStream_t s,
                      const int* refit_err) {
  if (nnodes < 2 || out.base) return (int)hipErrorInvalidValue;
  const size_t nn = (size_t)nnodes;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  hipError_t e;
  size_t scan_bytes = 0;
  e = rocprim::exclusive_scan(nullptr, scan_bytes, (int*)nullptr, (int*)nullptr, 0, nn, rocprim::plus<int>(), s);
  if (e != hipSuccess) return (int)e;
  // parent, flags, leaf, leafpos, idx | child lists | sizes | info | scan scratch
  const size_t need = 5 * up(sizeof(int) * nn) + up(sizeof(int4) * nn) + up(sizeof(int2) * nn) + 256 + up(scan_bytes);
  if (w.bytes < need) {  // the build that wrote `nodes` has synchronised: its scratch is free
    if (w.base) (void)hipFree(w.base);
    w.base = nullptr;
    w.bytes = 0;
    if ((e = hipMalloc(&w.base, need)) != hipSuccess) return (int)e;
    w.bytes = need;
  }
  // a full binary tree of nn - 1 nodes has (nn - 2) / 2 interior nodes; every record written is checked against
  // its part's room anyway (error bit 2)
  out.cap_bin = out.cap_wide = std::max(1, nnodes / 2);
  out.cap_leaves = nnodes;
  const size_t b_bin = up(sizeof(float4) * 4 * out.cap_bin), b_leaves = up(sizeof(float4) * 2 * out.cap_leaves),
               b_wide = up(sizeof(float4) * kWideStride * out.cap_wide);
  if ((e = hipMalloc(&out.base, b_bin + b_leaves + b_wide)) != hipSuccess) {
    out.base = nullptr;
    return (int)e;
  }
  out.bin = (float4*)out.base;
  out.leaves = (float4*)((char*)out.base + b_bin);
  out.wide = (float4*)((char*)out.base + b_bin + b_leaves);
  char* p = (char*)w.base;
  auto take = [&](size_t bytes) { char* q = p; p += up(bytes); return (void*)q; };
  int* parent = (int*)take(sizeof(int) * nn);
  int* flags = (int*)take(sizeof(int) * nn);
  int* leaf = (int*)take(sizeof(int) * nn);
  int* leafpos = (int*)take(sizeof(int) * nn);
  int* idx = (int*)take(sizeof(int) * nn);
  int4* ch = (int4*)take(sizeof(int4) * nn);
  int2* sz = (int2*)take(sizeof(int2) * nn);
  int* info = (int*)take(256);
  void* scratch = (void*)p;
  if (hipEventCreate(&out.e0) != hipSuccess || hipEventCreate(&out.e1) != hipSuccess) return (int)hipErrorUnknown;
  (void)hipEventRecord(out.e0, s);
  // parent and flags are adjacent: parent = -1 (no parent), flags = 0; an empty tree's parts read as one zero record
  if ((e = hipMemsetAsync(parent, 0xff, sizeof(int) * nn, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(flags, 0, sizeof(int) * nn, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(info, 0, 256, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(out.bin, 0, sizeof(float4) * 4, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(out.leaves, 0, sizeof(float4) * 2, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(out.wide, 0, sizeof(float4) * kWideStride, s)) != hipSuccess) return (int)e;
  const dim3 grid((unsigned)((nn + 255) / 256)), block(256);
  hipLaunchKernelGGL(trees_local, grid, block, 0, s, nodes, nnodes, parent, ch, sz, leaf, info, refit_err);
  size_t sb = scan_bytes;
  if ((e = rocprim::exclusive_scan(scratch, sb, leaf, leafpos, 0, nn, rocprim::plus<int>(), s)) != hipSuccess)
    return (int)e;
  hipLaunchKernelGGL(trees_sizes, grid, block, 0, s, nodes, nnodes, parent, ch, leaf, sz, flags);
  hipLaunchKernelGGL(trees_index, grid, block, 0, s, nodes, nnodes, parent, leaf, sz, idx, info);
  hipLaunchKernelGGL(trees_emit, grid, block, 0, s, nodes, nnodes, ch, leaf, leafpos, sz, idx, out.bin, out.cap_bin,
                     out.leaves, out.cap_leaves, out.wide, out.cap_wide, info);
  (void)hipEventRecord(out.e1, s);
  static_assert(sizeof(out.dev_info) == kInfoInts * sizeof(int), "dev_info holds the stage's counters");
  if ((e = hipMemcpyAsync(out.dev_info, info, sizeof(out.dev_info), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return (int)e;
  return (int)hipGetLastError();
}

int lbvh_refit_alloc(LbvhRefit& r, int n) {
  if (n < 1) return (int)hipErrorInvalidValue;
  if (r.base && r.n == n) return 0;
  lbvh_refit_free(r);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_order = up(sizeof(int) * (size_t)n), b_nodes = up(sizeof(int) * 2 * (size_t)n);
  const hipError_t e = hipMalloc(&r.base, b_order + 2 * b_nodes + 256);
  if (e != hipSuccess) {
    r.base = nullptr;
    return (int)e;
  }
  r.order = (int*)r.base;
  r.parent = (int*)((char*)r.base + b_order);
  r.flags = (int*)((char*)r.base + b_order + b_nodes);
  r.err = (int*)((char*)r.base + b_order + 2 * b_nodes);
  r.n = n;
  r.nnodes = 0;
  return 0;
}

void lbvh_refit_free(LbvhRefit& r) {
  if (r.base) (void)hipFree(r.base);
  r = LbvhRefit{};
}

int lbvh_refit_link(LbvhRefit& r, const float* nodes, int nnodes, hipStream_t s) {
  if (!r.base || nnodes < 2 || nnodes > 2 * r.n) return (int)hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(r.parent, 0xff, sizeof(int) * (size_t)nnodes, s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(r.err, 0, sizeof(int), s)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(refit_link, dim3((nnodes + 255) / 256), dim3(256), 0, s, nodes, nnodes, r.parent, r.err);
  r.nnodes = nnodes;
  return (int)hipGetLastError();
}

int lbvh_refit_nodes(LbvhRefit& r, float* nodes, const float* tri, TriLayout lay, hipStream_t s) {
  if (!r.base || r.nnodes < 2 || r.nnodes > 2 * r.n) return (int)hipErrorInvalidValue;
  // flags start at 0 for every refit; err keeps what lbvh_refit_link found (a tree with a bad link is not climbed
  // into a fault, every index is checked again, but it stays reported)
  const hipError_t e = hipMemsetAsync(r.flags, 0, sizeof(int) * (size_t)r.nnodes, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(refit_nodes, dim3((r.nnodes + 255) / 256), dim3(256), 0, s, nodes, r.nnodes, tri, r.n, lay,
                     r.order, r.parent, r.flags, r.err);
  return (int)hipGetLastError();
}

int lbvh_refit_reorder(const LbvhRefit& r, const float* tri, float* tri_out, hipStream_t s) {
  if (!r.base) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(refit_reorder, dim3((unsigned)(((size_t)r.n * kTriFloats + 255) / 256)), dim3(256), 0, s, tri,
                     r.order, r.n, tri_out);
  return (int)hipGetLastError();
}

int lbvh_trees_finish(LbvhTrees& t) {
  if (!t.base || !t.e0 || !t.e1) return (int)hipErrorInvalidValue;
  hipError_t e = hipEventSynchronize(t.e1);  // long complete: the caller has synchronised the stream
  if (e == hipSuccess) e = hipEventElapsedTime(&t.stage_ms, t.e0, t.e1);
  (void)hipEventDestroy(t.e0);
  (void)hipEventDestroy(t.e1);
  t.e0 = t.e1 = nullptr;
  if (e != hipSuccess) return (int)e;
  if (t.dev_info[kInfoErr] || t.nbin() > t.cap_bin || t.nwide() > t.cap_wide || t.nleaves() > t.cap_leaves)
    return (int)hipErrorInvalidValue;
  return 0;
}

}  // namespace ptk

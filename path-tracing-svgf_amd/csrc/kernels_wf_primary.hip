// kernels_wf_primary.hip — the wavefront path tracer's primary stage (kernels_wavefront.hip has the schedule): the
// camera rays' closest hits, by the per-pixel walk (wf_primary), by reference leaves binned to screen tiles
// (wf_primary_raster) or by the triangles themselves binned (wf_primary_tri). The pixels a rasteriser leaves to a walk
// go to wf_primary_coop (kernels_wf_trace.hip) or back to wf_primary.
#include <hip/hip_runtime.h>

#include "glsl_builtins.h"
#include "pt_device.h"
#include "pt_shading.h"
#include "wf_common.h"

using namespace glsl;

namespace ptk {

// ------------------------------------------------------------ primaries ---
constexpr int kTieFix = -2;  // hit.x of a pixel wf_primary_raster leaves to the walk (two triangles share its t)

// 16x16 screen tiles, each wave an 8x8 sub-tile: coherent camera rays.
// nslots: the subset's tiles; a block walks slots blockIdx.x, + gridDim.x, ... (launched with one slot per block)
template <int KS, bool DEEP>
__global__ void __launch_bounds__(256) PT_TRACE_ATTR wf_primary(PTParams p, int nslots) {
  __shared__ int stk[KS * 256];
  for (int slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const int tile = sched_tile(p.tiles, slot);  // cost-ordered dispatch (subset slot)
  const int gt = tile * p.tile_stride + p.tile_offset, ntx = (p.W + 15) / 16;
  const int tx = gt % ntx, ty = gt / ntx;
  const int x = tx * 16 + (wv & 1) * 8 + (ln & 7);
  const int y = p.y0 + ty * 16 + (wv >> 1) * 8 + (ln >> 3);
  bool valid = x < p.W && y < p.y1;
  const int pid = (y - p.y0) * p.W + x;
  bool count_ray = true;
  if (p.pr_fix) {  // after wf_primary_raster: walk only the pixels it flagged, or all of them after an overflow
    if (p.pr_fix[2]) {
      // the skipped scatter did not count the tiles back to zero: the block of subset slot `tile` clears the tiles of
      // its stride group (the last slot also the band's tail), so every band tile is cleared once
      if (threadIdx.x == 0) {
        const int all = ntx * ((p.y1 - p.y0 + 15) / 16), lo = tile * p.tile_stride;
        const int hi = tile + 1 == nslots ? all : min(all, lo + p.tile_stride);
        for (int j = lo; j < hi; ++j) p.leaf_bins.tile_count[j] = 0;
      }
    } else {
      if (p.closest_tree) return;  // the flagged pixels went to wf_primary_coop
      valid = valid && ldnt(&p.wf.hit[pid]).x == kTieFix;
      if (!__any(valid)) continue;
      count_ray = false;  // counted by the rasteriser
    }
  }
  uint32_t steps = 0;
  bool rewalk = false, retry = false, spill = false;
  if (valid) {
    v3 S = mk(p.eye[0], p.eye[1], p.eye[2]);
    v3 d = primary_dir(p, x, y);
    // Bound from the G-buffer: the surface this pixel rasterised lies at distance |P - eye|; the walk first seeks
    // only hits nearer than that (plus a margin). The closest hit, if it is nearer, lies in boxes the pruned walk
    // still visits in the reference's order (ties included), so the result is the unbounded walk's; when no hit
    // is found below the bound (a different ray, a grazing or culled surface) the walk is repeated unbounded.
    float bound = PT_INF;
    if (p.hint_pos.p && p.prune) {
      const float4 nd = pld(p.hint_nd, x, y);
      if (nd.w != 1.0f) {  // not background (zCenter == 1)
        const float4 P = pld(p.hint_pos, x, y);
        const float dist = length(sub(xyz(P), S));
        if (dist == dist) bound = dist * 1.001f + 1.0e-3f;
      }
    }
    float t;
    auto st = ray_stack<256, KS, DEEP>(stk + threadIdx.x, p, pid);
    int tri = closest_hit(p.scene, p.closest_tree, st, S, d, p.prune, &t, &steps, bound, &rewalk);
    if (tri < 0 && bound < PT_INF) {
      uint32_t more = 0;
      bool rw2 = false;
      tri = closest_hit(p.scene, p.closest_tree, st, S, d, p.prune, &t, &more, PT_INF, &rw2);
      steps += more;
      retry = true;
      rewalk = rewalk || rw2;
    }
    stnt(&p.wf.hit[pid], make_int2(tri, __float_as_int(t)));
    spill = st.spilled;
  }
  stat_add(p, kStatPrimRays, valid && count_ray ? 1u : 0u);
  stat_add(p, kStatPrimVisits, steps);
  stat_slots(p, kStatPrimSlots, steps);
  stat_add(p, kStatTieRewalks, rewalk ? 1u : 0u);
  stat_add(p, kStatPrimRetries, retry ? 1u : 0u);
  stat_add(p, kStatSpills, spill ? 1u : 0u);
  sched_cost(p.tiles, tile, steps);
  if (valid) add_row_cost(p, y - p.y0, pid, steps);
  }
}

// ------------------------------------------------ primaries by tile binning ---
// The primary rays' closest hits without a per-pixel BVH walk. The candidates of hitBVH for a ray are the
// triangles of the reference leaves whose own box the ray passes (hitAABB > 0: every reference ancestor box holds
// that box, so the walk reaches it — closest_hit's argument, pt_shading.h), the closest hit is the minimum t over
// them, and when one triangle alone attains it, that triangle. So each reference leaf is binned to the 16 x 16
// tiles whose pixels' primary rays can pass its box, and each pixel runs, over its tile's leaves, the walk's own
// leaf step: hitAABB on the leaf box with the walk's pruning bound, then hitTriangle on the leaf's triangles in
// order, seeking (as wf_primary) only hits nearer than this frame's G-buffer surface. A pixel whose minimum t two
// triangles share (the reference keeps the one its depth-first order meets first) or that finds nothing below the
// G-buffer bound is flagged and walked by wf_primary, as is every pixel if a list overflows. Same bits as wf_primary.
constexpr int kPChunk = 256;  // leaves staged in LDS per round
// per reference leaf: the pixel box of the primary rays that can pass its box — each face clipped to the widened
// frustum and projected; a box holding the eye covers the band — and the nearest t they can meet it at (t along
// the normalised ray is at least the camera-space depth w of the point)
__global__ void __launch_bounds__(256) pr_setup(PTParams p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.scene.nleaves) return;
  const float4 lo4 = p.scene.leaves[2 * i], hi4 = p.scene.leaves[2 * i + 1];
  const float lo[3] = {lo4.x, lo4.y, lo4.z}, hi[3] = {hi4.x, hi4.y, hi4.z};
  const float* m = p.camRot;  // primary_dir: right = m[0..2], up = m[4..6], back = m[8..10]
  const float sx = p.aspect_corrected ? (float)p.W / (float)p.H : 1.0f;
  int4 box = make_int4(0, p.y0, p.W - 1, p.y1 - 1);
  float tmin = 0.0f;
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float e = p.eye[a], tol = 1.0e-4f * (fabsf(e) + 1.0f);
    inside = inside && e >= lo[a] - tol && e <= hi[a] + tol;
  }
  if (!inside) {
    float3 C[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float X = (k & 1 ? hi[0] : lo[0]) - p.eye[0], Y = (k & 2 ? hi[1] : lo[1]) - p.eye[1],
                  Z = (k & 4 ? hi[2] : lo[2]) - p.eye[2];
      const float cx = (m[0] * X + m[1] * Y) + m[2] * Z, cy = (m[4] * X + m[5] * Y) + m[6] * Z,
                  cz = (m[8] * X + m[9] * Y) + m[10] * Z;
      C[k] = make_float3(cx / sx, cy, -cz);
    }
    // every corner inside the widened frustum (poly_box's clip planes) and in front: no clipping happens, and the
    // box's projection is the hull of its corners' projections (all w > 0)
    bool front = true;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      front = front && C[k].z > 0.0f && fabsf(C[k].x) <= 1.01f * C[k].z && fabsf(C[k].y) <= 1.01f * C[k].z;
    constexpr int F[6][4] = {{0, 2, 6, 4}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 3, 7, 6}, {0, 1, 3, 2}, {4, 5, 7, 6}};
    int4 u = make_int4(1, 1, 0, 0);
    float w = 3.0e38f;
    bool any = false;
    if (front) {  // nothing to clip: the box of the corners' projections (poly_box's arithmetic, unrolled)
      float x0 = 3.0e38f, y0 = 3.0e38f, x1 = -3.0e38f, y1 = -3.0e38f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float px = ((C[k].x / C[k].z + 1.0f) * (float)p.W - 1.0f) * 0.5f;
        const float py = ((C[k].y / C[k].z + 1.0f) * (float)p.H - 1.0f) * 0.5f;
        x0 = fminf(x0, px); x1 = fmaxf(x1, px);
        y0 = fminf(y0, py); y1 = fmaxf(y1, py);
        w = fminf(w, C[k].z);
      }
      u = pixel_box(p.leaf_bins, x0, y0, x1, y1);
      any = !(u.x > u.z || u.y > u.w);
    }
#pragma unroll
    for (int f = 0; f < 6; ++f) {  // (unrolled: the corner indices stay compile-time, C in registers)
      if (front) break;
      float3 A[16];
#pragma unroll
      for (int k = 0; k < 4; ++k) A[k] = C[F[f][k]];
      int4 fb;
      float ft;
      if (!poly_box(p.leaf_bins, p.H, A, 4, 1.0f, 1.0f, &fb, &ft)) continue;
      if (fb.x > fb.z || fb.y > fb.w) continue;
      u = any ? make_int4(min(u.x, fb.x), min(u.y, fb.y), max(u.z, fb.z), max(u.w, fb.w)) : fb;
      w = fminf(w, ft);
      any = true;
    }
    box = any ? u : make_int4(1, 1, 0, 0);
    tmin = any ? w * 0.9999f : 0.0f;
  }
  bins_count_item(p.leaf_bins, i, box, tmin);
}

// The G-buffer bound of wf_primary for a rasterised pixel: only hits nearer than the rasterised surface (plus a
// margin) are sought; a pixel that finds none below it is flagged for the walk (which retries unbounded).
__device__ __forceinline__ float raster_bound(const PTParams& p, bool valid, int x, int y, v3 S) {
  float bound = PT_INF;
  if (valid && p.hint_pos.aux && p.prune) {
    // the G-buffer pass formed this float from the same texels and this eye with the statements below (gb_finish;
    // pt_params binds the plane only for that eye): 4 bytes per pixel instead of two float4 texels. +inf: none
    const float b = p.hint_pos.aux[(size_t)prow(p.hint_pos, y) * p.hint_pos.W + x];
    if (b != __builtin_inff()) bound = b;
  } else if (valid && p.hint_pos.p && p.prune) {
    const float4 nd = pld(p.hint_nd, x, y);
    if (nd.w != 1.0f) {
      const float dist = length(sub(xyz(pld(p.hint_pos, x, y)), S));
      if (dist == dist) bound = dist * 1.001f + 1.0e-3f;
    }
  }
  return bound;
}
// A rasterised pixel's result: its hit, or the flag that leaves it to the walk (`walk`; with the SAH tree on it is
// queued for wf_primary_coop), and the counters. Every lane of the block calls it.
__device__ __forceinline__ void raster_finish(const PTParams& p, bool valid, bool walk, int pid, int best, float tbest,
                                              uint32_t steps, int tile, int y) {
  const int ln = threadIdx.x & 63;
  if (valid) stnt(&p.wf.hit[pid], walk ? make_int2(kTieFix, 0) : make_int2(best, __float_as_int(tbest)));
  if (p.closest_tree) {  // flagged pixels: the wave-cooperative closest-hit walk (wf_primary_coop)
    const unsigned long long m = __ballot(walk);
    if (m) {
      int base = 0;
      if (ln == __ffsll((long long)m) - 1) base = atomicAdd(p.wf.counters + kCtrStragC, __popcll(m));
      base = __shfl(base, __ffsll((long long)m) - 1);
      if (walk) p.wf.strag_c[base + __popcll(m & ((1ull << ln) - 1ull))] = pid;
    }
  }
  stat_add(p, kStatPrimRays, valid ? 1u : 0u);
  stat_add(p, kStatPrimVisits, steps);
  stat_slots(p, kStatPrimSlots, steps);
  sched_cost(p.tiles, tile, steps);
  if (valid) add_row_cost(p, y - p.y0, pid, steps);
}

#ifndef PT_RASTER_WAVES
// waves/SIMD wf_primary_raster is compiled for (0: the compiler's choice, 67 VGPRs = 7 waves). 8 (64 VGPRs, no spill)
// measured the same (kernel trace, one frame at a time: 916.6 / 921.3 us, surface view 666.3 / 658.9; with PT_SHADE_WAVES
// 6 as well the frame rate fell 0.5 %: profiles/r05/occupancy_r8/)
#define PT_RASTER_WAVES 0
#endif
#if PT_RASTER_WAVES > 0
#define PT_RASTER_ATTR __attribute__((amdgpu_waves_per_eu(PT_RASTER_WAVES)))
#else
#define PT_RASTER_ATTR
#endif
__global__ void __launch_bounds__(256) PT_RASTER_ATTR wf_primary_raster(PTParams p) {
  __shared__ float4 slo[kPChunk], shi[kPChunk];
  __shared__ int4 sbox[kPChunk];
  __shared__ float stmin[kPChunk];
  __shared__ short wlist[4][kPChunk];  // per wave: the chunk's leaves that can meet its pixels
  const Bins& bn = p.leaf_bins;
  if (bn.ctr[2]) return;  // overflow: wf_primary walks every pixel
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  // subset slot -> band tile (PTParams::tile_stride: a pass may trace every tile_stride-th tile; the bins cover all)
  const int tile = blockIdx.x, gt = tile * p.tile_stride + p.tile_offset, ntx = (p.W + 15) / 16;
  const int x = (gt % ntx) * 16 + (wv & 1) * 8 + (ln & 7);
  const int y = p.y0 + (gt / ntx) * 16 + (wv >> 1) * 8 + (ln >> 3);
  const bool valid = x < p.W && y < p.y1;
  const int pid = (y - p.y0) * p.W + x;
  const v3 S = mk(p.eye[0], p.eye[1], p.eye[2]);
  const v3 d = primary_dir(p, x, y);
  const v3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
  const float bound = raster_bound(p, valid, x, y, S);
  float tbest = bound;
  int best = -1;
  bool tied = false;
  uint32_t steps = 0;
  // The tile's loosest pruning bound: a pixel's bound (tbest) only falls, so a leaf entered beyond the largest bound of
  // the tile's pixels, with a wider margin than the walk's (below), is skipped by every pixel — it is left out of the
  // staged chunk. Surface tiles drop the leaves hidden behind their surfaces; a tile with a background pixel keeps all.
  __shared__ float wmax[4];
  __shared__ int wcount[4];
  float tb = valid ? bound : 0.0f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tb = fmaxf(tb, __shfl_xor(tb, o));
  if (ln == 0) wmax[wv] = tb;
  __syncthreads();
  const float tile_lim = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])) * 1.0004f + 4.0e-4f;
  const int off = bn.tile_off[gt], total = bn.tile_off[gt + 1] - off;
  for (int base = 0; base < total; base += kPChunk) {
    __syncthreads();
    const int j = base + (int)threadIdx.x;
    int leaf = 0;
    float tm = 0.0f;
    if (j < total) {
      leaf = bn.pairs[off + j];
      tm = bn.tmin[leaf];
    }
    const bool keep = j < total && !(tm > tile_lim);
    const unsigned long long km = __ballot(keep);
    if (ln == 0) wcount[wv] = __popcll(km);
    __syncthreads();
    int n = 0, slot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      slot += w < wv ? wcount[w] : 0;
      n += wcount[w];
    }
    if (keep) {  // compacted in thread order
      slot += __popcll(km & ((1ull << ln) - 1ull));
      slo[slot] = p.scene.leaves[2 * leaf];
      shi[slot] = p.scene.leaves[2 * leaf + 1];
      sbox[slot] = bn.box[leaf];
      stmin[slot] = tm;
    }
    __syncthreads();
    // this wave's share of the chunk: the staged leaves whose pixel box meets the wave's 8 x 8 pixels and that are not
    // entered beyond the loosest of its pixels' pruning bounds, in chunk order (the closest t, a unique closest
    // triangle and an exact tie met do not depend on the order the candidates are tested in); each lane then steps
    // through that list instead of the whole chunk
    float wl = valid ? tbest * 1.0002f + 2.0e-4f : 0.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wl = fmaxf(wl, __shfl_xor(wl, o));
    const int wx0 = x - (ln & 7), wy0 = y - (ln >> 3);
    int wn = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
      const int k = k0 + ln;
      bool ov = false;
      if (k < n) {
        const int4 b = sbox[k];
        ov = !(b.z < wx0 || b.x > wx0 + 7 || b.w < wy0 || b.y > wy0 + 7) && !(stmin[k] > wl);
      }
      const unsigned long long m = __ballot(ov);
      if (ov) wlist[wv][wn + __popcll(m & ((1ull << ln) - 1ull))] = (short)k;
      wn += __popcll(m);
    }
    __syncthreads();
    if (!valid) continue;
    for (int i = 0; i < wn; ++i) {
      const int k = wlist[wv][i];
      const int4 b = sbox[k];
      if (x < b.x || x > b.z || y < b.y || y > b.w) continue;  // no primary ray of this pixel passes the box
      const float lim = tbest * 1.0002f + 2.0e-4f;                // the walk's pruning bound (traverse<0>)
      if (stmin[k] > lim) continue;                               // entered beyond it
      const float4 lo = slo[k], hi = shi[k];
      float t0;
      const float dl = slab(S, inv, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, &t0);
      ++steps;
      if (!(dl > 0.0f) || t0 > lim) continue;
      const int ref = __float_as_int(lo.w), first = ref_leaf_first(ref), cnt = ref_leaf_count(ref);
      steps += (uint32_t)cnt;
      leaf_scan(p.scene.tri_geom, first, cnt, S, d, [&](int i, float t) {
        if (t < tbest) { tbest = t; best = i; tied = false; }
        else if (t == tbest && best >= 0) tied = true;
        return false;
      });
    }
  }
  const bool walk = valid && (tied || (best < 0 && bound < PT_INF));  // a tie, or nothing below the G-buffer bound
  raster_finish(p, valid, walk, pid, best, tbest, steps, tile, y);
}

// --------------------------------------------- primaries by binned triangles ---
// The same closest hits with the triangles themselves binned to the tiles (primary_raster = 2). The reference tests a
// triangle for a ray exactly when the ray passes the box of the triangle's leaf (above), so a pixel runs hitTriangle
// on the triangles whose screen box holds it and asks for the leaf box (through SceneDev::tri_leaf) only for a
// triangle that was hit at t <= the best so far: the closest t, a unique closest triangle and an exact tie met are
// those of the leaf rasteriser. A background pixel then tests the few triangles whose own box holds it instead of
// every triangle of every leaf whose (far larger) projected box does.
//
// Screen box (pr_tri_setup). hitTriangle accepts the ray when the point P = S + d t', t' the computed plane
// parameter, lies on one side of the three planes through an edge and N. With N perpendicular to the edges (checked:
// 1e-3) that is the prism over the triangle along N, blurred by the rounding of the three edge terms (about 12 eps M
// in distance, M the coordinate magnitude of the vertices and the eye); P lies on the pixel's ray up to its own
// rounding (a few eps M); and t' puts P within |dt N.d| of the plane N.x = N.p1, where the error dt of t' has the
// factor 1 / |N.d| that the product removes again: about 4 eps M + 3 eps t', however grazing the ray. The vertices
// themselves lie within `dev` of that plane (measured per triangle: a sliver's computed N need not be its normal). So
// P is within e = 3e-5 M + 2 dev of a point of the triangle (a generous bound of the sum, tripled for the slope of
// the projection), and the ray's pixel within e / w * max(W, H) / 2 pixels of the triangle's projection, w the
// smallest depth of the clipped triangle: the box is widened by that, rounded to whole pixels (what the rounding
// drops, under 0.75 of a pixel, kTriMargin covers), and a triangle with e >= 0.005 w, a vertex on the camera plane, a non-finite vertex or an N that is not
// perpendicular gets the whole band. A triangle with a non-finite N is dropped: its dn or t is NaN, or t is 0, and
// hitTriangle rejects every ray.
// Depth bound. t' = |P - S| up to rounding, and P is within e' = 8e-6 M + 2 dev of a triangle point, whose distance
// from the eye is at least its depth >= w; so t' >= w - e' - 3 eps w. The pruning test skips a triangle whose bound
// exceeds tbest * 1.0002 + 2e-4, and a triangle matters only with t' <= tbest: the bound 0.9999 w is safe when
// e' < 2e-4 w, and a triangle that does not meet this (near the eye against the scene's size; grazing does not
// enter) gets the bound 0 and is never depth-culled.
// pixels around a triangle's projected box: with the hit test's slack carried per triangle (`extra` below leaves at
// most 0.75 of a pixel of it), the rest is the rounding of the projection and of primary_dir's pixel coordinate,
// about 3 W eps pixels each (1.4e-3 at 4K; pr_tri_setup's 16-bit boxes bound W)
constexpr int kTriMargin = 1;
constexpr int kTChunk = 224;  // triangles staged per round: 18.4 KiB of LDS per block, 8 blocks (8 waves / SIMD) per CU

__global__ void __launch_bounds__(256) tri_leaf_map_kernel(const float4* __restrict__ leaves, int nleaves,
                                                           int* __restrict__ map, int ntris) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nleaves) return;
  const int ref = __float_as_int(leaves[2 * i].w);
  if (ref >= 0) return;  // a zeroed record, not a leaf ref
  const int first = ref_leaf_first(ref), cnt = ref_leaf_count(ref);
  for (int k = first; k < first + cnt; ++k)
    if (k >= 0 && k < ntris) map[k] = i;
}
int launch_tri_leaf_map(const float4* leaves, int nleaves, int* tri_leaf, int ntris, hipStream_t s) {
  if (ntris <= 0) return 0;
  hipError_t e = hipMemsetAsync(tri_leaf, 0xff, (size_t)ntris * sizeof(int), s);  // -1: in no leaf
  if (e != hipSuccess) return (int)e;
  if (nleaves > 0 && leaves)
    hipLaunchKernelGGL(tri_leaf_map_kernel, dim3((nleaves + 255) / 256), dim3(256), 0, s, leaves, nleaves, tri_leaf, ntris);
  return (int)hipGetLastError();
}

// per triangle: screen box and depth bound (above), binning counts. Both facings: hitTriangle does not cull.
__global__ void __launch_bounds__(256) pr_tri_setup(PTParams p) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.leaf_bins.n) return;
  const int4 band = make_int4(0, p.y0, p.W - 1, p.y1 - 1);
  int4 box = make_int4(1, 1, 0, 0);  // empty
  float tmin = 0.0f;
  const TriGeom tg = tri_load(p.scene.tri_geom, i);
  const v3 N = xyz(tg.n), v[3] = {xyz(tg.a), xyz(tg.b), xyz(tg.c)};
  const float big = 3.0e38f;
  const bool nfin = fabsf(N.x) <= big && fabsf(N.y) <= big && fabsf(N.z) <= big;  // (false for NaN too)
  if (p.scene.tri_leaf[i] >= 0 && nfin) {  // (a triangle in no leaf is never tested by the reference)
    box = band;
    const float* m = p.camRot;  // primary_dir: right = m[0..2], up = m[4..6], back = m[8..10]
    const float sx = p.aspect_corrected ? (float)p.W / (float)p.H : 1.0f;
    float3 A[16];
    float M = 0.0f;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float mag = fmaxf(fabsf(v[k].x), fmaxf(fabsf(v[k].y), fabsf(v[k].z)));
      fin = fin && mag <= big;
      M = fmaxf(M, mag);
      const float X = v[k].x - p.eye[0], Y = v[k].y - p.eye[1], Z = v[k].z - p.eye[2];
      const float cx = (m[0] * X + m[1] * Y) + m[2] * Z, cy = (m[4] * X + m[5] * Y) + m[6] * Z,
                  cz = (m[8] * X + m[9] * Y) + m[10] * Z;
      A[k] = make_float3(cx / sx, cy, -cz);
    }
    M += fmaxf(fabsf(p.eye[0]), fmaxf(fabsf(p.eye[1]), fabsf(p.eye[2])));
    const v3 E[3] = {sub(v[1], v[0]), sub(v[2], v[1]), sub(v[0], v[2])};
    bool perp = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) perp = perp && fabsf(dot(N, E[k])) <= 1.0e-3f * length(E[k]);
    const float dev = fmaxf(fabsf(dot(N, E[0])), fabsf(dot(N, E[2])));  // the vertices' distance from N.x = N.p1
    int4 b;
    float w;
    if (fin && perp) {
      if (!poly_box(p.leaf_bins, p.H, A, 3, 1.0f, 1.0f, &b, &w, kTriMargin)) {
        box = make_int4(1, 1, 0, 0);  // nothing of it in front of the camera inside the frustum
      } else if (w > 0.0f) {           // (0: a vertex on the camera plane, the band)
        const float e = 3.0e-5f * M + 2.0f * dev, ed = 8.0e-6f * M + 2.0f * dev;
        if (e < 0.005f * w) {
          const int extra = (int)(e / w * 0.5f * (float)max(p.W, p.H) + 0.25f);
          box = make_int4(max(b.x - extra, band.x), max(b.y - extra, band.y), min(b.z + extra, band.z),
                          min(b.w + extra, band.w));
          tmin = ed < 2.0e-4f * w ? w * 0.9999f : 0.0f;
        }
      }
    }
  }
  bins_count_item(p.leaf_bins, i, box, tmin);
}

__global__ void __launch_bounds__(256) PT_RASTER_ATTR wf_primary_tri(PTParams p) {
  __shared__ float4 sa[kTChunk];      // (p1, N.p1)
  __shared__ float sv[kTChunk * 9];   // p2, p3, N
  __shared__ uint2 sbox[kTChunk];     // (x0 | x1 << 16, y0 | y1 << 16)
  __shared__ float stmin[kTChunk];
  __shared__ int sidx[kTChunk];
  // per wave: the chunk's triangles that can meet its 8 x 8 pixels: slot | columns << 16 | rows << 24 (the pixels
  // of the wave inside the triangle's box)
  __shared__ uint32_t wlist[4][kTChunk];
  const Bins& bn = p.leaf_bins;
  if (bn.ctr[2]) return;  // overflow: wf_primary_coop / wf_primary walk every pixel
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  const int tile = blockIdx.x, gt = tile * p.tile_stride + p.tile_offset, ntx = (p.W + 15) / 16;
  const int x = (gt % ntx) * 16 + (wv & 1) * 8 + (ln & 7);
  const int y = p.y0 + (gt / ntx) * 16 + (wv >> 1) * 8 + (ln >> 3);
  const bool valid = x < p.W && y < p.y1;
  const int pid = (y - p.y0) * p.W + x;
  const v3 S = mk(p.eye[0], p.eye[1], p.eye[2]);
  const v3 d = primary_dir(p, x, y);
  const float bound = raster_bound(p, valid, x, y, S);
  float tbest = bound;
  int best = -1, last_leaf = -1;
  bool tied = false, last_ok = false;
  uint32_t steps = 0;
  // the tile's loosest pruning bound, as wf_primary_raster: triangles beyond it are left out of the staged chunk
  __shared__ float wmax[4];
  __shared__ int wcount[4];
  float tb = valid ? bound : 0.0f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tb = fmaxf(tb, __shfl_xor(tb, o));
  if (ln == 0) wmax[wv] = tb;
  __syncthreads();
  const float tile_lim = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])) * 1.0004f + 4.0e-4f;
  const uint32_t mine = (1u << (16 + (ln & 7))) | (1u << (24 + (ln >> 3)));
  const int wx0 = x - (ln & 7), wy0 = y - (ln >> 3);
  const int off = bn.tile_off[gt], total = bn.tile_off[gt + 1] - off;
  for (int base = 0; base < total; base += kTChunk) {
    __syncthreads();
    const int j = base + (int)threadIdx.x;
    const bool mine_j = (int)threadIdx.x < kTChunk && j < total;
    int tri = 0;
    float tm = 0.0f;
    if (mine_j) {
      tri = bn.pairs[off + j];
      tm = bn.tmin[tri];
    }
    const bool keep = mine_j && !(tm > tile_lim);
    const unsigned long long km = __ballot(keep);
    if (ln == 0) wcount[wv] = __popcll(km);
    __syncthreads();
    int n = 0, slot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      slot += w < wv ? wcount[w] : 0;
      n += wcount[w];
    }
    if (keep) {  // compacted in thread order
      slot += __popcll(km & ((1ull << ln) - 1ull));
      const float4* g = p.scene.tri_geom + 4 * (size_t)tri;
      const float4 g1 = g[1], g2 = g[2], g3 = g[3];
      const int4 b = bn.box[tri];
      sa[slot] = g[0];
      float* q = sv + 9 * slot;
      q[0] = g1.x; q[1] = g1.y; q[2] = g1.z;
      q[3] = g2.x; q[4] = g2.y; q[5] = g2.z;
      q[6] = g3.x; q[7] = g3.y; q[8] = g3.z;
      sbox[slot] = make_uint2((uint32_t)b.x | ((uint32_t)b.z << 16), (uint32_t)b.y | ((uint32_t)b.w << 16));
      stmin[slot] = tm;
      sidx[slot] = tri;
    }
    __syncthreads();
    // this wave's share of the chunk, in chunk order (the order does not change the closest t, a unique closest
    // triangle or an exact tie met): the staged triangles whose box meets the wave's pixels and whose bound does not
    // exceed the loosest of its pixels' pruning bounds, each with the pixels inside its box
    float wl = valid ? tbest * 1.0002f + 2.0e-4f : 0.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wl = fmaxf(wl, __shfl_xor(wl, o));
    int wn = 0;
    for (int k0 = 0; k0 < n; k0 += 64) {
      const int k = k0 + ln;
      uint32_t ent = 0;
      if (k < n && !(stmin[k] > wl)) {
        const uint2 b = sbox[k];
        const int c0 = max((int)(b.x & 0xffffu) - wx0, 0), c1 = min((int)(b.x >> 16) - wx0, 7);
        const int r0 = max((int)(b.y & 0xffffu) - wy0, 0), r1 = min((int)(b.y >> 16) - wy0, 7);
        if (c0 <= c1 && r0 <= r1)
          ent = (uint32_t)k | (((0xffu >> (7 - c1)) & (0xffu << c0) & 0xffu) << 16) |
                (((0xffu >> (7 - r1)) & (0xffu << r0) & 0xffu) << 24);
      }
      const unsigned long long m = __ballot(ent != 0u);
      if (ent) wlist[wv][wn + __popcll(m & ((1ull << ln) - 1ull))] = ent;
      wn += __popcll(m);
    }
    __syncthreads();
    if (!valid) continue;
    uint32_t next = wn > 0 ? wlist[wv][0] : 0u;
    for (int i = 0; i < wn; ++i) {
      const uint32_t ent = (uint32_t)__builtin_amdgcn_readfirstlane((int)next);  // the same for every lane
      next = wlist[wv][min(i + 1, wn - 1)];  // (read an iteration ahead)
      // the triangle's record is read before the tests that may skip it: every lane reads the same words, and the
      // reads then overlap instead of waiting for the box and bound tests
      const int k = (int)(ent & 0xffffu);
      const float tm = stmin[k];
      const float* q = sv + 9 * k;
      const TriGeom tg{sa[k], f4(q[0], q[1], q[2], 0.0f), f4(q[3], q[4], q[5], 0.0f), f4(q[6], q[7], q[8], 0.0f)};
      if ((ent & mine) != mine) continue;                 // this pixel lies outside the triangle's box
      if (tm > tbest * 1.0002f + 2.0e-4f) continue;       // wholly beyond the walk's pruning bound (traverse<0>)
      float t;
      ++steps;
      if (!tri_test(tg, S, d, &t) || !(t <= tbest)) continue;
      // a hit that counts: the reference tested this triangle only if the ray passes its leaf's box
      const int tri = sidx[k], leaf = p.scene.tri_leaf[tri];
      if (leaf != last_leaf) {
        const float4 lo = p.scene.leaves[2 * leaf], hi = p.scene.leaves[2 * leaf + 1];
        const v3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        float t0;
        last_ok = slab(S, inv, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, &t0) > 0.0f;
        last_leaf = leaf;
        ++steps;
      }
      if (!last_ok) continue;
      if (t < tbest) { tbest = t; best = tri; tied = false; }
      else if (best >= 0) tied = true;  // t == tbest
    }
  }
  const bool walk = valid && (tied || (best < 0 && bound < PT_INF));  // a tie, or nothing below the G-buffer bound
  raster_finish(p, valid, walk, pid, best, tbest, steps, tile, y);
}

// ------------------------------------------------------- the stage's launches ---
// One frame's primary hits into f.wf.hit, and from their costs the tile order of the bounce-0 shade and the next frame.
int launch_primary_stage(const PTParams& f, WfStack stack, int ntiles, hipStream_t s) {
  auto walk = [&](const PTParams& q, int blocks) {
    with_stack(stack, [&](auto ks, auto deep) {
      hipLaunchKernelGGL((wf_primary<ks(), deep()>), dim3(blocks), dim3(256), 0, s, q,
                         ntiles);
    });
  };
  if (f.primary_raster) {  // triangles (2) or leaves binned to every tile of the band; the subset's tiles rasterised
    const bool tris = f.primary_raster == 2;
    const int nitems = f.leaf_bins.n;
    if (nitems > 0) {
      if (tris) hipLaunchKernelGGL(pr_tri_setup, dim3((nitems + 255) / 256), dim3(256), 0, s, f);
      else hipLaunchKernelGGL(pr_setup, dim3((nitems + 255) / 256), dim3(256), 0, s, f);
    }
    const int rc = launch_bins(f.leaf_bins, s);
    if (rc) return rc;
    if (tris) hipLaunchKernelGGL(wf_primary_tri, dim3(ntiles), dim3(256), 0, s, f);
    else hipLaunchKernelGGL(wf_primary_raster, dim3(ntiles), dim3(256), 0, s, f);
    if (f.closest_tree) launch_primary_coop(f, s);
    static const bool fix_launch = [] {  // A/B only: PTSVGF_PRIMARY_FIX_LAUNCH=1 launches it anyway (512 blocks)
      const char* e = getenv("PTSVGF_PRIMARY_FIX_LAUNCH");
      return e && atoi(e) != 0;
    }();
    if (!f.closest_tree || fix_launch) {  // the flagged pixels (and, after an overflow, all) by the per-pixel walk
      PTParams q = f;
      q.pr_fix = f.leaf_bins.ctr;
      walk(q, f.closest_tree ? std::min(ntiles, 512) : ntiles);
    }
  } else {
    walk(f, ntiles);
  }
  if (f.tiles.cost)  // this frame's primary costs -> tile order of the bounce-0 shade and the next frame
    return launch_tile_sort(f.tiles.cost, f.tiles.perm_next, f.tiles.ntiles, s);
  return 0;
}

}  // namespace ptk

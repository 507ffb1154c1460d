// kernels_wf_shade.hip — the wavefront path tracer's stages without a traversal stack (kernels_wavefront.hip has the
// schedule): the shade of a bounce (wf_shade, wf_shade_counted), the busy-tile list of its keep mode, the finish that
// applies a bounce's shadow verdicts (wf_finish) and the unfolded draws' finalize (wf_finalize).
#include <hip/hip_runtime.h>

#include "glsl_builtins.h"
#include "pt_device.h"
#include "pt_shading.h"
#include "wf_common.h"

using namespace glsl;

namespace ptk {

// shade()'s MIS combination (:950-966) for given shadow verdicts: hdriLight zeroes
// its value and pdf when occluded, calculatePointLight only its value.
struct NeeTerms {
  v3 hcalc, pcalc, bcalc;
  float hpdf, ppdf, bpdf;
};
__device__ __forceinline__ v3 nee_hit_light(v3 red, const NeeTerms& t, bool occ_h, bool occ_p) {
  v3 hcalc = t.hcalc, pcalc = t.pcalc;
  float hpdf = t.hpdf;
  if (occ_h) { hpdf = 0.0f; hcalc = splat(0.0f); }  // :934-937
  if (occ_p) pcalc = splat(0.0f);                   // :905-909 (pdf kept)
  float sw = ((hpdf + t.ppdf) + t.bpdf) + 1e-6f;
  float w1 = hpdf / sw, w2 = t.ppdf / sw, w3 = t.bpdf / sw;
  return mul(red, add(add(muls(hcalc, w1), muls(pcalc, w2)), muls(t.bcalc, w3)));
}
__device__ __forceinline__ bool zero_bits(v3 a) {  // all three exactly +0.0f
  return (__float_as_uint(a.x) | __float_as_uint(a.y) | __float_as_uint(a.z)) == 0u;
}

// A path's end: wf_finalize's statements for the radiance `light` of pixel (x, y).
__device__ __forceinline__ void terminal_write(const PTParams& p, int x, int y, v3 light) {
  light = vclamp(light, 0.0f, p.clamp_threshold);  // :1110-1113
  v3 color = splat(0.0f);
  if (!f_isnan(light.x) && !f_isnan(light.y) && !f_isnan(light.z)) color = light;
  if (p.accumulate && p.last.p) {  // :1116-1119
    float4 lc = pld(p.last, x, y);
    color = mixv(xyz(lc), color, 1.0f / (float)(p.frameCounter + 1u));
  }
  pst(p.color, x, y, f4(color.x, color.y, color.z, 1.0f));
}
// A bounce's shadow verdicts applied to the path of pixel `pid`: wf_finish's statements on (red, light).
__device__ __forceinline__ void finish_apply(const PTParams& p, int pid, v3* red_io, v3* light_io) {
  float4 q0 = ldnt(&p.wf.pend0[pid]), q1 = ldnt(&p.wf.pend1[pid]), q2 = ldnt(&p.wf.pend2[pid]), q3 = ldnt(&p.wf.pend3[pid]);
  NeeTerms nt;
  nt.hcalc = xyz(q0); nt.pcalc = xyz(q1); nt.bcalc = xyz(q2);
  nt.hpdf = q0.w; nt.bpdf = q1.w;
  nt.ppdf = p.pointLightSize != 0 ? (2.0f * PT_PI) / (float)p.pointLightSize : 0.0f;
  v3 cosb = xyz(q3);
  v3 red = *red_io, light = *light_io;
  const bool occ_p = p.wf.occ_p[pid] != 0;
  // The verdict cache's write-back (point_cache.h), only in the launch that consumes bounce 0's verdicts (every other
  // launch gets kPcOff): the light whose ray the bounce-0 shade queued for this pixel is now known. The five kernels
  // that write occ_p stay as they are, so a cached verdict is the one the walk produced.
  if (p.point_cache != kPcOff) {
    const uint32_t w = p.wf.pcache[pid];
    if (pc_pending(w) >= 0) p.wf.pcache[pid] = (uint16_t)pc_resolve(w, occ_p);
  }
  v3 hitLight = nee_hit_light(red, nt, p.wf.occ_h[pid] != 0, occ_p);
  red = mul(red, divs(cosb, nt.bpdf));
  light = add(light, hitLight);
  *red_io = red;
  *light_io = light;
}

// ------------------------------------------------------------------ shade ---
// Bounce i: consume the closest hit of the ray in (ray_o, ray_d); on a hit,
// sample the next direction and prepare both NEE contributions (:948-968).
// Shadow rays whose verdict cannot change a bit of the result (a light below the
// surface: zero BRDF) are not queued; the others go to one compacted list.
#ifndef PT_SHADE_WAVES
// waves/SIMD wf_shade is compiled for, at least (0: the compiler's choice). 4: the folded shades of later bounces,
// left to the compiler, take 152 / 148 VGPRs = 3 waves; held to 4 they fit 128 VGPRs with 20 / 12 bytes of private
// segment (the unfolded kernel: 128 VGPRs either way). The first-bounce instantiations take 84 / 82 = 5 waves.
#define PT_SHADE_WAVES 4
#endif
#if PT_SHADE_WAVES > 0
#define PT_SHADE_ATTR __attribute__((amdgpu_waves_per_eu(PT_SHADE_WAVES)))
#else
#define PT_SHADE_ATTR
#endif
// FOLD (uniform shade_fold): paths end where they end. A path that ends in this shade (a miss, a hit that pushes no
// ray) writes its pixel's `color` itself (terminal_write) and stores no state; a shade after the first applies the
// previous bounce's shadow verdicts in registers (finish_apply: the wf_finish launch between two shades is gone); the
// last bounce's wf_finish<true> writes `color` for the paths still alive, and wf_finalize is not launched. FIRST /
// LAST (the bounce is the first / the last of the path; read only with FOLD) drop at compile time the loads the first
// bounce does not have and the stores nothing reads after the last: ray_d and seed. `red` and `light` are still
// stored on the last bounce's continuing paths, whose wf_finish<true> reads both. The statements and their order
// per path are those of the unfolded launches, so every plane keeps its bits.
// COUNTED (wf_shade_counted: sample `sample` >= 1 of an spp draw with a count plane bound, DESIGN.md "Adaptive sample
// counts"): a bounce-0 pixel whose count c has max(c, 1) <= sample is no pixel of this launch: it reads and stores
// nothing and appends to no list. sample_counts: one uint8 per frame pixel, global rows.
template <bool FOLD, bool FIRST, bool LAST, bool COUNTED>
__device__ __forceinline__ void shade_body(const PTParams& p, int bounce_rt, const int* __restrict__ list_in,
                                           const int* __restrict__ counts_in, int* __restrict__ list_out,
                                           int* __restrict__ counts_out, int* __restrict__ shadow_out,
                                           int* __restrict__ shadow_counts, int cap,
                                           const uint8_t* __restrict__ sample_counts, int sample) {
  // folded: bounce_rt is any bounce of the instantiation's kind; only `bounce == 0` is decided at compile time
  const int bounce = FOLD && FIRST ? 0 : bounce_rt;
  const bool first = FOLD ? FIRST : bounce == 0;
  // keep mode (PTParams::busy) exists in the folded bounce-0 shade of a one-sample draw alone
  constexpr bool kKeep = FOLD && FIRST && !COUNTED;
  // bounce 0: one tile per block. Later bounces: 256 list items per chunk, a block taking chunks blockIdx.x,
  // + gridDim.x, ... (a grid a multiple of kSeg: chunk c appends to segment c % kSeg, as one block per chunk did)
  int total = 0;
  if (!first)
    for (int i = 0; i < kLiveBins * kSeg; ++i) total += counts_in[i];
  for (int c = blockIdx.x; first || c * 256 < total; c += gridDim.x) {
    const int k = c * 256 + threadIdx.x;
    int pid = 0;
    bool valid;
    if (first) {
      // one 16 x 16 primary tile per block, in descending order of this frame's primary-ray cost
      // (tiles.perm_next, sorted right after wf_primary): the rays of expensive tiles are appended to
      // the lists first, so every later list-driven trace launch starts its slowest rays first
      const int ntx = (p.W + 15) / 16;
      int slot;
      if (kKeep && p.busy) {  // keep mode: the tiles that hold a primary hit, in the same order (launch_busy_tiles)
        if ((int)blockIdx.x >= p.busy[0]) return;
        slot = p.busy[1 + blockIdx.x];
      } else {
        slot = p.tiles.cost ? p.tiles.perm_next[blockIdx.x] : (int)blockIdx.x;
      }
      const int tile = slot * p.tile_stride + p.tile_offset;
      const int x = (tile % ntx) * 16 + (threadIdx.x & 15), ly = (tile / ntx) * 16 + (threadIdx.x >> 4);
      valid = x < p.W && ly < p.y1 - p.y0;
      pid = ly * p.W + x;
      if (COUNTED && valid) valid = sample < max((int)sample_counts[(size_t)(p.y0 + ly) * p.W + x], 1);
    } else {
      valid = bins_get(list_in, counts_in, kLiveBins, cap, k, &pid);
    }
    bool push = false, need_h = false, need_p = false;
    bool served = false;  // (bounce 0, point_cache = use) the point-light verdict came from the cache: no ray
    int pbin = 0;  // point-light list of this ray (light index mod kPointBins)
    int lbin = 0;  // live list of the continuing ray (direction octant)
    if (valid) {
      int x, y;
      pix_xy(p, pid, &x, &y);
      int2 hr = ldnt(&p.wf.hit[pid]);
      v3 S, d;
      uint32_t seed;
      v3 light, red;
      // bounce 0 with the verdict cache engaged (point_cache.h): the pixel's word, and whether this thread stores it.
      // Reset: every pixel stores a fresh word. Use: only a pixel that queues a ray whose verdict is not known yet.
      // (Folded bounce-0 instantiations only: the unfolded shade, shade_fold = 0, decides `first` at run time and
      // spilled 32 bytes more with this in it, so the host bypasses the cache for it.)
      constexpr bool kPc = FOLD && FIRST;
      uint32_t pcw = 0;
      bool pc_store = kPc && p.point_cache == kPcReset;
      if (first) {
        S = mk(p.eye[0], p.eye[1], p.eye[2]);
        d = primary_dir(p, x, y);
        seed = ((uint32_t)x * 1973u + (uint32_t)y * 9277u + p.frameCounter * 26699u) | 1u;  // :433-436
        wang_hash(&seed);  // AA jitter rand() x2 (:1060), never applied
        wang_hash(&seed);
        light = splat(0.0f);
        red = splat(1.0f);
      } else {
        S = xyz(ldnt(&p.wf.ray_o[pid]));
        d = xyz(ldnt(&p.wf.ray_d[pid]));
        seed = ldnt(&p.wf.seed[pid]);
        light = xyz(ldnt(&p.wf.light[pid]));
        red = xyz(ldnt(&p.wf.red[pid]));
        if (FOLD) finish_apply(p, pid, &red, &light);  // the previous bounce's verdicts (its wf_finish)
      }
      if (kKeep && p.busy && hr.x < 0) {
        // keep mode: `color`, `emission` and `albedo` already hold what the branch below would store
      } else if (hr.x < 0) {  // miss (:1084-1087)
        light = add(light, mul(hdr_color(p, d), red));
        // (folded, null planes: a sample after the first of an spp draw, whose first-hit planes are sample 0's; the
        // unfolded instantiation keeps its code: launch_wavefront points such a sample's stores elsewhere)
        if (first && (!FOLD || p.emission.p)) {
          pst(p.emission, x, y, f4(0.0f, 0.0f, 0.0f, 1.0f));
          pst(p.albedo, x, y, f4(0.0f, 0.0f, 0.0f, 1.0f));
        }
        if (FOLD) terminal_write(p, x, y, light);
      } else {
        Hit h = decode_hit(p.scene, hr.x, __int_as_float(hr.y), S, d);
        if (first && (!FOLD || p.emission.p)) {
          pst(p.emission, x, y, f4(h.m.emissive.x, h.m.emissive.y, h.m.emissive.z, 1.0f));
          pst(p.albedo, x, y, f4(h.m.baseColor.x, h.m.baseColor.y, h.m.baseColor.z, 1.0f));
        }
        uint32_t ps = ((uint32_t)x * 1973u + (uint32_t)y * 9277u + (uint32_t)(114514 / 1919) * 26699u) | 1u;
        float cpu = u32_to_unit(wang_hash(&ps));
        float cpv = u32_to_unit(wang_hash(&ps));
        float xi1 = p.sobol_u[bounce] + cpu;
        if (xi1 > 1.0f) xi1 -= 1.0f;
        if (xi1 < 0.0f) xi1 += 1.0f;
        float xi2 = p.sobol_v[bounce] + cpv;
        if (xi2 > 1.0f) xi2 -= 1.0f;
        if (xi2 < 0.0f) xi2 += 1.0f;
        float xi3 = u32_to_unit(wang_hash(&seed));
        v3 V = neg(h.viewDir);
        v3 L = sample_brdf(xi1, xi2, xi3, V, h.normal, h.m);
        // the reference ends the path on NdotL <= 0 (:1016, :1098): a NaN NdotL (a NaN vertex normal) goes on, its
        // radiance turns NaN and the pixel ends at 0 (:1110-1113); `> 0` ended such a path with what it had gathered
        if (!(dot(h.normal, L) <= 0.0f)) {
          push = true;
                  v3 brdf = brdf_eval(V, h.normal, L, h.m);
          float bpdf = brdf_pdf(V, h.normal, L, h.m);
          // hdriLight, evaluated as if unoccluded (:922-946)
          float r1 = u32_to_unit(wang_hash(&seed));
          float r2 = u32_to_unit(wang_hash(&seed));
          v3 hd = sample_hdr(p, r1, r2);
          float hpdf;
          v3 hv = hdr_color_pdf(p, hd, &hpdf);
          v3 hb = brdf_eval(V, h.normal, hd, h.m);
          v3 hcalc = divs(mul(muls(hb, f_abs(dot(hd, h.normal))), hv), hpdf);
          // calculatePointLight, as if unoccluded (:884-919)
          v3 pcalc = splat(0.0f);
          float4 shp = f4(0.0f, 0.0f, 0.0f, -1.0f);
          int li = 0;
          if (p.pointLightSize != 0) {
            float ppdf = (2.0f * PT_PI) / (float)p.pointLightSize;
            li = (int)(u32_to_unit(wang_hash(&seed)) * (float)p.pointLightSize);
            pbin = li & (kPointBins - 1);
            v3 lpos = splat(0.0f), lrad = splat(0.0f);
            if (li >= 0 && li < p.scene.nlights_buf) {
              const float* lp = p.scene.lights + 6 * li;
              lpos = mk(lp[0], lp[1], lp[2]);
              lrad = mk(lp[3], lp[4], lp[5]);
            }
            v3 ld = normalize(sub(lpos, h.P));
            float dist = length(sub(lpos, h.P));
            v3 plv = divs(lrad, dist * dist);
            v3 pb = brdf_eval(V, h.normal, ld, h.m);
            pcalc = divs(muls(mul(plv, pb), f_abs(dot(ld, h.normal))), ppdf);
            shp = f4(ld.x, ld.y, ld.z, dist);
          }
          v3 cosb = muls(brdf, f_abs(dot(L, h.normal)));
          v3 bcalc = divs(mul(h.m.emissive, cosb), bpdf);
          // A verdict only zeroes terms: with the point value exactly +0 (light below the
          // surface: zero BRDF) its ray cannot change a bit; the HDR verdict also moves the
          // MIS weights, so it is dropped only when every term is +0 and every pdf finite.
          const bool pz = zero_bits(pcalc);
          need_p = shp.w >= 0.0f && !pz;
          need_h = !(pz && zero_bits(hcalc) && zero_bits(bcalc) && __builtin_isfinite(hpdf) && __builtin_isfinite(bpdf));
          // The verdict "light li is occluded from this pixel's first hit" does not depend on the frame: once a ray
          // has brought it back (finish_apply), later frames of the same view store it instead of queueing the ray.
          uint8_t occ_p0 = 0;
          if (kPc && p.point_cache != kPcOff && need_p && (unsigned)li < (unsigned)kPcLights) {
            if (p.point_cache == kPcUse) {
              pcw = p.wf.pcache[pid];
              const int v = pc_lookup(pcw, li);
              if (v >= 0) {
                occ_p0 = (uint8_t)v;
                need_p = false;
                served = true;
              }
            }
            if (need_p) {
              pcw = pc_mark_pending(pcw, li);
              pc_store = true;
            }
          }
          stnt(&p.wf.pend0[pid], f4(hcalc.x, hcalc.y, hcalc.z, hpdf));
          stnt(&p.wf.pend1[pid], f4(pcalc.x, pcalc.y, pcalc.z, bpdf));
          stnt(&p.wf.pend2[pid], f4(bcalc.x, bcalc.y, bcalc.z, 0.0f));
          stnt(&p.wf.pend3[pid], f4(cosb.x, cosb.y, cosb.z, 0.0f));
          stnt(&p.wf.sh_h[pid], f4(hd.x, hd.y, hd.z, 0.0f));
          stnt(&p.wf.sh_p[pid], shp);
          stnt(&p.wf.ray_o[pid], f4(h.P.x, h.P.y, h.P.z, 0.0f));
          if (!(FOLD && LAST)) stnt(&p.wf.ray_d[pid], f4(L.x, L.y, L.z, 0.0f));
          stnt(&p.wf.red[pid], f4(red.x, red.y, red.z, 0.0f));
          stnt(&p.wf.occ_h[pid], (uint8_t)0);
          stnt(&p.wf.occ_p[pid], occ_p0);
        } else if (FOLD) {
          terminal_write(p, x, y, light);
        }
      }
      if (!FOLD || (push && !LAST)) stnt(&p.wf.seed[pid], seed);
      if (!FOLD || push) stnt(&p.wf.light[pid], f4(light.x, light.y, light.z, 0.0f));
      if (pc_store) p.wf.pcache[pid] = (uint16_t)pcw;
    }
    if (FOLD && FIRST && p.point_cache == kPcUse) {
      // pt_debug_point_cache_counts: one add per block that served any, spread over 8 words as the lists' segment
      // counts are (a 4K frame has 32 400 blocks; per wave into one word the adds queued up at one L2 address)
      const int n = __syncthreads_count(served);
      if (threadIdx.x == 0 && n) atomicAdd(&p.wf.counters[kCtrPcServed + (blockIdx.x & 7)], n);
    }
    // HDR and point-light shadow rays go to separate lists so trace waves stay homogeneous

    block_push_shade(push, lbin, need_h, need_p, pbin, pid, list_out, counts_out, shadow_out, shadow_counts, cap, c);
    if (first) break;
    __syncthreads();  // the next chunk's push reuses block_push_shade's shared counters
  }
}

template <bool FOLD, bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) PT_SHADE_ATTR wf_shade(PTParams p, int bounce_rt, const int* __restrict__ list_in,
                                                const int* __restrict__ counts_in, int* __restrict__ list_out,
                                                int* __restrict__ counts_out, int* __restrict__ shadow_out,
                                                int* __restrict__ shadow_counts, int cap) {
  shade_body<FOLD, FIRST, LAST, false>(p, bounce_rt, list_in, counts_in, list_out, counts_out, shadow_out, shadow_counts,
                                       cap, nullptr, 0);
}

// The bounce-0 shade of sample `sample` >= 1 of an spp draw with a count plane bound (the unfolded one: FOLD = LAST =
// false, as wf_shade<false, false, false> at bounce 0). Launched in place of wf_shade only then.
template <bool FOLD, bool LAST>
__global__ void __launch_bounds__(256) PT_SHADE_ATTR wf_shade_counted(PTParams p, int* __restrict__ list_out,
                                                                      int* __restrict__ counts_out,
                                                                      int* __restrict__ shadow_out,
                                                                      int* __restrict__ shadow_counts, int cap,
                                                                      const uint8_t* __restrict__ sample_counts,
                                                                      int sample) {
  shade_body<FOLD, FOLD, LAST, true>(p, 0, nullptr, nullptr, list_out, counts_out, shadow_out, shadow_counts, cap,
                                     sample_counts, sample);
}

// ------------------------------------------------------- the busy-tile list ---
// The bounce-0 shade's keep mode visits only the tiles that hold a primary hit (PTParams::busy). Block b looks at the
// tile the bounce-0 shade's block b takes (p.wf.hit is the primary plane here, as for that shade) and leaves its name
// in scratch[b], or -1 when every pixel of it misses. Every index comes from the launch geometry: b < ntiles.
__global__ void __launch_bounds__(256) wf_busy_mark(PTParams p, int* __restrict__ scratch) {
  const int ntx = (p.W + 15) / 16;
  const int slot = p.tiles.cost ? p.tiles.perm_next[blockIdx.x] : (int)blockIdx.x;
  const int tile = slot * p.tile_stride + p.tile_offset;
  const int x = (tile % ntx) * 16 + (threadIdx.x & 15), ly = (tile / ntx) * 16 + (threadIdx.x >> 4);
  const bool hit = x < p.W && ly < p.y1 - p.y0 && ldnt(&p.wf.hit[ly * p.W + x]).x >= 0;
  const int any = __syncthreads_or(hit);
  if (threadIdx.x == 0) scratch[blockIdx.x] = any ? slot : -1;
}
// One block packs the names that are not -1 to busy[1 ..], keeping their order, and writes their number to busy[0].
// n names at most, so entry 1 + (names before this one) stays below 1 + n.
__global__ void __launch_bounds__(1024) wf_busy_pack(const int* __restrict__ scratch, int n, int* __restrict__ busy) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int c = 0; c < n; c += 1024) {
    const int i = c + (int)threadIdx.x;
    const int v = i < n ? scratch[i] : -1;
    const unsigned long long m = __ballot(v >= 0);
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int k = 0; k < w; ++k) off += wsum[k];
    if (v >= 0) busy[1 + off + __popcll(m & ((1ull << lane) - 1ull))] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int k = 0; k < 16; ++k) t += wsum[k];
      base += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) busy[0] = base;
}

int launch_busy_tiles(const PTParams& p, int* busy, hipStream_t s) {
  const int ntiles = wf_subset_tiles(p.W, std::max(0, p.y1 - p.y0), p.tile_stride, p.tile_offset);
  if (ntiles <= 0 || !busy || !p.wf.hit0) return (int)hipErrorInvalidValue;
  PTParams f = p;
  f.wf.hit = f.wf.hit0;
  int* scratch = busy + 1 + ntiles;
  hipLaunchKernelGGL(wf_busy_mark, dim3(ntiles), dim3(256), 0, s, f, scratch);
  hipLaunchKernelGGL(wf_busy_pack, dim3(1), dim3(1024), 0, s, (const int*)scratch, ntiles, busy);
  return (int)hipGetLastError();
}

// ----------------------------------------------------------------- finish ---
// TERMINAL (the last bounce's finish with shade_fold): the path ends here, so its pixel's `color` is written
// (terminal_write) and neither `red` nor `light` is stored.
template <bool TERMINAL>
__global__ void __launch_bounds__(256) wf_finish(PTParams p, const int* __restrict__ list,
                                                 const int* __restrict__ counts, int cap) {
  int total = 0;
  for (int i = 0; i < kLiveBins * kSeg; ++i) total += counts[i];
  for (int k = blockIdx.x * 256 + threadIdx.x; k < total; k += gridDim.x * 256) {
    int pid;
    if (!bins_get(list, counts, kLiveBins, cap, k, &pid)) continue;
    v3 red = xyz(ldnt(&p.wf.red[pid])), light = xyz(ldnt(&p.wf.light[pid]));
    finish_apply(p, pid, &red, &light);
    if (TERMINAL) {
      int x, y;
      pix_xy(p, pid, &x, &y);
      terminal_write(p, x, y, light);
    } else {
      stnt(&p.wf.red[pid], f4(red.x, red.y, red.z, 0.0f));
      stnt(&p.wf.light[pid], f4(light.x, light.y, light.z, 0.0f));
    }
  }
}

// --------------------------------------------------------------- finalize ---
__global__ void __launch_bounds__(256) wf_finalize(PTParams p) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= p.W * (p.y1 - p.y0)) return;
  int x, y;
  pix_xy(p, k, &x, &y);
  if (p.tile_stride > 1) {  // pixels of tiles outside the subset keep their contents
    const int t = ((y - p.y0) >> 4) * ((p.W + 15) / 16) + (x >> 4);
    if (t % p.tile_stride != p.tile_offset) return;
  }
  terminal_write(p, x, y, xyz(ldnt(&p.wf.light[k])));
}

// ------------------------------------------------------- the stage's launches ---
// Bounce i's shade of one frame: one block per primary tile at bounce 0, the list-driven grid after. Unfolded draws
// (shade_fold = 0, A/B) launch the one run-time instantiation for every bounce.
void launch_shade(const WfDraw& d, const PTParams& f, int i, bool fold, bool last, hipStream_t s) {
  const bool first = i == 0;
  const auto kernel = !fold   ? wf_shade<false, false, false>
                      : first ? (last ? wf_shade<true, true, true> : wf_shade<true, true, false>)
                              : (last ? wf_shade<true, false, true> : wf_shade<true, false, false>);
  const int* live_in = f.wf.counters + kWfCtr * (i > 0 ? i - 1 : 0);
  hipLaunchKernelGGL(kernel, dim3(first ? d.ntiles : d.gL), dim3(256), 0, s, f, i, (const int*)wf_live_list(f, i + 1),
                     live_in, wf_live_list(f, i), f.wf.counters + kWfCtr * i, f.wf.shadow_list,
                     f.wf.counters + kWfCtr * i + kCtrHdr, d.cap);
}

// The bounce-0 shade of sample `sample` >= 1 of an spp draw with a count plane: samples after the first skip the
// pixels that do not take them (sample 0 exists everywhere).
void launch_shade_counted(const WfDraw& d, const PTParams& f, bool fold, bool last, const uint8_t* sample_counts,
                          int sample, hipStream_t s) {
  const auto kernel = !fold ? wf_shade_counted<false, false>
                            : (last ? wf_shade_counted<true, true> : wf_shade_counted<true, false>);
  hipLaunchKernelGGL(kernel, dim3(d.ntiles), dim3(256), 0, s, f, wf_live_list(f, 0), f.wf.counters, f.wf.shadow_list,
                     f.wf.counters + kCtrHdr, d.cap, sample_counts, sample);
}

void launch_finish(const WfDraw& d, const PTParams& f, int i, bool terminal, hipStream_t s) {
  const auto kernel = terminal ? wf_finish<true> : wf_finish<false>;
  hipLaunchKernelGGL(kernel, dim3(d.gL), dim3(256), 0, s, f, (const int*)wf_live_list(f, i),
                     (const int*)(f.wf.counters + kWfCtr * i), d.cap);
}

void launch_finalize(const WfDraw& d, const PTParams& f, hipStream_t s) {
  hipLaunchKernelGGL(wf_finalize, dim3((d.N + 255) / 256), dim3(256), 0, s, f);
}

}  // namespace ptk

// wf_common.h — what the wavefront path tracer's translation units share (kernels_wavefront.hip: the schedule;
// kernels_wf_primary.hip, kernels_wf_trace.hip, kernels_wf_shade.hip: its stages; kernels_spp.hip: the resolve): the
// traversal block and its occupancy attribute, the compacted ray lists, the trace counters, the per-lane stack, the
// primary ray, and the stage launchers that cross those files. Included by them alone; what capi*.hip calls is
// declared in pt_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "glsl_builtins.h"
#include "pt_device.h"
#include "pt_shading.h"

namespace ptk {

constexpr int kTB = 128;  // threads per traversal block (LDS stack: kStack*kTB*4 = 16 KiB)
// Resident waves per SIMD the traversal kernels are compiled for. Round 3 (SLP vectorizer on): 98 VGPRs left alone,
// 96 at 5 waves (4K 179.8 -> 185.8 fps, profiles/r03/occupancy_ab.log). With SLP off the 4-wide refill walks need
// 63-67 VGPRs; 8 waves fits them in 64 without spills, which pays once the LDS stack allows 8 waves (PT_WIDE_KS 16:
// 8 KiB per 2-wave block). Round 4, same box, two alternating repetitions (profiles/r04/occupancy_ab.log): default
// 24 entries / 5 waves 210.8 / 210.5 fps at 4K, 68.5 / 68.6 surface view; 16 / 5 waves 212.2 / 211.7, 68.9 / 68.6;
// 16 / 8 waves 214.7 / 212.3, 69.4 / 69.0; 12 / 8 waves 199.9 / 198.3, 59.9 / 59.2 (more rays overflow to the
// cooperative walk). Round 5: the sign-selected planes of the 4-wide step (PT_WIDE_SIGNED) need a few more VGPRs; at
// 8 waves they spill 40-44 B per lane, at 7 (72 VGPRs) 8-12 B outside the walk loop: 7 kept (pt_device.h PT_WIDE_SIGNED,
// profiles/r05/wide_signed/).
#ifndef PT_TRACE_WAVES_PER_EU
#define PT_TRACE_WAVES_PER_EU 7
#endif
#if PT_TRACE_WAVES_PER_EU > 0
#define PT_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(PT_TRACE_WAVES_PER_EU)))
#else
#define PT_TRACE_ATTR
#endif

// LDS stack entries of the 4-wide lane-refill walks. Unlike the binary walks (sized by the tree's depth: kStack /
// kStackSmall), a 4-wide walk whose pushes would overflow hands its ray to the cooperative walk (wide_step), so the
// stack can be smaller than the deepest path: it bounds the resident waves (kTB x entries x 4 B of LDS per block).
// Re-measured at 7 waves per SIMD (round 5, profiles/r05/wide_ks/): 20 and 22 entries (both still 7 waves: 10 / 11 KB
// per 2-wave block) within noise of 16 at 4K and on the surface view.
#ifndef PT_WIDE_KS
#define PT_WIDE_KS 16
#endif
constexpr int kWideKS = PT_WIDE_KS;

__device__ __forceinline__ void pix_xy(const PTParams& p, int pid, int* x, int* y) {
  *x = pid % p.W;
  *y = p.y0 + pid / p.W;
}

// ---------------------------------------------------------- ray lists ---
// Compacted ray lists are split into kSeg segments, one per XCD group of
// blocks (blockIdx % kSeg), each with its own counter: a producer block makes
// ONE atomic per list (block-aggregated through LDS), and the 8 counters spread
// those atomics over 8 addresses (one word saturates near 90 atomics/us,
// MI355X_MICROARCH.md "dequeue"). Consumers map a dense index onto the
// segments with the 8 counts (scalar loads).
constexpr int kSeg = 8;

__device__ __forceinline__ int seg_total(const int* __restrict__ counts) {
  int t = 0;
#pragma unroll
  for (int s = 0; s < kSeg; ++s) t += counts[s];
  return t;
}
// A list of `nbins` bins (bin b: items + b * kSeg * cap, counts + b * kSeg), read as one dense range.
__device__ __forceinline__ bool bins_get(const int* __restrict__ items, const int* __restrict__ counts, int nbins,
                                         int cap, int k, int* v) {
  int base = 0;
  for (int b = 0; b < nbins; ++b) {
#pragma unroll
    for (int s = 0; s < kSeg; ++s) {
      const int c = counts[b * kSeg + s];
      if (k < base + c) {
        *v = items[((size_t)b * kSeg + s) * cap + (k - base)];
        return true;
      }
      base += c;
    }
  }
  return false;
}
__device__ __forceinline__ bool seg_get(const int* __restrict__ items, const int* __restrict__ counts, int cap, int k,
                                        int* v) {
  int base = 0;
#pragma unroll
  for (int s = 0; s < kSeg; ++s) {
    const int c = counts[s];
    if (k < base + c) {
      *v = items[s * cap + (k - base)];
      return true;
    }
    base += c;
  }
  return false;
}

// Block-wide append of up to one item to each of the shade lists: the live rays into kLiveBins lists by
// direction octant, the HDR shadow rays, and the point-light shadow rays into kPointBins lists by light index
// (rays of one bin traverse alike, so a trace wave holding one bin diverges less). Every thread of the
// 256-thread block must call it. One atomic per (list, bin) per block.
constexpr int kLists = kLiveBins + 1 + kPointBins;
__device__ __forceinline__ void block_push_shade(bool p_live, int lbin, bool p_h, bool p_p, int bin, int v,
                                                 int* __restrict__ live, int* live_counts, int* __restrict__ shadow,
                                                 int* shadow_counts, int cap, int chunk) {
  __shared__ int wc[kLists][4];
  __shared__ int base[kLists];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long m[kLists];
#pragma unroll
  for (int b = 0; b < kLiveBins; ++b) m[b] = __ballot(p_live && lbin == b);
  m[kLiveBins] = __ballot(p_h);
#pragma unroll
  for (int b = 0; b < kPointBins; ++b) m[kLiveBins + 1 + b] = __ballot(p_p && bin == b);
  if (lane == 0)
#pragma unroll
    for (int l = 0; l < kLists; ++l) wc[l][wv] = __popcll(m[l]);
  __syncthreads();
  const int seg = chunk % kSeg;  // the chunk's segment (wf_list_capacity: at most 256 items per chunk)
  if (threadIdx.x < kLists) {
    const int l = threadIdx.x;
    const int t = (wc[l][0] + wc[l][1]) + (wc[l][2] + wc[l][3]);
    int* c = l < kLiveBins ? live_counts + l * kSeg : shadow_counts + (l - kLiveBins) * kSeg;
    base[l] = t ? atomicAdd(c + seg, t) : 0;
  }
  __syncthreads();
  const unsigned long long lt = (1ull << lane) - 1ull;
  // this lane's masks by constant indices and selects: a per-lane index into m[] put it in scratch (or LDS) memory
  unsigned long long mlive = m[0], mpoint = m[kLiveBins + 1];
#pragma unroll
  for (int j = 1; j < kLiveBins; ++j) mlive = lbin == j ? m[j] : mlive;
#pragma unroll
  for (int j = 1; j < kPointBins; ++j) mpoint = bin == j ? m[kLiveBins + 1 + j] : mpoint;
  if (p_live) {
    int o = base[lbin];
    for (int w = 0; w < wv; ++w) o += wc[lbin][w];
    live[((size_t)lbin * kSeg + seg) * cap + o + __popcll(mlive & lt)] = v;
  }
  if (p_h) {
    int o = base[kLiveBins];
    for (int w = 0; w < wv; ++w) o += wc[kLiveBins][w];
    shadow[seg * cap + o + __popcll(m[kLiveBins] & lt)] = v;
  }
  if (p_p) {
    const int li = kLiveBins + 1 + bin;
    int o = base[li];
    for (int w = 0; w < wv; ++w) o += wc[li][w];
    shadow[(size_t)(1 + bin) * kSeg * cap + seg * cap + o + __popcll(mpoint & lt)] = v;
  }
}

// traversal counters (PTParams::wf.stats, pt_pass_set_trace_stats): a wave sum, one 64-bit atomic per wave.
// Call with every lane of the wave active.
__device__ __forceinline__ void stat_add(const PTParams& p, int k, uint32_t v) {
  if (!p.wf.stats || k >= p.wf.stats_n) return;  // (a buffer of fewer counters: those past its end are skipped)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(p.wf.stats + k, (unsigned long long)v);
}

__device__ __forceinline__ void stat_slots(const PTParams& p, int k, uint32_t v) {  // 64 x the wave maximum
  if (!p.wf.stats || k >= p.wf.stats_n) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(p.wf.stats + k, 64ull * v);
}

// load-balancing probe: accumulate traversal steps per band row (only when requested)
#ifndef PT_STEP_MAX
__device__ __forceinline__ void add_row_cost(const PTParams& p, int local_row, int, uint32_t steps) {
  if (p.wf.row_cost) atomicAdd(p.wf.row_cost + local_row, steps);
}
#else  // investigation build (tools/exp_build.sh stepmax -DPT_STEP_MAX): per-pixel maximum of the steps
__device__ __forceinline__ void add_row_cost(const PTParams& p, int, int pid, uint32_t steps) {
  if (p.wf.row_cost) atomicMax(p.wf.row_cost + pid, steps);
}
#endif

// This lane's traversal stack: its LDS column, and with DEEP (a reference tree deeper than the LDS stack, launched
// only for such trees) the pixel's spill column for the entries beyond it.
template <int STRIDE, int KS, bool DEEP>
__device__ __forceinline__ auto ray_stack(int* lds_column, const PTParams& p, int pid) {
  if constexpr (DEEP) return SpillStack<STRIDE, KS>{lds_column, p.wf.spill + pid, p.wf.spill_stride};
  else return LdsStack<STRIDE>{lds_column};
}

__device__ __forceinline__ v3 primary_dir(const PTParams& p, int x, int y) {
  float pixx = (float)(2 * x + 1) / (float)p.W - 1.0f;
  float pixy = (float)(2 * y + 1) / (float)p.H - 1.0f;
  if (p.aspect_corrected) pixx = pixx * ((float)p.W / (float)p.H);
  const float* m = p.camRot;
  return normalize(mk((m[0] * pixx + m[4] * pixy) + (m[8] * -1.0f + m[12] * 0.0f),
                      (m[1] * pixx + m[5] * pixy) + (m[9] * -1.0f + m[13] * 0.0f),
                      (m[2] * pixx + m[6] * pixy) + (m[10] * -1.0f + m[14] * 0.0f)));
}

// ----------------------------------------------------- stage launchers ---
// The traversal stack a draw's per-lane walks are instantiated for (wf_stack_kind, kernels_wavefront.hip): the LDS
// stack bounds resident waves, so a tree that fits kStackSmall entries gets more of them; kStack otherwise; a
// reference tree deeper than that walks kSpillKS entries in LDS and the rest in the pixel's spill column.
enum class WfStack { kSmall, kFull, kDeep };
// f(KS, DEEP), the kind's template arguments as integral constants: the one place that pairs them.
template <class F>
void with_stack(WfStack k, F&& f) {
  switch (k) {
    case WfStack::kSmall: f(std::integral_constant<int, kStackSmall>{}, std::false_type{}); break;
    case WfStack::kFull: f(std::integral_constant<int, kStack>{}, std::false_type{}); break;
    case WfStack::kDeep: f(std::integral_constant<int, kSpillKS>{}, std::true_type{}); break;
  }
}

// One draw as the stage launchers see it (launch_wavefront fills it in): frame, or sample, b of nb is ps[b].
struct WfDraw {
  const PTParams* ps;
  int nb;
  WfStack stack;
  int N;       // band pixels of one frame
  int cap;     // capacity of a ray-list segment (wf_list_capacity)
  int ntiles;  // the subset's tiles: grid of the primary stage, the bounce-0 shade and the spp resolve
  int gL;      // grid of the list-driven shade (bounces > 0) and finish launches (list_blocks)
};
inline int* wf_live_list(const PTParams& f, int i) { return (i & 1) ? f.wf.list1 : f.wf.list0; }  // bounce i's

// Each launches on the stream given and returns nothing; launch_wavefront reads hipGetLastError() once at its end.
// `f`: the frame's parameters as the launch gets them, with launch_wavefront's per-launch edits applied.
// kernels_wf_primary.hip (the only one that can fail before its end: the bins and the tile sort return their errors)
int launch_primary_stage(const PTParams& f, WfStack stack, int ntiles, hipStream_t s);
// kernels_wf_trace.hip
void launch_primary_coop(const PTParams& f, hipStream_t s);
void launch_closest(const WfDraw& d, int i, hipStream_t s);       // bounce i's rays (i > 0), every frame's
void launch_shadow(const WfDraw& d, int i, hipStream_t s);        // the shadow rays bounce i's shades queued
void launch_shadow_stats(const WfDraw& d, int i, hipStream_t s);  // (traversal counters only)
// kernels_wf_shade.hip
void launch_shade(const WfDraw& d, const PTParams& f, int i, bool fold, bool last, hipStream_t s);
void launch_shade_counted(const WfDraw& d, const PTParams& f, bool fold, bool last, const uint8_t* sample_counts,
                          int sample, hipStream_t s);
void launch_finish(const WfDraw& d, const PTParams& f, int i, bool terminal, hipStream_t s);
void launch_finalize(const WfDraw& d, const PTParams& f, hipStream_t s);
// kernels_spp.hip
void launch_spp_resolve(const SppResolve& rs, const SppAdaptive* ad, int ntiles, hipStream_t s);

}  // namespace ptk

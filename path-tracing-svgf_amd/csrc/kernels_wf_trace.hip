// kernels_wf_trace.hip — the wavefront path tracer's list-driven traversals (kernels_wavefront.hip has the schedule):
// a bounce's closest hits and its shadow verdicts, one ray per lane (wf_trace_closest, wf_trace_shadow) or with lane
// refill (the *_refill kernels), the point-light rays by the lights' triangle bins (wf_shadow_point_bins), and the
// wave-cooperative walks that finish what those hand over (the *_coop kernels, the primary stage's among them).
#include <hip/hip_runtime.h>

#include "glsl_builtins.h"
#include "pt_device.h"
#include "pt_shading.h"
#include "wf_common.h"

using namespace glsl;

namespace ptk {

#ifndef PT_WIDE_SHADOW_SORT
#define PT_WIDE_SHADOW_SORT 0  // shadow rays' 4-wide walk: 1 = nearest child first, 0 = slot order
#endif

// ----------------------------------------------------------- bounce trace ---
template <int KS, bool DEEP>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR wf_trace_closest(PTParams p, const int* __restrict__ list,
                                                                       const int* __restrict__ counts, int cap) {
  __shared__ int stk[KS * kTB];
  const int k = blockIdx.x * kTB + threadIdx.x;
  int pid;
  const bool valid = bins_get(list, counts, kLiveBins, cap, k, &pid);
  if (!p.wf.stats && !valid) return;  // (with counters on, every lane stays for the wave sums)
  uint32_t steps = 0;
  bool rewalk = false, spill = false;
  if (valid) {
    float4 o = ldnt(&p.wf.ray_o[pid]), dd = ldnt(&p.wf.ray_d[pid]);
    float t;
    auto st = ray_stack<kTB, KS, DEEP>(stk + threadIdx.x, p, pid);
    int tri = closest_hit(p.scene, p.closest_tree, st, xyz(o), xyz(dd), p.prune, &t, &steps, PT_INF, &rewalk);
    stnt(&p.wf.hit[pid], make_int2(tri, __float_as_int(t)));
    add_row_cost(p, pid / p.W, pid, steps);
    spill = st.spilled;
  }
  stat_add(p, kStatSpills, spill ? 1u : 0u);
  stat_add(p, kStatBounceRays, valid ? 1u : 0u);
  stat_add(p, kStatBounceVisits, steps);
  stat_slots(p, kStatBounceSlots, steps);
  stat_add(p, kStatTieRewalks, rewalk ? 1u : 0u);
}

// The point-light lists wf_shadow_point_bins decides (bit c: list c): those of the lights with usable bins. The shadow
// walks take the others with the HDR list: a light whose entries overflowed, a non-finite light, a list past the
// lights the bins were built for.
__device__ __forceinline__ uint32_t bins_lists(const PTParams& p) {
  uint32_t m = 0;
  if (p.point_bins)
    for (int c = 0; c < kPointBins; ++c)
      if (c < p.pbins.nl && p.pbins.info[c * kPointBinsInfo] == 0) m |= 1u << c;
  return m;
}

// Shadow rays from the compacted lists wf_shade queued: HDR rays, then point-light rays.
template <int KS, bool WIDE, bool DEEP>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR wf_trace_shadow(PTParams p, const int* __restrict__ list,
                                                                      const int* __restrict__ counts, int cap,
                                                                      int* __restrict__ strag_count) {
  __shared__ int stk[KS * kTB];
  const int k = blockIdx.x * kTB + threadIdx.x;
  const int nh = seg_total(counts);  // HDR list first, then the point-light lists bin by bin
  const bool point = k >= nh;
  int pid = -1;
  bool valid = true;
  if (!point) {
    seg_get(list, counts, cap, k, &pid);
  } else {
    const uint32_t skip = bins_lists(p);  // wf_shadow_point_bins takes these lists
    int r = k - nh;
    valid = false;
#pragma unroll
    for (int b = 0; b < kPointBins; ++b) {
      if ((skip >> b) & 1u) continue;
      const int nb = seg_total(counts + (1 + b) * kSeg);
      if (r < nb) {
        seg_get(list + (size_t)(1 + b) * kSeg * cap, counts + (1 + b) * kSeg, cap, r, &pid);
        valid = true;
        break;
      }
      r -= nb;
    }
  }
  bool deferred = false, spill = false;
  uint32_t steps = 0;
  if (valid) {
    float4 o = ldnt(&p.wf.ray_o[pid]);
    const float4 dir = point ? ldnt(&p.wf.sh_p[pid]) : ldnt(&p.wf.sh_h[pid]);  // point: (direction, distance)
    int occ = WIDE ? anyhit4<kTB, KS>(p.scene, stk + threadIdx.x, xyz(o), xyz(dir), point, dir.w, &steps) : -1;
    if (occ < 0) {  // binary walk (default), or the 4-wide stack overflowed
      auto st = ray_stack<kTB, KS, DEEP>(stk + threadIdx.x, p, pid);
      occ = anyhit2(anyhit_scene(p.scene), st, xyz(o), xyz(dir), point, dir.w, &steps, p.wf.shadow_budget, &deferred);
      spill = st.spilled;
    }
    if (!deferred) (point ? p.wf.occ_p : p.wf.occ_h)[pid] = occ;
    add_row_cost(p, pid / p.W, pid, steps);
  }
  stat_add(p, kStatShadowRays, valid && pid >= 0 ? 1u : 0u);
  stat_add(p, kStatSpills, spill ? 1u : 0u);
  stat_add(p, kStatShadowVisits, steps);
  stat_slots(p, kStatShadowSlots, steps);
  // rays past the step budget go to the cooperative walk (one wave-aggregated append per wave)
  const unsigned long long m = __ballot(deferred);
  if (m) {
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(strag_count, __popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (deferred) p.wf.straggler[base + __popcll(m & ((1ull << lane) - 1ull))] = pid | (point ? (int)0x80000000 : 0);
  }
}

// Dense index k of the shadow lists (HDR list, then the point-light lists bin by bin) -> pixel, kind.
// `skip`: point-light lists left out of the dense range (bins_lists).
__device__ __forceinline__ bool shadow_item(const int* __restrict__ list, const int* __restrict__ counts, int cap,
                                            int nh, int k, int* pid, bool* point, uint32_t skip = 0u) {
  if (k < nh) {
    *point = false;
    return seg_get(list, counts, cap, k, pid);
  }
  *point = true;
  int r = k - nh;
#pragma unroll
  for (int b = 0; b < kPointBins; ++b) {
    if ((skip >> b) & 1u) continue;
    const int nb = seg_total(counts + (1 + b) * kSeg);
    if (r < nb) return seg_get(list + (size_t)(1 + b) * kSeg * cap, counts + (1 + b) * kSeg, cap, r, pid);
    r -= nb;
  }
  return false;
}

// Dense index k over a batch's frames (per-frame totals tot[b]) -> frame b and its local index (wave-uniform data).
__device__ __forceinline__ int batch_frame(const int* tot, int nb, int* k) {
  for (int b = 0; b < nb; ++b) {
    if (*k < tot[b]) return b;
    *k -= tot[b];
  }
  return -1;
}

// Work queue of the refill traversal kernels: the list's dense index range is cut into 8 regions, one per XCD,
// each with its own head word (one returning atomic per grab of kGrab items; a per-XCD head keeps the grabs of
// 256 CUs off one word, MI355X_MICROARCH.md "dequeue"). A wave drains its XCD's region first, then the others;
// regions seen exhausted (a relaxed load of the head) are skipped without an atomic. Wave-uniform.
#ifndef PT_REFILL_QUEUE
#define PT_REFILL_QUEUE 0
#endif
constexpr int kGrab = 64;
struct WaveQueue {
  int* heads;
  int total, xcd;
  unsigned done;  // regions known exhausted
  int next, end;  // current grab [next, end)
  // static chunks (PT_REFILL_QUEUE 0): this wave's virtual wave index, the grid's waves, chunk rounds, big waves
  int vw, gw, R, big;
  __device__ __forceinline__ void chunk() {
    if (vw < big) {
      next = vw * 64 * R;
      end = next + 64 * R;
    } else {
      next = min(big * 64 * R + (vw - big) * 64, total);
      end = min(next + 64, total);
    }
  }
  __device__ __forceinline__ bool grab() {
    if (!PT_REFILL_QUEUE) {  // static chunks: the chunk of virtual wave vw + the grid's waves, if any
      vw += gw;
      chunk();
      return next < end;
    }
    for (int t = 0; t < 8; ++t) {
      const int r = (xcd + t) & 7;
      if ((done >> r) & 1u) continue;
      const int rs = (int)(((long long)total * r) >> 3), re = (int)(((long long)total * (r + 1)) >> 3);
      if (rs + __hip_atomic_load(heads + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= re) {
        done |= 1u << r;
        continue;
      }
      int base = 0;
      if ((threadIdx.x & 63) == 0) base = atomicAdd(heads + r, kGrab);
      base = __builtin_amdgcn_readfirstlane(__shfl(base, 0));
      if (rs + base < re) {
        next = rs + base;
        end = min(next + kGrab, re);
        return true;
      }
      done |= 1u << r;
    }
    return false;
  }
};
// Resident blocks the refill kernels launch with the queue: enough to fill the chip at their occupancy (5 waves/SIMD
// at 86 VGPRs, 2-wave blocks); waves beyond the work exit at their first grab.
constexpr int kRefillBlocks = 256 * 10;
// Static chunks (default), guided: the first PTParams::refill percent of the list goes out in chunks of 64 * R items
// (R = kRefillRounds) to the first waves, the rest in chunks of 64 (one item per lane) to the waves after them, so
// the launch does not end on long refill waves; idle lanes take new items only once at least kRefillMin lanes of
// the wave are idle (a refill stalls the whole wave for the new rays' loads). PT_REFILL_QUEUE=1: the per-XCD work
// queue above instead (measured slower: 109 fps against 148 without refill at 4K).
// Measured at 4K (tools/lib_ab.sh, R = 4, kRefillMin = 16): refill 0 / 50 / 75 / 85 % -> 147.7 / 156.0 / 159.3 /
// 158.7 fps with 4 frames in flight, 117.1 / 116.0 / 110.0 / 108.1 fps serial: the refill waves raise the share of
// busy lanes (shadow 0.42 -> 0.65) but lengthen the launch's tail, which other frames in flight fill.
// The cap on R (end of round 2, same box, K = 4, tools/lib_ab.sh + lib_ab_views.sh): 4 / 8 / 12 / 16 -> 179.6 / 182.6 /
// 183.1 / 182.6 fps at 4K, surface view 53.1 -> 57.2 fps with 12, 1080p unchanged (its lists give R < 4 anyway);
// kRefillMin 8 / 16 / 32: 180.1 / 179.6 / 178.0.
#ifndef PT_REFILL_ROUNDS
#define PT_REFILL_ROUNDS 24  // round 4 (every item refilled, 8 waves per SIMD): 8 / 12 / 16 / 24 / 32 / 48 -> surface
#endif                       // view 73.1 / 74.9 / 75.1 / 75.6 / 75.7 / 75.7 fps, 4K 221-222 throughout
#ifndef PT_REFILL_MIN
#define PT_REFILL_MIN 16
#endif
constexpr int kRefillRounds = PT_REFILL_ROUNDS, kRefillMin = PT_REFILL_MIN;
// Chunk rounds per big wave, from the list length: a big wave lasts about R one-ray waves, which pays only when the
// launch spans several rounds of resident waves anyway (at 1080p the lists are too short: refill there measured
// 367 -> 312 fps with R = 4 everywhere; with R from the length 380 fps at 1080p, 156.6 at 4K). kResidentWaves: 256 CUs
// x 20 waves (86 VGPRs: 5 waves per SIMD). Estimates of 16 / 12 / 8 waves per CU (more rounds per wave) measured
// 182.8 / 181.2 / 177.5 fps against 183.7 at 4K, the surface view unchanged (end of round 2).
// Round 4: the refill kernels now run 8 waves per SIMD (32 per CU); re-measured with that occupancy, 26 per CU gave
// 221.4 / 221.1 fps at 4K against 219.1 / 218.7 for 20 and 220.7 / 220.4 for 32, the surface view within noise
// (profiles/r04/refill_waves_ab.log).
#ifndef PT_RESIDENT_WAVES
#define PT_RESIDENT_WAVES (256 * 26)
#endif
constexpr int kResidentWaves = PT_RESIDENT_WAVES;
#ifndef PT_REFILL_DIV
#define PT_REFILL_DIV 1
#endif
// `waves`: the resident waves the launch may count on (0: the chip, kResidentWaves). A band renderer's launches are
// small and share the chip with the other frames in flight: sized for the whole chip they get one round per wave
// (no refill at all); sized for a share of it they keep refilling.
__device__ __forceinline__ int refill_rounds(int total, int waves) {
  const int r = total / (64 * (waves > 0 ? waves : kResidentWaves) * PT_REFILL_DIV);
  return r < 1 ? 1 : (r > kRefillRounds ? kRefillRounds : r);
}
__device__ __forceinline__ WaveQueue refill_queue(int* heads, int total, int big_pct, int waves) {
  WaveQueue q{heads, total, (int)(blockIdx.x & 7), 0u, 0, 0, 0, 0, 1, 0};
  if (PT_REFILL_QUEUE) {
    q.grab();
  } else {
    q.vw = blockIdx.x * (kTB / 64) + (threadIdx.x >> 6);
    q.gw = gridDim.x * (kTB / 64);
    q.R = refill_rounds(total, waves);
    q.big = q.R > 1 ? (int)((long long)total * big_pct / 100) / (64 * q.R) : 0;  // waves with big chunks
    q.chunk();
    q.done = 0xffu;
  }
  return q;
}
// The static chunks' grid. Until round 6 it had a wave for every 64 items the lists could hold (2 per pixel for the
// shadow rays: 129 600 blocks at 4K) while the frame's lists hold a fraction of that: every wave past the work read
// the list counts and left, ~250 000 of them per shadow launch, at the launch's end. Now at most
// PTSVGF_REFILL_GRID blocks (read once; default 256 CUs x 26 waves x 2 rounds / 2 waves per block; 0 = unbounded),
// and a wave whose chunk is done takes the chunk of its virtual wave + the grid's waves (WaveQueue::grab): the same
// chunks, hence the same per-ray walks and results.
inline int refill_blocks(int items_max, int grid = 0) {
  static const int cap = [] {
    const char* e = getenv("PTSVGF_REFILL_GRID");
    return e ? std::max(0, atoi(e)) : kResidentWaves * 2 / (kTB / 64);
  }();
  const int need = (items_max + kTB - 1) / kTB;
  if (PT_REFILL_QUEUE) return need < kRefillBlocks ? need : kRefillBlocks;
  const int c = grid > 0 ? grid : cap;
  return c > 0 && need > c ? c : need;
}

// Traversal counters only (PTParams::wf.stats set): of one frame's shadow rays of a bounce, those toward point lights
// and those found occluded, from the verdicts.
__global__ void __launch_bounds__(256) wf_shadow_stats(PTParams p, const int* __restrict__ list,
                                                       const int* __restrict__ counts, int cap) {
  const int nh = seg_total(counts);
  int tot = nh;
#pragma unroll
  for (int c = 0; c < kPointBins; ++c) tot += seg_total(counts + (1 + c) * kSeg);
  uint32_t npoint = 0, nocc = 0;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < tot; k += gridDim.x * blockDim.x) {
    int pid;
    bool point;
    if (!shadow_item(list, counts, cap, nh, k, &pid, &point)) continue;
    npoint += point ? 1u : 0u;
    nocc += (point ? p.wf.occ_p : p.wf.occ_h)[pid] != 0 ? 1u : 0u;
  }
  stat_add(p, kStatShadowPoint, npoint);
  stat_add(p, kStatShadowOccluded, nocc);
  // with the bins on, the rays of the lists they do not take were walked: counted as handed over
  if (p.point_bins && blockIdx.x == 0 && threadIdx.x == 0 && kStatShadowPointFallback < p.wf.stats_n) {
    const uint32_t taken = bins_lists(p);
    unsigned long long left = 0;
    for (int c = 0; c < kPointBins; ++c)
      if (!((taken >> c) & 1u)) left += (unsigned long long)seg_total(counts + (1 + c) * kSeg);
    if (left) atomicAdd(p.wf.stats + kStatShadowPointFallback, left);
  }
}

// Shadow rays with lane refill. In wf_trace_shadow a wave lives as long as its longest ray while lanes whose rays
// ended idle: only ~42 % of the lane slots of shadow waves do traversal work on the 4K bench frame (35 % on the
// surface view; trace counters, bench.py "lane_efficiency"). Here waves stay resident and, between two leaf phases
// of their while-while walks, hand list items from the work queue to their idle lanes, so lanes stay busy until the
// queue runs dry. Per ray the walk is anyhit2's (same boxes, same pruning bound, same triangle tests, visit order
// per ray unchanged); any-hit verdicts do not depend on which lane or when.
// With a visit budget (PTParams::wf.shadow_budget) a ray still undecided past it is handed to the wave-cooperative
// walk (wf_shadow_coop) and its lane takes the next item, as in wf_trace_shadow.
// WIDE: the walk runs on the 4-wide form of the any-hit tree (pack_wide: the same candidate triangles); a ray whose
// pushes would overflow the LDS stack goes to the cooperative walk like a ray past the visit budget.
template <int KS, bool DEEP, bool WIDE>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR wf_trace_shadow_refill(PTParams p, ListBatch lb, int cap,
                                                                             int* __restrict__ heads,
                                                                             int* __restrict__ strag_count) {
  __shared__ int stk[KS * kTB];
  const int lane = threadIdx.x & 63;
  int nh[kMaxBatch], tot[kMaxBatch];
  int total = 0;
  const uint32_t skip = bins_lists(p);
  for (int b = 0; b < lb.nb; ++b) {
    nh[b] = seg_total(lb.counts[b]);
    tot[b] = nh[b];
#pragma unroll
    for (int c = 0; c < kPointBins; ++c)  // (the lists wf_shadow_point_bins takes are not walked)
      if (!((skip >> c) & 1u)) tot[b] += seg_total(lb.counts[b] + (1 + c) * kSeg);
    total += tot[b];
  }
  WaveQueue q = refill_queue(heads, total, p.refill, p.refill_waves);
  if (q.next >= q.end) return;
  const SceneDev sc = anyhit_scene(p.scene);
  const unsigned long long below = (1ull << lane) - 1ull;
  auto st = ray_stack<kTB, KS, DEEP>(stk + threadIdx.x, p, 0);
  bool have = false, point = false, spill = false, ovf = false;
  int pid = 0, sp = 0, node = kNone, leaf = kNone;
  v3 S = splat(0.0f), d = splat(0.0f), inv = splat(0.0f);
  float lim = 0.0f, maxd = 0.0f;
  uint32_t nvis = 0, nray = 0, rvis = 0;
  const uint32_t budget = p.wf.shadow_budget;
  while (true) {
    const unsigned long long idle = __ballot(!have);
    if (__popcll(idle) >= (__ballot(have) ? kRefillMin : 1) && (q.next < q.end || q.grab())) {
      // refill: the next items go to the idle lanes in lane order
      int k = q.next + __popcll(idle & below);
      const int fb = k < q.end ? batch_frame(tot, lb.nb, &k) : -1;
      if (!have && fb >= 0 && shadow_item(lb.list[fb], lb.counts[fb], cap, nh[fb], k, &pid, &point, skip)) {
        pid += fb * lb.n;
        rvis = 0;
        const float4 o = ldnt(&p.wf.ray_o[pid]);
        const float4 dir = point ? ldnt(&p.wf.sh_p[pid]) : ldnt(&p.wf.sh_h[pid]);  // point: (direction, distance)
        S = xyz(o);
        d = xyz(dir);
        inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        maxd = dir.w;
        lim = point ? maxd * 1.0002f + 2.0e-4f : __builtin_inff();
        sp = 0;
        node = WIDE ? p.scene.root4 : sc.root_ref;
        leaf = kNone;
        ovf = WIDE && PT_WIDE_SIGNED && !finite3(inv);  // axis-parallel (wide_step's signed planes): the coop walk
        if (node < 0) { leaf = node; node = kNone; }
        if (ovf) node = leaf = kNone;
        if constexpr (DEEP) st = ray_stack<kTB, KS, DEEP>(stk + threadIdx.x, p, pid);
        have = true;
        ++nray;
      }
      q.next = min(q.next + __popcll(idle), q.end);
    }
    if (!__any(have)) break;
    while (node >= 0) {  // anyhit2's descent (only lanes holding a ray have node >= 0)
      nvis += PT_NODE_VISIT;
      ++rvis;
      if constexpr (WIDE) {
        if (!wide_step<KS, PT_WIDE_SHADOW_SORT>(p.scene.bvh4, node, st, sp, S, inv, lim)) {  // stack full: coop walk
          ovf = true;
          node = leaf = kNone;
        }
        if (node < 0 && node != kNone && leaf == kNone) {
          leaf = node;
          node = sp > 0 ? st.get(--sp) : kNone;
        }
        if (!__any(leaf == kNone)) break;
        continue;
      }
      const float4* nd = sc.bvh + 4 * node;
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
      if (node < 0 && node != kNone && leaf == kNone) {
        leaf = node;
        node = sp > 0 ? st.get(--sp) : kNone;
      }
      if (!__any(leaf == kNone)) break;
    }
    bool hit = false;
    while (leaf != kNone) {  // anyhit2's leaf phase
      const int first = ref_leaf_first(leaf), cnt = ref_leaf_count(leaf);
      nvis += (uint32_t)cnt;
      rvis += (uint32_t)cnt;
      if (leaf_scan(sc.tri_geom, first, cnt, S, d, [&](int, float t) {
            return t < PT_INF && (!point || length(sub(add(S, muls(d, t)), S)) < maxd);
          })) {
        hit = true;
        break;
      }
      leaf = kNone;
      if (node < 0 && node != kNone) {
        leaf = node;
        node = sp > 0 ? st.get(--sp) : kNone;
      }
    }
    if (have && !ovf && (hit || (node == kNone && leaf == kNone))) {  // this lane's ray is decided
      (point ? p.wf.occ_p : p.wf.occ_h)[pid] = hit;
      have = false;
      node = leaf = kNone;
      spill = spill || st.spilled;
    }
    // past the budget, or the 4-wide walk's stack full: the cooperative walk decides it
    const bool defer = have && (ovf || (budget && rvis > budget));
    const unsigned long long m = __ballot(defer);
    if (m) {
      int base = 0;
      if (lane == __ffsll((long long)m) - 1) base = atomicAdd(strag_count, __popcll(m));
      base = __shfl(base, __ffsll((long long)m) - 1);
      if (defer) {
        p.wf.straggler[base + __popcll(m & below)] = pid | (point ? (int)0x80000000 : 0);
        have = false;
        node = leaf = kNone;
        spill = spill || st.spilled;
      }
    }
  }
  stat_add(p, kStatShadowRays, nray);
  stat_add(p, kStatSpills, spill ? 1u : 0u);
  stat_add(p, kStatShadowVisits, nvis);
  stat_slots(p, kStatShadowSlots, nvis);
}

// Bounce rays (closest hit) with lane refill, as wf_trace_shadow_refill: per ray closest_hit's walk on the SAH tree
// over the reference leaves (pruned), and for a ray whose best t was met exactly by a second triangle the walk again
// on the reference tree in the reference's order (traverse<0>; the same lane restarts it before taking a new ray).
// Production switches only (closest_tree = prune = 1); the host keeps wf_trace_closest otherwise.
// With a visit budget (PTParams::wf.closest_budget) a ray still walking past it goes to the cooperative closest-hit
// walk (wf_closest_coop) and its lane takes the next item.
// WIDE: the walk runs on the 4-wide form of the SAH tree (pack_wide: the same candidate triangles, so the same
// minimum t); a ray whose best t was met exactly by a second triangle, or whose pushes would overflow the LDS stack,
// goes to the cooperative walk (wf_closest_coop), which re-walks ties on the reference tree.
template <int KS, bool DEEP, bool WIDE>
__global__ void __launch_bounds__(kTB) PT_TRACE_ATTR wf_trace_closest_refill(PTParams p, ListBatch lb, int cap,
                                                                              int* __restrict__ heads,
                                                                              int* __restrict__ strag_count) {
  __shared__ int stk[KS * kTB];
  const int lane = threadIdx.x & 63;
  int tot[kMaxBatch];
  int total = 0;
  for (int b = 0; b < lb.nb; ++b) {
    tot[b] = 0;
#pragma unroll
    for (int c = 0; c < kLiveBins * kSeg; ++c) tot[b] += lb.counts[b][c];
    total += tot[b];
  }
  WaveQueue q = refill_queue(heads, total, p.refill, p.refill_waves);
  if (q.next >= q.end) return;
  const unsigned long long below = (1ull << lane) - 1ull;
  auto st = ray_stack<kTB, KS, DEEP>(stk + threadIdx.x, p, 0);
  bool have = false, rewalk = false, tied = false, spill = false, ovf = false;
  int pid = 0, sp = 0, node = kNone, leaf = kNone, best = -1;
  const float4* tree = p.scene.bvh_any;  // this lane's tree: the SAH tree, or the reference tree for a re-walk
  v3 S = splat(0.0f), d = splat(0.0f), inv = splat(0.0f);
  float tbest = PT_INF;
  uint32_t nvis = 0, nray = 0, nrewalk = 0, rvis = 0;
  const uint32_t budget = p.wf.closest_budget;
  while (true) {
    const unsigned long long idle = __ballot(!have);
    if (__popcll(idle) >= (__ballot(have) ? kRefillMin : 1) && (q.next < q.end || q.grab())) {
      int k = q.next + __popcll(idle & below);
      const int fb = k < q.end ? batch_frame(tot, lb.nb, &k) : -1;
      if (!have && fb >= 0 && bins_get(lb.list[fb], lb.counts[fb], kLiveBins, cap, k, &pid)) {
        pid += fb * lb.n;
        const float4 o = ldnt(&p.wf.ray_o[pid]), dd = ldnt(&p.wf.ray_d[pid]);
        S = xyz(o);
        d = xyz(dd);
        inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        tree = p.scene.bvh_any;
        node = WIDE ? p.scene.root4c : p.scene.root_any;
        rewalk = false;
        ovf = WIDE && PT_WIDE_SIGNED && !finite3(inv);  // axis-parallel (wide_step's signed planes): the coop walk
        tbest = PT_INF;
        best = -1;
        tied = false;
        sp = 0;
        leaf = kNone;
        if (node < 0) { leaf = node; node = kNone; }
        if (ovf) node = leaf = kNone;
        if constexpr (DEEP) st = ray_stack<kTB, KS, DEEP>(stk + threadIdx.x, p, pid);
        have = true;
        rvis = 0;
        ++nray;
      }
      q.next = min(q.next + __popcll(idle), q.end);
    }
    if (!__any(have)) break;
    while (node >= 0) {  // traverse<0>'s descent, pruned by the current best t
      nvis += PT_NODE_VISIT;
      ++rvis;
      if constexpr (WIDE) {
        if (!wide_step<KS, true>(p.scene.bvh4, node, st, sp, S, inv, tbest * 1.0002f + 2.0e-4f)) {
          ovf = true;  // stack full: the cooperative walk
          node = leaf = kNone;
        }
        if (node < 0 && node != kNone && leaf == kNone) {
          leaf = node;
          node = sp > 0 ? st.get(--sp) : kNone;
        }
        if (!__any(leaf == kNone)) break;
        continue;
      }
      const float4* nd = tree + 4 * node;
      const float4 q0 = nd[0], q1 = nd[1], q2 = nd[2], q3 = nd[3];
      float t0l, t0r;
      const float dl = slab(S, inv, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, &t0l);
      const float dr = slab(S, inv, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, &t0r);
      const float lim = tbest * 1.0002f + 2.0e-4f;
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
      if (node < 0 && node != kNone && leaf == kNone) {
        leaf = node;
        node = sp > 0 ? st.get(--sp) : kNone;
      }
      if (!__any(leaf == kNone)) break;
    }
    while (leaf != kNone) {  // traverse<0>'s leaf phase: strict '<' keeps the first triangle at a given t
      const int first = ref_leaf_first(leaf), cnt = ref_leaf_count(leaf);
      nvis += (uint32_t)cnt;
      rvis += (uint32_t)cnt;
      leaf_scan(p.scene.tri_geom, first, cnt, S, d, [&](int i, float t) {
        if (t < tbest) {
          tbest = t;
          best = i;
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
    if (have && !ovf && node == kNone && leaf == kNone && !(WIDE && tied)) {  // this lane's walk is complete
      if (!WIDE && !rewalk && tied) {  // exact tie: walk the ray again on the reference tree, in the reference's order
        rewalk = true;
        ++nrewalk;
        tree = p.scene.bvh;
        node = p.scene.root_ref;
        tbest = PT_INF;
        best = -1;
        tied = false;
        sp = 0;
        if (node < 0) { leaf = node; node = kNone; }
      } else {
        stnt(&p.wf.hit[pid], make_int2(best, __float_as_int(tbest)));
        have = false;
        spill = spill || st.spilled;
      }
    }
    // past the budget, the 4-wide walk's stack full, or (4-wide) an exact tie met: the cooperative walk finishes it
    const bool defer = have && (ovf || (budget && rvis > budget) ||
                                (WIDE && tied && node == kNone && leaf == kNone));
    const unsigned long long m = __ballot(defer);
    if (m) {
      int base = 0;
      if (lane == __ffsll((long long)m) - 1) base = atomicAdd(strag_count, __popcll(m));
      base = __shfl(base, __ffsll((long long)m) - 1);
      if (defer) {
        p.wf.strag_c[base + __popcll(m & below)] = pid;
        have = false;
        node = leaf = kNone;
        spill = spill || st.spilled;
      }
    }
  }
  stat_add(p, kStatBounceRays, nray);
  stat_add(p, kStatSpills, spill ? 1u : 0u);
  stat_add(p, kStatBounceVisits, nvis);
  stat_slots(p, kStatBounceSlots, nvis);
  stat_add(p, kStatTieRewalks, nrewalk);
}

// Point-light shadow rays by the lights' triangle bins (PTParams::pbins, kernels_pointbins.hip) instead of a tree
// walk. A point-light ray is occluded iff some triangle T passes (1) the ray passes the box of T's reference leaf,
// (2) hitTriangle accepts, (3) t < PT_INF and length(d t) < maxd: a verdict that does not depend on which triangles
// are tested besides, or in which order (anyhit2 / wf_trace_shadow_refill evaluate the same three). Every triangle
// that can pass (2) and (3) for a ray toward light l lies in the list of the cell holding -d on l's cube map or in
// l's catch-all list (the build's footprint argument), with `near` no greater than the light's distance from any
// acceptable point, which lies between S and the light: entries with near beyond maxd * 1.0002 + 2e-4 (the walk's
// pruning bound) are skipped, and the lists ascend by near, so the scan stops at the first.
// The build's argument holds for d = normalize(L - S) and maxd = length(L - S) of the light L the bins were built
// around: the kernel recomputes both with wf_shade's expressions and takes only rays whose stored bits match; any
// other ray (a light index past the lists' lights, new light positions the bins have not seen, a non-finite
// direction, an axis-parallel one) goes to the cooperative walk through the straggler list. The lists of a light
// without usable bins, and of a light index past the bins' lights, stay with the shadow walk (bins_lists).
// Lists of light l = list l of each frame; one wave takes 64 consecutive items of one list, so the light is
// wave-uniform. The next entry's triangle is fetched one iteration ahead and the entry after that two ahead: the
// addresses are known up front, so the loads of consecutive entries overlap. (Fetching the triangle only for an
// entry whose near and sub-cell box say it will be tested measured slower, 810 against 681 us per launch: DESIGN.md.)
__global__ void __launch_bounds__(256) wf_shadow_point_bins(PTParams p, ListBatch lb, int cap,
                                                            int* __restrict__ strag_count) {
  const PointBinsDev& pb = p.pbins;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int nw = gridDim.x * 4;
  int vc = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));  // this wave's next chunk of 64
  const int R = pb.R, ncell = pb.ncell();
  uint32_t nvis = 0, nray = 0, nbin = 0, nfall = 0, wvis = 0;
  for (int fb = 0; fb < lb.nb; ++fb) {
    for (int c = 0; c < kPointBins; ++c) {
      const int* counts = lb.counts[fb] + (1 + c) * kSeg;
      const int* list = lb.list[fb] + (size_t)(1 + c) * kSeg * cap;
      const int n = seg_total(counts), nch = (n + 63) >> 6;
      if (c >= pb.nl || pb.info[c * kPointBinsInfo] != 0) continue;  // no usable bins: the shadow walk takes the list
      const int* f = pb.info + (c < pb.nl ? c : 0) * kPointBinsInfo;
      const v3 L = mk(__int_as_float(f[2]), __int_as_float(f[3]), __int_as_float(f[4]));
      const int2* hdr = pb.hdr + (size_t)(c < pb.nl ? c : 0) * (ncell + 1);
      const uint2* ent = pb.ent + (size_t)(c < pb.nl ? c : 0) * pb.cap;
      for (; vc < nch; vc += nw) {
        int pid = 0;
        const bool valid = seg_get(list, counts, cap, vc * 64 + lane, &pid);
        pid += fb * lb.n;
        bool fall = valid;
        int occ = 0;
        uint32_t vis = 0;
        if (valid) {
          const float4 o = ldnt(&p.wf.ray_o[pid]), dir = ldnt(&p.wf.sh_p[pid]);
          const v3 S = xyz(o), d = xyz(dir);
          const float maxd = dir.w;
          const v3 ld = normalize(sub(L, S));  // wf_shade's expressions
          const float dist = length(sub(L, S));
          const v3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
          const bool same = __float_as_uint(ld.x) == __float_as_uint(d.x) && __float_as_uint(ld.y) == __float_as_uint(d.y) &&
                            __float_as_uint(ld.z) == __float_as_uint(d.z) && __float_as_uint(dist) == __float_as_uint(maxd);
          if (same && finite3(inv) && __builtin_isfinite(maxd)) {
            fall = false;
            // the cell of -d: the face of its largest component (x before y before z on a tie), then (x, y) / w
            const v3 v = neg(d);
            const float ax = fabsf(v.x), ay = fabsf(v.y), az = fabsf(v.z);
            const int a = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2);
            const float w = a == 0 ? v.x : (a == 1 ? v.y : v.z);
            const float xf = a == 0 ? v.y : (a == 1 ? v.z : v.x), yf = a == 0 ? v.z : (a == 1 ? v.x : v.y);
            const float aw = fabsf(w);
            const float px = (xf / aw + 1.0f) * 0.5f * (float)R, py = (yf / aw + 1.0f) * 0.5f * (float)R;
            const int cx = min(max((int)floorf(px), 0), R - 1), cy = min(max((int)floorf(py), 0), R - 1);
            // where in its cell, in 1 / 16 of the cell (the floor of the position in 1 / 256, as the build floors its
            // extent): an entry's sub-cell box holds every direction of the cell from which a ray can be found to hit
            // its triangle (the build's extent, rounded outward)
            const uint32_t qx = (uint32_t)min(max((int)floorf((px - (float)cx) * 256.0f), 0), 255) >> 4;
            const uint32_t qy = (uint32_t)min(max((int)floorf((py - (float)cy) * 256.0f), 0), 255) >> 4;
            const int2 h0 = hdr[ncell], h1 = hdr[((2 * a + (w < 0.0f ? 1 : 0)) * R + cy) * R + cx];
            const int n0 = h0.y, ne = n0 + h1.y;
            const float lim = maxd * 1.0002f + 2.0e-4f;
            auto entry = [&](int j) {  // catch-all entries (near 0) first, then the cell's, ascending
              j = min(j, ne - 1);
              return j < n0 ? ent[h0.x + j] : ent[h1.x + (j - n0)];
            };
            // whether the scan tests entry e's triangle: near (its high 16 bits: no greater than the build's) within
            // the ray's bound, and the ray's position inside the sub-cell box
            auto near_ok = [&](uint2 e) { return !(__uint_as_float(e.y << 16) > lim); };
            auto wanted = [&](uint2 e) {
              const uint32_t sb = e.y >> 16;
              return near_ok(e) && !(qx < (sb & 15u) || qx > ((sb >> 4) & 15u) || qy < ((sb >> 8) & 15u) || qy > (sb >> 12));
            };
            if (ne > 0) {
              uint2 e1 = entry(0), e2 = entry(1);
              TriGeom g1 = tri_load(p.scene.tri_geom, (int)e1.x);
              int last_leaf = -1;
              bool last_ok = false;
              for (int i = 0; i < ne; ++i) {
                const uint2 cur = e1;
                const TriGeom tg = g1;
                e1 = e2;
                g1 = tri_load(p.scene.tri_geom, (int)e1.x);
                e2 = entry(i + 2);
                if (!near_ok(cur)) break;  // this one and all after it lie beyond the ray's start
                if (!wanted(cur)) continue;
                float t;
                ++vis;
                if (!tri_test(tg, S, d, &t)) continue;
                if (!(t < PT_INF && length(sub(add(S, muls(d, t)), S)) < maxd)) continue;
                // a hit that counts: the reference tested this triangle only if the ray passes its leaf's box
                const int leaf = p.scene.tri_leaf[cur.x];
                if (leaf != last_leaf) {
                  const float4 lo = p.scene.leaves[2 * leaf], hi = p.scene.leaves[2 * leaf + 1];
                  float t0;
                  last_ok = slab(S, inv, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, &t0) > 0.0f;
                  last_leaf = leaf;
                  ++vis;
                }
                if (last_ok) {
                  occ = 1;
                  break;
                }
              }
            }
            p.wf.occ_p[pid] = (uint8_t)occ;
          }
        }
        nray += valid ? 1u : 0u;
        nbin += valid && !fall ? 1u : 0u;
        nfall += fall ? 1u : 0u;
        nvis += vis;
        uint32_t wm = vis;  // the wave's longest scan
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, o));
        wvis += wm;
        const unsigned long long m = __ballot(fall);
        if (m) {
          int base = 0;
          if (lane == __ffsll((long long)m) - 1) base = atomicAdd(strag_count, __popcll(m));
          base = __shfl(base, __ffsll((long long)m) - 1);
          if (fall) p.wf.straggler[base + __popcll(m & below)] = pid | (int)0x80000000;
        }
      }
      vc -= nch;
    }
  }
  stat_add(p, kStatShadowRays, nray);
  stat_add(p, kStatShadowVisits, nvis);
  if (p.wf.stats && kStatShadowSlots < p.wf.stats_n && lane == 0 && wvis)
    atomicAdd(p.wf.stats + kStatShadowSlots, 64ull * wvis);
  stat_add(p, kStatShadowPointBinned, nbin);
  stat_add(p, kStatShadowPointFallback, nfall);
}

// The shadow rays wf_trace_shadow deferred: one wave per ray walks cooperatively (shadow_coop_walk). A fixed
// grid strides over the straggler list (its length is known only on the device).
constexpr int kCoopWaves = 4;          // waves per block
#ifndef PT_COOP_BLOCKS
#define PT_COOP_BLOCKS 512
#endif
// 2048 waves in flight; 1024 / 2048 blocks measured within noise (profiles/r05/coop_blocks/: 4K 229.1 / 229.6 / 229.5 fps,
// surface view 78.8 / 78.9 / 79.0, one frame at a time 166.3 / 166.4 / 167.1)
constexpr int kCoopBlocks = PT_COOP_BLOCKS;
constexpr int kCoopCap = 1024;         // LDS stack entries per wave
__global__ void __launch_bounds__(64 * kCoopWaves) wf_shadow_coop(PTParams p, const int* __restrict__ strag_count) {
  __shared__ int st[kCoopWaves][kCoopCap];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = *strag_count;
  for (int r = blockIdx.x * kCoopWaves + wv; r < n; r += gridDim.x * kCoopWaves) {
    const int item = p.wf.straggler[r];
    const bool point = item < 0;
    const int pid = item & 0x7fffffff;
    const float4 o = ldnt(&p.wf.ray_o[pid]);
    const float4 dir = point ? ldnt(&p.wf.sh_p[pid]) : ldnt(&p.wf.sh_h[pid]);
    const bool occ = shadow_coop_walk(anyhit_scene(p.scene), st[wv], kCoopCap, xyz(o), xyz(dir), point, dir.w);
    if ((threadIdx.x & 63) == 0) (point ? p.wf.occ_p : p.wf.occ_h)[pid] = occ;
  }
}

// The bounce rays wf_trace_closest_refill deferred: one wave per ray (closest_coop_walk).
__global__ void __launch_bounds__(64 * kCoopWaves) wf_closest_coop(PTParams p, const int* __restrict__ strag_count) {
  __shared__ int st[kCoopWaves][kCoopCap];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = *strag_count;
  uint32_t nrewalk = 0;
  for (int r = blockIdx.x * kCoopWaves + wv; r < n; r += gridDim.x * kCoopWaves) {
    const int pid = p.wf.strag_c[r];
    const float4 o = ldnt(&p.wf.ray_o[pid]), dd = ldnt(&p.wf.ray_d[pid]);
    float t;
    bool rw;
    const int tri = closest_coop_walk(p.scene, st[wv], kCoopCap, xyz(o), xyz(dd), &t, &rw);
    if ((threadIdx.x & 63) == 0) {
      stnt(&p.wf.hit[pid], make_int2(tri, __float_as_int(t)));
      nrewalk += rw ? 1u : 0u;
    }
  }
  stat_add(p, kStatTieRewalks, nrewalk);
}

// The primary rays wf_primary_raster flagged (an exact-t tie, or no hit below the G-buffer bound): one wave per ray
// (closest_coop_walk: closest_hit's answer, unbounded, ties walked on the reference tree).
// After a pair-list overflow (leaf_bins.ctr[2]: the rasteriser skipped the frame) every pixel of the subset's tiles is
// walked here the same way, and the tile counts the skipped scatter left are cleared; until round 6 a wf_primary
// launch of one block per tile did that, and every frame paid for its launch.
__global__ void __launch_bounds__(64 * kCoopWaves) wf_primary_coop(PTParams p, const int* __restrict__ strag_count) {
  __shared__ int st[kCoopWaves][kCoopCap];
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (p.leaf_bins.ctr && p.leaf_bins.ctr[2]) {
    const int ntx = (p.W + 15) / 16, all = ntx * ((p.y1 - p.y0 + 15) / 16);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < all; j += gridDim.x * blockDim.x)
      p.leaf_bins.tile_count[j] = 0;
    const int nsub = all / p.tile_stride + (all % p.tile_stride > p.tile_offset ? 1 : 0);  // the subset's tiles
    uint32_t nrays = 0, nrewalk = 0;
    for (int r = blockIdx.x * kCoopWaves + wv; r < nsub * 256; r += gridDim.x * kCoopWaves) {
      const int gt = (r >> 8) * p.tile_stride + p.tile_offset, i = r & 255;
      const int x = (gt % ntx) * 16 + (i & 15), y = p.y0 + (gt / ntx) * 16 + (i >> 4);
      if (x >= p.W || y >= p.y1) continue;  // wave-uniform
      const int pid = (y - p.y0) * p.W + x;
      float t;
      bool rw;
      const int tri = closest_coop_walk(p.scene, st[wv], kCoopCap, mk(p.eye[0], p.eye[1], p.eye[2]),
                                        primary_dir(p, x, y), &t, &rw);
      if ((threadIdx.x & 63) == 0) {
        stnt(&p.wf.hit[pid], make_int2(tri, __float_as_int(t)));
        nrewalk += rw ? 1u : 0u;
        ++nrays;
      }
    }
    stat_add(p, kStatPrimRays, nrays);
    stat_add(p, kStatTieRewalks, nrewalk);
    return;
  }
  const int n = *strag_count;
  uint32_t nrewalk = 0, nretry = 0;
  for (int r = blockIdx.x * kCoopWaves + wv; r < n; r += gridDim.x * kCoopWaves) {
    const int pid = p.wf.strag_c[r];
    const int x = pid % p.W, y = p.y0 + pid / p.W;
    const v3 S = mk(p.eye[0], p.eye[1], p.eye[2]);
    float t;
    bool rw;
    const int tri = closest_coop_walk(p.scene, st[wv], kCoopCap, S, primary_dir(p, x, y), &t, &rw);
    if ((threadIdx.x & 63) == 0) {
      stnt(&p.wf.hit[pid], make_int2(tri, __float_as_int(t)));
      nrewalk += rw ? 1u : 0u;
      ++nretry;
    }
  }
  stat_add(p, kStatTieRewalks, nrewalk);
  stat_add(p, kStatPrimRetries, nretry);
}


// ------------------------------------------------------- the stage's launches ---
// nb > 1 (a batch's frames, an spp draw's samples): ONE launch of a lane-refill kernel takes every frame's lists of a
// bounce, with frame 0's parameters, work-queue heads and straggler list; the one-ray-per-lane kernels run per frame.
void launch_primary_coop(const PTParams& f, hipStream_t s) {
  hipLaunchKernelGGL(wf_primary_coop, dim3(kCoopBlocks), dim3(64 * kCoopWaves), 0, s, f,
                     (const int*)(f.wf.counters + kCtrStragC));
}

// the refill walks on the 4-wide trees (a deep tree keeps the binary walks, whose stack can spill)
static bool wide_walk(const WfDraw& d) { return d.stack != WfStack::kDeep && d.ps[0].refill && d.ps[0].scene.bvh4; }

void launch_closest(const WfDraw& d, int i, hipStream_t s) {
  const PTParams& p = d.ps[0];
  if (!(p.refill && p.closest_tree && p.prune && p.scene.bvh_any)) {
    for (int b = 0; b < d.nb; ++b)
      with_stack(d.stack, [&](auto ks, auto deep) {
        hipLaunchKernelGGL((wf_trace_closest<ks(), deep()>), dim3((d.N + kTB - 1) / kTB), dim3(kTB), 0, s, d.ps[b],
                           (const int*)wf_live_list(d.ps[b], i + 1),
                           (const int*)(d.ps[b].wf.counters + kWfCtr * (i - 1)), d.cap);
      });
    return;
  }
  ListBatch lb{d.nb, d.N, {}, {}};
  for (int b = 0; b < d.nb; ++b) {
    lb.list[b] = wf_live_list(d.ps[b], i + 1);
    lb.counts[b] = d.ps[b].wf.counters + kWfCtr * (i - 1);
  }
  int* heads = p.wf.counters + kWfCtr * i + kCtrQClosest;
  int* strag = p.wf.counters + kWfCtr * i + kCtrStragC;
  const dim3 grid(refill_blocks(d.nb * d.N, p.refill_grid));
  const bool wide = wide_walk(d);
  if (wide)
    hipLaunchKernelGGL((wf_trace_closest_refill<kWideKS, false, true>), grid, dim3(kTB), 0, s, p, lb, d.cap, heads, strag);
  else
    with_stack(d.stack, [&](auto ks, auto deep) {
      hipLaunchKernelGGL((wf_trace_closest_refill<ks(), deep(), false>), grid, dim3(kTB), 0, s, p, lb, d.cap, heads, strag);
    });
  if (p.wf.closest_budget || wide)  // (4-wide: ties and stack overflows go there too)
    hipLaunchKernelGGL(wf_closest_coop, dim3(kCoopBlocks), dim3(64 * kCoopWaves), 0, s, p, (const int*)strag);
}

void launch_shadow(const WfDraw& d, int i, hipStream_t s) {
  const PTParams& p = d.ps[0];
  // point-light shadow rays by the lights' triangle bins (every frame of a batch agrees: capi_draw_pt.hip); deep trees keep
  // the walk
  const bool pbins = d.stack != WfStack::kDeep && p.point_bins;
  // its grid: a wave per 64 point-light rays (at most one per pixel), at most the resident waves (8 per SIMD), each
  // striding over the lists' chunks
  auto point_blocks = [](int pixels) { return std::max(1, std::min((pixels + 255) / 256, 256 * 8)); };
  ListBatch lb{d.nb, d.N, {}, {}};
  for (int b = 0; b < d.nb; ++b) {
    lb.list[b] = d.ps[b].wf.shadow_list;
    lb.counts[b] = d.ps[b].wf.counters + kWfCtr * i + kCtrHdr;
  }
  if (!p.refill) {
    for (int b = 0; b < d.nb; ++b) {
      const PTParams& f = d.ps[b];
      const ListBatch one{1, d.N, {lb.list[b]}, {lb.counts[b]}};
      int* strag = f.wf.counters + kWfCtr * i + kCtrStrag;
      if (pbins) hipLaunchKernelGGL(wf_shadow_point_bins, dim3(point_blocks(d.N)), dim3(256), 0, s, f, one, d.cap, strag);
      with_stack(d.stack, [&](auto ks, auto deep) {
        const auto kernel = f.scene.bvh4 ? wf_trace_shadow<ks(), true, deep()> : wf_trace_shadow<ks(), false, deep()>;
        hipLaunchKernelGGL(kernel, dim3((2 * d.N + kTB - 1) / kTB), dim3(kTB), 0, s, f, one.list[0], one.counts[0],
                           d.cap, strag);
      });
      if (f.wf.shadow_budget || pbins)
        hipLaunchKernelGGL(wf_shadow_coop, dim3(kCoopBlocks), dim3(64 * kCoopWaves), 0, s, f, (const int*)strag);
    }
    return;
  }
  int* heads = p.wf.counters + kWfCtr * i + kCtrQShadow;
  int* strag = p.wf.counters + kWfCtr * i + kCtrStrag;  // shadow rays handed to the cooperative walk
  if (pbins)  // the point-light rays by the lights' triangle bins; the walk below takes the other lists
    hipLaunchKernelGGL(wf_shadow_point_bins, dim3(point_blocks(d.nb * d.N)), dim3(256), 0, s, p, lb, d.cap, strag);
  const dim3 grid(refill_blocks(2 * d.nb * d.N, p.refill_grid));
  const bool wide = wide_walk(d);
  if (wide)
    hipLaunchKernelGGL((wf_trace_shadow_refill<kWideKS, false, true>), grid, dim3(kTB), 0, s, p, lb, d.cap, heads, strag);
  else
    with_stack(d.stack, [&](auto ks, auto deep) {
      hipLaunchKernelGGL((wf_trace_shadow_refill<ks(), deep(), false>), grid, dim3(kTB), 0, s, p, lb, d.cap, heads, strag);
    });
  if (p.wf.shadow_budget || wide || pbins)  // (the bins hand the rays they cannot take to it)
    hipLaunchKernelGGL(wf_shadow_coop, dim3(kCoopBlocks), dim3(64 * kCoopWaves), 0, s, p, (const int*)strag);
}

void launch_shadow_stats(const WfDraw& d, int i, hipStream_t s) {  // (traversal counters only)
  for (int b = 0; b < d.nb; ++b)
    hipLaunchKernelGGL(wf_shadow_stats, dim3((d.N + 255) / 256), dim3(256), 0, s, d.ps[b],
                       (const int*)d.ps[b].wf.shadow_list, (const int*)(d.ps[b].wf.counters + kWfCtr * i + kCtrHdr),
                       d.cap);
}

}  // namespace ptk

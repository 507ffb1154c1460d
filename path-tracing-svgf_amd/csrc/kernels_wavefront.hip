// kernels_wavefront.hip — the production path tracer: path_tracing.frag's main()
// (:1056-1128) split into stages so that BVH traversal runs in small,
// high-occupancy kernels and shading runs without a traversal stack:
//
//   per bounce i:  trace_closest -> shade -> trace_shadow (HDR + point light) -> finish
//   then          finalize (clamp / NaN / accumulate / store)
//
// With shade_fold (the default) a path's colour is stored where the path ends, in the shade or the last bounce's
// finish, and a bounce's finish runs at the top of the next bounce's shade: no finalize, one finish per frame.
//
// Rays that stay alive are compacted into a list with one wave-ballot atomic per
// wave, so traversal waves carry only live rays (58 % of the 4K frame is sky).
// The arithmetic per pixel is exactly the megakernel's (and the reference's):
// shade() evaluates both light contributions as if unoccluded, finish() applies
// the shadow verdicts with the reference's selection (hdriLight :934-937 zeroes
// pdf and value; calculatePointLight :905-909 zeroes the value only), so outputs
// stay bit-identical to the CPU oracle. RNG consumption order per pixel is
// unchanged: AA x2, then per bounce xi_3, r1, r2, light pick.
#include <hip/hip_runtime.h>

#include "glsl_builtins.h"
#include "pt_device.h"
#include "pt_shading.h"
#include "wf_common.h"

using namespace glsl;

namespace ptk {

// PT_WIDE_SIGNED's child test (wide_step) takes t1 > 0 as t1 >= the least f32 subnormal: compiled with this file's
// flags, max(x, least subnormal) must stay above 0 for x = 0 (x comes from memory, so nothing folds at compile time)
__global__ void __launch_bounds__(64) subnormal_probe_kernel(const float* zero, int* out) {
  if (threadIdx.x == 0) out[0] = fmaxf(zero[0], __builtin_bit_cast(float, 1u)) > 0.0f ? 1 : 0;
}
int subnormal_probe(hipStream_t s) {
  void* buf = nullptr;
  if (hipMalloc(&buf, 8) != hipSuccess) return -1;
  int host = -1;
  bool ok = hipMemsetAsync(buf, 0, 8, s) == hipSuccess;
  if (ok) hipLaunchKernelGGL(subnormal_probe_kernel, dim3(1), dim3(64), 0, s, (const float*)buf, (int*)buf + 1);
  ok = ok && hipGetLastError() == hipSuccess &&
       hipMemcpyAsync(&host, (int*)buf + 1, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess &&
       hipStreamSynchronize(s) == hipSuccess;
  (void)hipFree(buf);
  return ok ? host : -1;
}

// A producer block appends at most 256 items to the segment blockIdx % kSeg; the most blocks
// an appending launch has is the larger of the per-pixel grid and the bounce-0 tile grid.
int wf_list_capacity(int W, int rows) {
  const int blocks = std::max((W * rows + 255) / 256, ((W + 15) / 16) * ((rows + 15) / 16));
  return (blocks + kSeg - 1) / kSeg * 256;
}

// Tiles of the subset k * stride + offset among the band's 16 x 16 tiles (PTParams::tile_stride).
int wf_subset_tiles(int W, int rows, int stride, int offset) {
  const int n = ((W + 15) / 16) * ((rows + 15) / 16);
  if (stride < 1 || offset < 0 || offset >= stride) return -1;
  return offset < n ? (n - offset + stride - 1) / stride : 0;
}

// Grid of the list-driven shade (bounces > 0) and finish launches: until round 6 one block per 256 pixels (32 400 at
// 4K), most of them past the list's end, reading its counts and leaving. Now at most PTSVGF_LIST_BLOCKS (read once;
// default 2 048, a multiple of kSeg; 0 = one per 256 pixels) striding over 256-item chunks.
static int list_blocks(int n_items_max, int grid = 0) {
  static const int cap = [] {
    const char* e = getenv("PTSVGF_LIST_BLOCKS");
    const int v = e ? std::max(0, atoi(e)) : 2048;
    return (v + kSeg - 1) / kSeg * kSeg;
  }();
  const int need = (n_items_max + 255) / 256;
  const int c = grid > 0 ? (grid + kSeg - 1) / kSeg * kSeg : cap;
  return c > 0 && need > c ? c : need;
}

// The traversal stack of a draw (WfStack, wf_common.h), from its first frame: the frames of a batch share a scene.
static WfStack wf_stack_kind(const PTParams& p) {
  if (p.wf.spill) return WfStack::kDeep;
  return p.stack_need <= kStackSmall ? WfStack::kSmall : WfStack::kFull;
}

// ---- the per-launch edits of a frame's parameters (kernel bodies know nothing of them) ----
// The primary hit lives in wf.hit0, not wf.hit: the stage's launches and the bounce-0 shades below get a copy of the
// frame's parameters whose `hit` is that plane (kernel bodies unchanged), and the bounce-1 trace overwrites wf.hit
// alone. Nothing the stage computes depends on frameCounter (the jitter of :1060-1062 is never applied), so with
// reuse_primary (the caller compared the key of everything the stage reads, static_key.h) the stage is skipped: hit0
// and the tile order of the last stage that ran (tile_sort_kernel cleared `cost` then, and nothing outside the stage
// adds to it) are what this stage would write. hit0 is written and read only by draws of its own pass, like every
// other array of the pass's wavefront state: whatever orders two draws of a pass over ray_o or the lists (one
// stream, or the caller's events before a slot is reused) orders the stage's writes before every later draw's reads.
static PTParams primary_params(const PTParams& frame) {
  PTParams f = frame;
  f.wf.hit = f.wf.hit0;
  return f;
}
// Bounce i's shade of frame (or sample) b. `single`: one frame, one sample, no deep tree, folded shades, which is
// what the verdict cache and the keep mode ask for (the caller bypasses both otherwise: point_cache_mode_for and
// first_hit_mode_for, capi_static.hip). `spp`: the frames are the samples of an spp draw.
static PTParams shade_params(const WfDraw& d, int b, int i, bool fold, bool single, bool spp) {
  PTParams f = d.ps[b];
  // The bounce-0 point-light verdict cache (point_cache.h): the mode goes to the bounce-0 shade, which looks verdicts
  // up and marks the rays it queues, and to the one launch that consumes bounce 0's verdicts (finish_apply), which
  // writes them back: the bounce-1 shade, or at depth 1 bounce 0's wf_finish (finish_params). Every other launch gets
  // kPcOff.
  f.point_cache = single && (i == 0 || (i == 1 && fold)) ? d.ps[0].point_cache : (int)kPcOff;
  // keep mode is the bounce-0 shade's alone; the first-hit planes go null with it, so the hit pixels' stores into them
  // fall away as a later sample's do
  f.busy = i == 0 && single ? d.ps[0].busy : nullptr;
  if (f.busy) f.emission = f.albedo = Plane{};
  if (i == 0) {
    // The bounce-0 shade reads the primary hit plane (above); sample b of an spp draw reads sample 0's (and, the
    // samples being copies of one pass, its tiles.perm_next). No launch of this draw after the stage writes hit0:
    // the bounce-1 trace writes wf.hit. The first-hit planes are sample 0's alone: the folded shade skips the
    // stores of null planes; the unfolded one (shade_fold = 0, A/B) has no such branch and stores into the
    // sample's own colour plane, every texel of which its wf_finalize writes afterwards on `s`.
    f.wf.hit = d.ps[spp ? 0 : b].wf.hit0;
    if (spp && b > 0) f.emission = f.albedo = fold ? Plane{} : d.ps[b].color;
  }
  return f;
}
// Bounce i's finish of a frame: bounce 0's consumes the verdicts the cache waits for (shade_params).
static PTParams finish_params(const PTParams& frame, int i, bool single) {
  PTParams f = frame;
  f.point_cache = i == 0 && single ? frame.point_cache : (int)kPcOff;
  return f;
}

// Launch order of one frame. With a WfFork (uniform trace_fork) the closest-hit trace of bounce 1 (it needs only the
// rays and live list the bounce-0 shade wrote) runs beside the bounce-0 shadow trace and finish on the side stream;
// the join comes before the bounce-1 shade, which reuses the shadow list and reads the finished throughput. The two
// traversal launches then fill each other's tails. Without `fk` the launches are serial. (With shade_fold the
// bounce-0 finish is part of the bounce-1 shade and the join follows the shadow walk.)
// nb > 1: a batch of frames (pt_pass_draw_batch) — per-frame launches for the primaries, shades and finishes, ONE
// launch per bounce for the list-driven traversals of every frame's rays (lane-refill kernels; the one-ray-per-lane
// kernels run per frame). Frame b's wavefront state lies at pid offset b * N of ps[0]'s, its counters at
// ps[0].wf.counters + b * kWfCounters; the batched launches use frame 0's work-queue heads and straggler lists.
// rs (an spp draw, launch_pathtrace_wavefront_spp): the nb "frames" are the samples of one frame. The primary stage
// runs for sample 0 alone and every sample's bounce-0 shade reads sample 0's hit; each path's end writes its sample's
// plane (ps[s].color) and wf_spp_resolve folds the planes into rs->color after the last finish.
// ad (with rs; DESIGN.md "Adaptive sample counts"): with ad->counts the bounce-0 shades of samples >= 1 are
// wf_shade_counted, and with either plane the resolve is wf_spp_resolve_adaptive; every other launch is unchanged.
static int launch_wavefront(const PTParams* ps, int nb, hipStream_t s, const WfFork* fk,
                            const SppResolve* rs = nullptr, const SppAdaptive* ad = nullptr,
                            bool reuse_primary = false) {
  const PTParams& p = ps[0];
  const int rows = p.y1 - p.y0;
  if (rows <= 0) return 0;
  const int N = p.W * rows;
  const int cap = wf_list_capacity(p.W, rows);  // per segment; the host sized the lists with the same function
  hipError_t e = hipMemsetAsync(p.wf.counters, 0, (size_t)nb * kWfCounters * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  const int ntiles = wf_subset_tiles(p.W, rows, p.tile_stride, p.tile_offset);
  if (ntiles <= 0) return 0;
  const WfDraw d{ps, nb, wf_stack_kind(p), N, cap, ntiles, list_blocks(N, p.list_grid)};
  const bool deep = d.stack == WfStack::kDeep;
  // deep trees keep one stream: both walks would use the pixel's spill columns
  const bool split = fk && !deep && p.max_depth > 1;
  // paths end in place (shade_fold; a path of no bounce has no shade to end in: wf_finalize writes its colour)
  const bool fold = p.shade_fold && p.max_depth > 0;
  const bool single = nb == 1 && !rs && !deep && fold;  // (shade_params)
  const bool counted = rs && ad && ad->counts;          // the bounce-0 shades of samples >= 1 skip pixels

  for (int b = 0; b < (rs ? 1 : nb) && !reuse_primary; ++b) {  // (the primary ray does not depend on the sample)
    const int rc = launch_primary_stage(primary_params(ps[b]), d.stack, ntiles, s);
    if (rc) return rc;
  }
  for (int i = 0; i < p.max_depth; ++i) {
    const bool last = i + 1 == p.max_depth;
    if (i > 0) launch_closest(d, i, s);
    if (i == 1 && split) {
      const hipError_t e = hipStreamWaitEvent(s, fk->join, 0);
      if (e != hipSuccess) return (int)e;
    }
    for (int b = 0; b < nb; ++b) {
      const PTParams f = shade_params(d, b, i, fold, single, rs != nullptr);
      if (counted && i == 0 && b > 0) launch_shade_counted(d, f, fold, last, ad->counts, b, s);
      else launch_shade(d, f, i, fold, last, s);
    }
    hipStream_t ss = s;  // the shadow walk's and finish's stream
    if (i == 0 && split) {
      hipError_t e = hipEventRecord(fk->fork, s);
      if (e == hipSuccess) e = hipStreamWaitEvent(fk->side, fk->fork, 0);
      if (e != hipSuccess) return (int)e;
      ss = fk->side;
    }
    launch_shadow(d, i, ss);
    if (p.wf.stats) launch_shadow_stats(d, i, ss);
    // folded: bounce i's verdicts are applied at the top of the bounce-(i + 1) shade; the last bounce's finish ends
    // the paths still alive
    for (int b = 0; b < nb && !(fold && !last); ++b) launch_finish(d, finish_params(ps[b], i, single), i, fold, ss);
    if (i == 0 && split) {
      const hipError_t e = hipEventRecord(fk->join, ss);
      if (e != hipSuccess) return (int)e;
    }
  }
  if (!fold)
    for (int b = 0; b < nb; ++b) launch_finalize(d, ps[b], s);
  // every sample's colour is written by now on `s` (the last bounce's finish or wf_finalize; a trace_fork joined
  // before the bounce-1 shade)
  if (rs) launch_spp_resolve(*rs, ad, ntiles, s);
  return (int)hipGetLastError();
}

int launch_pathtrace_wavefront(const PTParams& p, hipStream_t s, const WfFork* fk, bool reuse_primary) {
  return launch_wavefront(&p, 1, s, fk, nullptr, nullptr, reuse_primary);
}

int launch_pathtrace_wavefront_batch(const PTParams* ps, int nb, hipStream_t s, const WfFork* fk) {
  if (nb < 1 || nb > kMaxBatch) return (int)hipErrorInvalidValue;
  return launch_wavefront(ps, nb, s, fk);
}

int launch_pathtrace_wavefront_spp(const PTParams* ps, const SppResolve& rs, hipStream_t s, const WfFork* fk,
                                   const SppAdaptive* ad, bool reuse_primary) {
  if (rs.n < 2 || rs.n > kMaxBatch) return (int)hipErrorInvalidValue;
  if (ad && !ad->counts && !ad->stats && !ad->moments) ad = nullptr;
  return launch_wavefront(ps, rs.n, s, fk, &rs, ad, reuse_primary);
}

}  // namespace ptk

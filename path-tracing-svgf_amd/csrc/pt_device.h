// pt_device.h — parameter blocks and HBM layouts shared by the C-ABI layer
// (capi.hip, capi_draw_*.hip) and the kernels. Everything here is plain data; no torch types.
//
// HBM layout (DESIGN.md "Data layout"):
//  * frame planes: RGBA32F (float4) row-major, one plane per GL texture, holding
//    global rows [row0, row0+rows) of a W x H frame (row0 = 0, rows = H on 1 GPU);
//  * optional compact side plane `aux` (float, 4 B/px) next to a plane whose only
//    consumer-visible channel is .y (the depth fwidth of gNormalDepthFwidth):
//    written by the G-buffer kernel, read by the a-trous kernel instead of the
//    16-B texel (52 B/px/iteration instead of 64). Its magnitude is .y (always
//    >= 0, or a NaN with the sign clear); its SIGN BIT flags zCenter == 1 (the
//    pixel's gNormalAndLinearZ.w, background sentinel), so the a-trous skips
//    reading the normal/depth texel of pixels it only copies;
//  * scene: tri_geom  4 x float4 / triangle  (p1,N.p1)(p2,-)(p3,-)(N,-)  intersection
//           tri_shade 9 x float4 / triangle  normals, material, uv, objIndex  closest hit only
//           bvh       4 x float4 / interior node: both children's AABBs + child refs
//    (children refs >= 0: interior index; < 0: leaf = -(first*16 + count) - 1);
//           bvh4      7 x float4 / node: the 4-wide collapse for any-hit (shadow) rays,
//                     lo.x[4] hi.x[4] lo.y[4] hi.y[4] lo.z[4] hi.z[4] refs[4];
//  * HDR map / importance cache: float4 per texel (RGB32F padded), row-major.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "point_cache.h"
#include "pt_layout.h"  // kStack, kWideStride, kNoneRef and the PT_KSTACK / PT_WIDE_STRIDE / PT_WIDE_ORDER defaults

namespace ptk {

// PT_WIDE_SIGNED = 1 (default since round 5): the 4-wide walks pick each child's near / far planes by the ray's
// direction signs (which float4 is loaded) instead of slab's 6 min / max per child (pt_shading.h wide_step): 99 -> 92
// VALU per shadow node step in the ISA. Same bits. With the traversal kernels at 7 waves per SIMD (wf_common.h
// PT_TRACE_WAVES_PER_EU), same box, two alternating repetitions (profiles/r05/wide_signed/): 4K 222.5 / 222.4 ->
// 225.3 / 225.2 fps, surface view 73.9 / 74.0 -> 78.1 / 78.0 (at 8 waves it spills 40-44 B per lane: 223.0, 77.1;
// at 6: 223.0, 76.6)
#ifndef PT_WIDE_SIGNED
#define PT_WIDE_SIGNED 1
#endif
// Traversal counters: a node visit counts PT_NODE_VISIT (1; a diagnostic build with 0 counts triangle tests only)
#ifndef PT_NODE_VISIT
#define PT_NODE_VISIT 1
#endif
constexpr int kStackSmall = 24;    // smaller LDS stack (more resident waves) for trees that fit it
// LDS entries of the spilling traversal stack (SpillStack): a tree deeper than this walks kSpillKS entries in LDS and
// the rest in global memory. Default kStack (spill only beyond the 32-entry stack); PT_SPILL_KS < kStackSmall trades
// rare global spills for more resident waves (A/B).
#ifndef PT_SPILL_KS
#define PT_SPILL_KS PT_KSTACK
#endif
constexpr int kSpillKS = PT_SPILL_KS;
constexpr int kBlock = 256;      // threads per block for per-pixel kernels
constexpr int kPointBins = 4;     // point-light shadow lists, one per light index mod 4 (coherent waves)
constexpr int kLiveBins = 1;  // live-ray lists (by direction octant, 8 of them, measured 4 % slower: one list)
// wavefront list counters per bounce (8 segments each): live bins, HDR shadow, point bins, straggler count
constexpr int kCtrHdr = 8 * kLiveBins, kCtrPoint = kCtrHdr + 8, kCtrStrag = kCtrPoint + 8 * kPointBins;
// per-XCD work-queue heads of the refill traversal kernels launched in bounce i: shadow rays, closest-hit rays
constexpr int kCtrQShadow = kCtrStrag + 1, kCtrQClosest = kCtrQShadow + 8, kCtrStragC = kCtrQClosest + 8;
// bounce 0's base only: bounce-0 point-light verdicts the verdict cache served, in 8 words by block (point_cache.h;
// those queued as rays are the kCtrPoint counts)
constexpr int kCtrPcServed = kCtrStragC + 1;
constexpr int kWfCtr = (kCtrPcServed + 8 + 63) / 64 * 64;
constexpr int kWfCounters = 4 * kWfCtr;  // 4 bounces  // "no node" (leaf refs are >= -(2^31 - 1))

struct Plane {          // banded RGBA32F plane
  float4* p;
  const float* aux;     // optional compact channel (see above), may be null
  int W;                // row width (pixels)
  int row0;             // global row of local row 0
  int rows;             // allocated rows
};

// Cost-ordered dispatch of a tiled traversal launch (kernels_sched.hip). The
// slowest waves of a traversal launch (rays through dense geometry: ~1000 node and
// triangle visits at ~0.7 us each) set its tail; started last in raster order they
// finish long after the bulk. Each launch records every tile's slowest wave and the
// next launch dispatches tiles in descending order of that cost, so the long waves
// start first and overlap the bulk. Dispatch order only: results are unchanged.
struct TileSched {
  const int* perm;      // launch slot -> tile index, may be null (raster order)
  int* perm_next;       // where the order from this launch's costs is written (the same buffer as perm)
  uint32_t* cost;       // per tile: max traversal steps of its waves in this launch, may be null
  int ntiles;
};

struct Tex {            // non-banded float4 image (HDR map / cache)
  const float4* p;
  int W, H;
};

struct SceneDev {
  const float4* tri_geom;
  const float4* tri_shade;
  const float4* bvh;
  int root_ref;         // >= 0 interior node index, < 0 leaf ref
  const float4* bvh4;   // 4-wide collapse of bvh for any-hit rays (7 x float4 / node), may be null
  int root4;
  int root4c;           // root of the closest-hit walks' 4-wide tree in bvh4 (= root4 unless PTSVGF_WIDE_COLLAPSE 2 / 3)
  const float4* bvh_any;  // binary any-hit tree over bvh's leaves (host_trees.cpp build_anyhit_tree), may be null
  int root_any;
  int ntris;
  const float* lights;  // 6 floats per light (PointLight: position, radiance)
  int nlights_buf;      // lights actually present in the buffer
  // material_array (main.cpp:184-205): RGBA8 2-D array, layer-major rows of tex_w texels, may be null
  const uint32_t* texarr;
  int tex_w, tex_h, tex_layers;
  int use_normal_map;   // uniform use_normal_map (path_tracing.frag:338)
  // the reference tree's leaves (2 x float4 each: (box lo, leaf ref bits), (box hi, -)): the primary-ray tile
  // rasteriser's items (wf_primary_raster)
  const float4* leaves;
  int nleaves;
  // per triangle of tri_geom: the index into `leaves` of the reference leaf holding it, -1 for a triangle no leaf
  // holds (launch_tri_leaf_map); the triangle rasteriser's items are the triangles (wf_primary_tri)
  const int* tri_leaf;
};

// Wavefront path-tracer state (kernels_wavefront.hip and its stages, kernels_wf_*.hip): SoA per band pixel.
struct WFState {
  float4 *ray_o, *ray_d;        // current ray (origin, direction)
  float4 *light, *red;          // radiance accumulator, path throughput ("reduction")
  float4 *pend0, *pend1, *pend2, *pend3;  // NEE terms awaiting the shadow verdicts
  float4 *sh_h, *sh_p;          // shadow directions (HDR; point light + distance in .w)
  int2* hit;                    // closest hit (triangle, t bits)
  uint32_t* seed;               // RNG state (path_tracing.frag:433)
  uint8_t *occ_h, *occ_p;       // shadow verdicts
  int *list0, *list1;           // compacted live-ray lists (ping-pong), kLiveBins bins of kSeg segments of `cap`
  int* shadow_list;             // compacted shadow rays of one bounce: HDR list, then kPointBins point-light
                                // lists (by light index), each kSeg segments of `cap`
  int* counters;                // per bounce i, base kWfCtr*i: [0, kCtrHdr) live-bin segment counts, then 8 HDR,
                                // 8 kPointBins point-light counts, [kCtrStrag] cooperative-walk stragglers,
                                // 8 + 8 work-queue heads (kCtrQShadow, kCtrQClosest)
  uint32_t* row_cost;           // optional: traversal steps per band row (load-balancing probe), may be null
  int* straggler;               // shadow rays past the step budget: pid | (point << 31), count at kCtrStrag
  uint32_t shadow_budget;       // node + triangle visits before a shadow ray is handed to the cooperative walk (0: never)
  int* strag_c;                 // bounce rays past closest_budget (count at kCtrStragC): the cooperative closest walk
  uint32_t closest_budget;      // node + triangle visits before a bounce ray is handed to it (0: never; refill kernel)
  unsigned long long* stats;    // optional traversal counters (kStat*), wave-aggregated atomics; may be null
  int stats_n;                  // counters the caller's buffer holds: counter k is written only when k < stats_n
  int* spill;                   // deep trees only: stack entries past the LDS stack, entry kStack + j of pixel pid at
  size_t spill_stride;          // spill[j * spill_stride + pid] (spill_stride = band pixels); null otherwise
  // The primary hit (triangle, t bits), a plane of its own: the primary stage writes it and every bounce-0 shade
  // reads it, `hit` being overwritten by the bounce-1 trace. It survives the draw, so a later draw of the same pass
  // from the same view skips the stage (DESIGN.md "Static view"). Host side only: launch_wavefront passes it to the
  // primary and bounce-0 launches as their `hit`; no kernel names this field.
  int2* hit0;
  // The bounce-0 point-light verdicts of this pass's pixels from the view hit0 was traced for (point_cache.h): one
  // word per pixel, touched only by draws whose PTParams::point_cache is not kPcOff.
  uint16_t* pcache;
};
// Traversal counters of one path-tracing draw (pt_pass_set_trace_stats): rays traced and node + triangle visits
// per traversal kind, tie re-walks on the reference tree, primary rays retried unbounded after the G-buffer bound, rays
// whose stack went past the LDS stack into the spill columns (deep reference trees), and per traversal kind the lane
// slots its waves occupied (64 x the wave's largest visit count, summed over waves): visits / slots is the share of
// SIMD lanes doing useful traversal work (divergence: a wave runs as long as its longest ray); of the shadow rays
// (lane-refill walks), those toward point lights and those found occluded.
enum { kStatPrimRays, kStatPrimVisits, kStatBounceRays, kStatBounceVisits, kStatShadowRays, kStatShadowVisits,
       kStatTieRewalks, kStatPrimRetries, kStatSpills, kStatPrimSlots, kStatBounceSlots, kStatShadowSlots,
       kStatShadowPoint, kStatShadowOccluded,
       // point-light rays the light's triangle bins decided (wf_shadow_point_bins) / handed to the walk instead
       kStatShadowPointBinned, kStatShadowPointFallback, kStatCount };
constexpr int kStatCountV2 = kStatShadowOccluded + 1;  // the 14 counters pt_trace_stats_count() has always reported

// A path-tracing draw over several frames' pixels (pt_pass_draw_batch): frame b's pixels are the pids
// [b * n, (b + 1) * n) of one shared per-pixel wavefront state; its lists hold frame-local pids. The list-driven
// traversal kernels take every frame's list of a bounce at once, so one launch traces the whole batch's rays.
constexpr int kMaxBatch = 8;
struct ListBatch {
  int nb;               // frames
  int n;                // pixels per frame (the pid offset of frame b is b * n)
  const int* list[kMaxBatch];
  const int* counts[kMaxBatch];
};

// Several samples per pixel in one draw (uniform spp = n, DESIGN.md "Samples per pixel"): the n samples run as the n
// "frames" of a batch over one shared primary hit, each path's end writes its sample's colour to plane s of
// `samples` (float4 per band pixel, n planes `stride` texels apart), and wf_spp_resolve folds them in sample order
// into the pass's colour attachment.
struct SppResolve {
  int n;                  // samples, 2 .. kMaxBatch
  const float4* samples;  // sample s of band pixel pid: samples[s * stride + pid]
  size_t stride;          // band pixels
  Plane color, last;      // the pass's colour attachment; lastFrame (read when accumulate != 0 and last.p)
  int accumulate;
  uint32_t frameCounter;  // the frame's own counter F (the accumulation weight), not a sample's
  int W, y0, y1;          // the band, and the tile subset the draw traced (PTParams::tile_stride)
  int tile_stride, tile_offset;
};

// Per-pixel sample counts and statistics of an spp draw (DESIGN.md "Adaptive sample counts"), both addressed by frame
// pixel in global rows (y * W + x) and either one optional. counts: pixel's samples n = min(max(c, 1), N); sample s
// exists iff s < n. stats: the resolve writes (mean, unbiased variance) of the samples' luminances, (l_0, -1) at n < 2.
// moments (DESIGN.md "SVGF from sample moments"; optional, addressed like the other two): the resolve writes (mu, nu,
// r, float(n)) of the samples demodulated by the draw's own `emission` and `albedo` planes (read only when moments is
// set), for the reproject and variance passes' sampler gSampleMoments.
struct SppAdaptive {
  const uint8_t* counts;
  float2* stats;
  float4* moments;
  Plane emission, albedo;
};

// pt_sample_counts_derive: the next draw's count plane from a draw's statistics, followed along this frame's motion
// vectors (spp_counts_kernel). motion / nd: gMotion / gNormalAndLinearZ of the whole W x H frame.
struct SppCountsParams {
  const float2* stats;
  const float4* motion;
  const float4* nd;
  uint8_t* out;
  int W, H, nmax;
  float lag, tol;
};
int launch_spp_counts(const SppCountsParams& c, hipStream_t s);

// pt_sample_counts_pool: the next draw's count plane from luminance statistics pooled over the slot's draws
// (spp_pool_kernel; tests/adaptive_pool_ref.py). stats / counts_prev / pool_in: the previous draw's statistics, the
// count plane it read (its spp nmax_prev) and the pool plane of its step, all in that draw's pixel coordinates and
// each optional; pool_out: float4 (m, v, w, z) per frame pixel; rule 0 relative, 1 absolute.
struct SppPoolParams {
  const float2* stats;
  const uint8_t* counts_prev;
  const float4* pool_in;
  const float4* motion;
  const float4* nd;
  float4* pool_out;
  uint8_t* out;
  int W, H, nmax, nmax_prev, rule;
  float lag, tol, wmax, zeta;
};
int launch_spp_pool(const SppPoolParams& c, hipStream_t s);

// Screen-tile binning of items (the G-buffer's triangles, the path tracer's BVH leaves) for the tile rasterisers:
// an item-specific setup kernel writes each item's pixel box and counts it into the 16 x 16 tiles of the band it
// covers (bins_count_item); launch_bins then bins the large items, scans and scatters (kernels_pt.hip).
constexpr int kRTile = 16;
constexpr int kLargeTiles = 8;   // items covering more tiles are binned by a whole block
constexpr int kBoxMargin = 2;    // pixels added around a projected box (projection vs ray arithmetic)
struct Bins {
  int n;                // items
  int4* box;            // per item: pixel box (x0, y0, x1, y1) of the pixels whose ray it can meet; empty: x0 > x1
  float* tmin;          // per item: lower bound of the ray parameter of any hit (0 when unknown)
  int* tile_count;      // per tile of the band: items binned to it; the scatter counts it back to zero
  int* tile_off;        // ntiles + 1: exclusive scan of tile_count
  int* pairs;           // item indices grouped by tile
  int pair_cap;
  int* large;           // items whose box covers more than kLargeTiles tiles (binned by whole blocks)
  int large_cap;
  int* ctr;             // [0] large items, [1] binned pairs, [2] overflow (the caller's fallback then runs)
  int W, y0, y1;        // band: tiles counted from row y0
};

// Point-light triangle bins (kernels_pointbins.hip): per light l < nl a cube map of 6 x R x R direction cells around
// the light. Cell c = (face * R + row) * R + column of light l has the header hdr[l * (ncell + 1) + c] = (first
// entry, entries) into ent + l * cap; header ncell is the light's catch-all list (triangles the build cannot bound:
// every ray to the light tests them). An entry is 8 bytes, (triangle, near16 | box16 << 16): near16 the high 16 bits
// of the float `near`, a lower bound of the distance from the light to any point of the triangle a shadow ray can be
// found to hit (a cell's entries ascend by it; truncating a float >= 0 rounds it down); the box (x0 | x1 << 4 |
// y0 << 8 | y1 << 12, in 1 / 16 of the cell) holds every direction of the cell from which such a ray can arrive.
// info: kPointBinsInfo ints per light: [0] != 0: the light has no usable bins (a non-finite position, or the entries
// overflowed `cap`: its rays walk; 2: the light moved and its lists are pending, capi_draw_pt.hip point_bins_for), [1] entries, [2..4] float bits of the light position the bins were built around,
// [5] float bits of Mtot, the coordinate magnitude of the scene plus the light's, [6] the catch-all list's entries,
// [7] the (triangle, face) boxes of the light's last build that went to pb_bin_large (kernels_pointbins.hip).
constexpr int kPointBinsInfo = 8;
constexpr int kPointBinsMaxR = 128;  // (the build packs a cell box into 4 x 8 bits)
struct PointBinsDev {
  const int2* hdr;
  const uint2* ent;
  const int* info;
  int R, nl, cap;
  __host__ __device__ int ncell() const { return 6 * R * R; }
};

struct PTParams {
  int W, H, y0, y1;     // frame size (global) and rows to compute
  Plane color, emission, albedo, last;  // outputs (+ lastFrame input)
  SceneDev scene;
  Tex hdr, cache;
  // hdrMap's radiance (.xyz) and hdrCache's pdf (.z) of each texel in one float4 (capi_draw_pt.hip pt_params, hdr_merged), when both
  // textures have one size: the NEE's hdr_color + hdr_pdf at one direction then read one texture (null: two)
  Tex hdr_pdf;
  int hdrResolution;
  int pointLightSize;
  uint32_t frameCounter;
  float eye[3];
  float camRot[16];     // column-major inverse(view)
  int accumulate;
  float clamp_threshold;
  int max_depth;
  int aspect_corrected;
  int prune;            // closest-hit pruning (parity-safe margin)
  int closest_tree;     // closest-hit rays walk the SAH tree over the reference leaves (closest_hit, pt_shading.h)
  int stack_need;       // deepest interior level of the binary BVH (selects the LDS stack size)
  int refill;           // > 0: percent of each bounce/shadow list traced by lane-refill waves (kernels_wf_trace.hip)
  int refill_waves;     // resident waves a refill launch is sized for (0: the whole chip, kResidentWaves)
  int refill_grid;      // most blocks of a refill launch (uniform refill_grid; 0: PTSVGF_REFILL_GRID / its default)
  int list_grid;        // most blocks of the list-driven shade / finish (uniform list_grid; 0: PTSVGF_LIST_BLOCKS)
  int shade_fold;       // wavefront: paths write `color` where they end, a bounce's verdicts are applied by the next
                        // shade (uniform shade_fold, default 1; 0: wf_finish per bounce and wf_finalize, for A/B)
  float sobol_u[4], sobol_v[4];  // sobolVec2(frameCounter+1, b): uniform across pixels
  WFState wf;
  // optional bound for the primary rays from this frame's G-buffer (world position + normal/linearZ planes,
  // drawn before on the same stream): see wf_primary. p == null: no bound
  Plane hint_pos, hint_nd;
  TileSched tiles;      // primary-ray tiles (16 x 16 px), indexed by subset slot (below)
  // Tile subset (wavefront path tracer only): trace the 16 x 16 tiles t = k * tile_stride + tile_offset of
  // the band (raster tile order), k = 0 .. tiles.ntiles - 1; other pixels are left untouched. Stride 1,
  // offset 0 = every tile. Interleaved subsets give every rank of a multi-GPU frame an equal share of the
  // expensive tiles (ptsvgf.dist, DESIGN.md "Multi-GPU").
  int tile_stride, tile_offset;
  // primary rays by tile rasterisation (primary_raster uniform) of the reference leaves (1: wf_primary_raster) or of
  // the triangles (2: wf_primary_tri): the bins of those items, and for the wf_primary launch that follows it the
  // bins' counters (pr_fix non-null: that launch walks only the pixels the rasteriser flagged — exact-t ties — or
  // every pixel after a list overflow)
  Bins leaf_bins;
  int primary_raster;
  const int* pr_fix;
  // point_bins != 0: the point-light shadow rays of the lights with usable bins are decided by wf_shadow_point_bins
  // over `pbins`; the shadow walks take the HDR rays and the other lights' (uniform point_bins; capi_draw_pt.hip point_bins_for)
  int point_bins;
  PointBinsDev pbins;
  // the bounce-0 point-light verdict cache's mode for this launch (PointCacheMode, point_cache.h). launch_wavefront
  // hands it to the bounce-0 shade and to the launch that consumes bounce 0's verdicts; every other launch gets kPcOff.
  int point_cache;
  // The bounce-0 shade's keep mode (DESIGN.md "Static view, part 4"), read by the folded bounce-0 instantiations
  // alone: non-null when the host has proven (capi_static.hip first_hit_mode_for) that `color` already holds this
  // draw's miss texels and `emission` / `albedo` this draw's first-hit texels. A miss pixel then does nothing,
  // launch_wavefront passes both first-hit planes null, and block b shades tile busy[1 + b] of the pass's busy-tile
  // list (the tiles of the bounce-0 order that hold a primary hit, in that order; busy[0]: how many), blocks past its
  // length return.
  const int* busy;
};
// The busy-tile list of a whole-frame draw whose primary hit plane (wf.hit0) is complete: busy[0] = the number of
// tiles with a pixel whose hit0.x >= 0, busy[1 ..] those tiles as the bounce-0 shade names them (tiles.perm_next's
// entry, or the block index without a tile order), in the shade's order. busy: 2 * ntiles + 1 ints, the upper ntiles
// scratch. Two launches on s.
int launch_busy_tiles(const PTParams& p, int* busy, hipStream_t s);
inline size_t busy_tiles_ints(int ntiles) { return 2 * (size_t)ntiles + 1; }

struct GBufParams {
  int W, H, y0, y1;
  Plane world, normal_depth, motion, fwidth;
  float* fwidth_aux;    // compact depth-fwidth plane (rows of fwidth), may be null
  // compact primary-ray bound plane (rows of world), may be null: per pixel the float the path tracer's primary
  // rasterisers prune with (raster_bound, kernels_wf_primary.hip), for primary rays that start at bound_eye
  float* bound_aux;
  float bound_eye[3];
  unsigned char* tflags;  // a-trous per-tile surface flags (atrous_mark_tiles) of rows [tf_y0, tf_y1), may be null
  int tf_off[5];          // their per-step offsets (atrous_flag_offset)
  int tf_y0, tf_y1;       // the rows the a-trous passes draw (default: the G-buffer's own rows)
  const float4* geom;   // 4 x float4 per raster triangle (walk): (p1,idx)(e1,-)(e2,-)(Ng,-)
  const float4* nrm;    // 3 x float4 per raster triangle (closest hit only): n1, n2, n3
  const float4* disp;   // object motion, or null: 3 x float4 per raster triangle, (prev - cur of vertex j, moved flag)
  const float4* bvh;
  int root_ref;
  int stack_need;       // deepest interior level of the raster BVH
  float eye[3];
  float invR[9];        // row-major R^T (camera-to-world rotation)
  float P00, P11;       // projection diagonal (pixel ray scale)
  float M[16];          // projection * view (column-major)
  float PV[16];         // pre_viewproj
  TileSched tiles;      // 16 x 16 px tiles
  uint32_t* motion_max; // optional: max |motion.y| (float bits) over the launch's surface pixels, zeroed by the host
  Bins bins;            // tile-binned rasterisation (gbuffer_mode 1): items = the raster triangles; bins.ctr null
                        // when the ray cast runs alone
};

struct ReprojParams {
  int W, H, y0, y1;
  Plane motion, color, albedo, emission, prev_illum, prev_moments, nd, prev_nd, fwidth;
  Plane out_illum, out_moments;
  float inv_w, inv_h, depth_thr, normal_thr;
  int block;  // 1: the four history taps from one 3x3 texel block per plane when they tile it (same texels, same bits)
  Plane sm;   // gSampleMoments (kernels_svgf.hip header), p == null: not bound
  // static background (DESIGN.md "Static view, part 3"): per 16 x 16 block of the frame, 0 iff the host has proven that
  // the block's stores would change nothing; such a block exits before its first load. Null: every block runs.
  const unsigned char* busy16;
};

struct VarianceParams {
  int W, H, y0, y1;
  Plane illum, moments, nd, fwidth, out;
  float phi_color, phi_normal;
  Plane sm;  // gSampleMoments (kernels_svgf.hip header), p == null: not bound
  const unsigned char* busy16;  // as ReprojParams::busy16
};

struct AtrousParams {
  int W, H, y0, y1;
  Plane illum, nd, fwidth, out;
  int step;
  float phi_color, phi_normal;
  const unsigned char* tile_any;  // tiled kernel: per-tile "holds a surface pixel" flags of this step, or null
  // tiled kernel, static background (DESIGN.md "Static view, part 3"): in tile_any's layout, 0 iff the host has proven
  // that the tile's copy (and fused modulate) would store what out (and mod) already hold; such a background tile
  // returns without the copy. Null: every tile runs.
  const unsigned char* busy;
  // fused modulate (the last iteration of a frame, fast driver): mod.p != null writes modulate_kernel's output of
  // this draw's rows from `out`'s values, albedo and emission (every plane must store the draw's rows)
  Plane albedo, emission, mod;
};
// Tiles of the tiled a-trous (kernels_atrous.hip): 64 * NX columns x TJ rows of one residue class mod S, one wave
// per 64-column strip of a tile row (64 * TJ * NX <= 1024 threads); tile (g, b, bx) of step S has byte
// (g * S + b) * NXT + bx in that step's flags. The staged footprint is (TJ + 4) x (64 NX + 4S) texels for TJ x 64 NX
// pixels. PT_ATROUS_TJ (rows for S <= 8) / PT_ATROUS_TJ16, PT_ATROUS_NX16 (S = 16) choose the shape (A/B).
#ifndef PT_ATROUS_TJ
#define PT_ATROUS_TJ 8
#endif
#ifndef PT_ATROUS_TJ16
#define PT_ATROUS_TJ16 8
#endif
#ifndef PT_ATROUS_NX16
#define PT_ATROUS_NX16 2
#endif
__host__ __device__ constexpr int atrous_tile_tj(int S) { return S >= 16 ? PT_ATROUS_TJ16 : PT_ATROUS_TJ; }
__host__ __device__ constexpr int atrous_tile_nx(int S) { return S >= 16 ? PT_ATROUS_NX16 : 1; }
static_assert(64 * PT_ATROUS_TJ <= 1024 && 64 * PT_ATROUS_TJ16 * PT_ATROUS_NX16 <= 1024, "a-trous tile too large");
__device__ __forceinline__ void atrous_mark_tiles(unsigned char* flags, const int* off, int W, int x, int r) {
#pragma unroll
  for (int si = 0; si < 5; ++si) {
    const int S = 1 << si, nx = atrous_tile_nx(S), nxt = (W + 64 * nx - 1) / (64 * nx);
    const int g = r / (S * atrous_tile_tj(S)), b = r % S;
    flags[off[si] + (size_t)(g * S + b) * nxt + x / (64 * nx)] = 1;
  }
}
// per-tile surface flags of the tiled a-trous for the 5 steps (1, 2, 4, 8, 16) of rows [y0, y1), from the
// depth-fwidth plane's sign bits: atrous_flag_bytes() bytes, step si's flags at atrous_flag_offset(si)
size_t atrous_flag_bytes(int W, int y0, int y1);
size_t atrous_flag_offset(int si, int W, int y0, int y1);
int atrous_tile_flags(const Plane& fwidth, int W, int y0, int y1, unsigned char* flags, hipStream_t s);
// The quiet-tile flags of a whole W x H frame (capi_state.h QuietSet): a byte of `flags` (the a-trous tiles of the five
// steps, in the layout above over rows [0, H)) and of `flags16` (16 x 16 blocks, row-major, (W + 15) / 16 per row) is
// set to 1 iff a pixel of the tile is a surface pixel by the compact depth-fwidth plane `aux` (rows from row0) or a
// hit in the primary plane hit0 (pixel y * W + x); then counts[0 .. 5]: the bytes set per shape. All of them zeroed first.
int launch_quiet_flags(const float* aux, int row0, const int2* hit0, int W, int H, unsigned char* flags,
                       unsigned char* flags16, uint32_t* counts, hipStream_t s);

struct ModulateParams {
  int W, H, y0, y1;
  Plane albedo, emission, illum, nd, out;
};

struct OutputParams {
  int W, H, y0, y1;
  Plane in, out;
};

struct TAAParams {
  int W, H, y0, y1;
  Plane cur, prev, vel, nd, out;
  uint32_t frameCounter;
};

// Tile-shard transfer (kernels_shard.hip): the pixels of the 16 x 16 tile subset (t = k * stride + seg.offset, tiles
// numbered row-major from row tile_y0, W / 16 per row) in rows [seg.y0, seg.y1) of each plane, to (unpack = 0) or from
// (1) the segment's packed block: plane-major, rows in order, each row's subset tiles in x order.
constexpr int kShardSegs = 16;
struct ShardSeg {
  int y0, y1, offset;
  float4* packed;
};
struct ShardCopy {
  int W, tile_y0, stride, nseg, nplanes, unpack;
  float4* plane[4];
  int row0[4];
  ShardSeg seg[kShardSegs];
};

}  // namespace ptk

#if defined(__HIPCC__)
namespace ptk {
// Launchers (kernels_*.hip). Return hipError_t as int.
int launch_shard_copy(const ShardCopy& c, hipStream_t s);
long long shard_pixels(int W, int tile_y0, int stride, int offset, int y0, int y1);  // per plane
int launch_pathtrace(const PTParams& p, hipStream_t s);
// A side stream for the wavefront's bounce-0 shadow rays: they and the bounce-1 closest-hit rays both come from the
// bounce-0 shade and touch disjoint buffers, so the two walks run at once and fill each other's launch tails.
// `fork` is recorded on the draw's stream after that shade, `join` on the side stream after the bounce-0 finish.
struct WfFork {
  hipStream_t side;
  hipEvent_t fork, join;
};
// reuse_primary: p.wf.hit0 (and the tile order in p.tiles.perm_next) still hold what the primary stage would write for
// this draw (the caller's key compare, static_key.h): the stage is not launched
int launch_pathtrace_wavefront(const PTParams& p, hipStream_t s, const WfFork* fk = nullptr,
                               bool reuse_primary = false);
// 1 when the walk kernels' translation unit keeps f32 subnormals (max(0, least subnormal) > 0, evaluated on the device
// with the walk code's compile flags), as PT_WIDE_SIGNED's one-compare child test needs; 0 if it flushes; < 0 a HIP error
int subnormal_probe(hipStream_t s);
int wf_list_capacity(int W, int rows);  // per-segment capacity of the compacted ray lists (8 segments)
int wf_subset_tiles(int W, int rows, int stride, int offset);  // tiles of a PTParams tile subset (< 0: invalid)
int launch_gbuffer(const GBufParams& p, hipStream_t s);
int launch_gbuffer_raster(const GBufParams& p, hipStream_t s);
int launch_gbuffer_adopt(const GBufParams& p, hipStream_t s);  // side data of G-buffer planes written elsewhere  // bins, resolves, and the ray cast on overflow
int launch_bins(const Bins& b, hipStream_t s);  // after the item setup kernel: large items, scan, scatter
// SceneDev::tri_leaf of `ntris` triangles from the `nleaves` reference leaves' refs (first, count)
int launch_tri_leaf_map(const float4* leaves, int nleaves, int* tri_leaf, int ntris, hipStream_t s);
// nb frames' path tracing with batched traversal launches (ps[b]: frame b, its wavefront state at pid offset b * n)
int launch_pathtrace_wavefront_batch(const PTParams* ps, int nb, hipStream_t s, const WfFork* fk = nullptr);
// rs.n samples of one frame (ps[s]: sample s, built by spp_sample_params, spp_params.h): the primary stage runs for
// sample 0 alone, every sample's bounce-0 shade reads its hit, and wf_spp_resolve writes rs.color after the last finish
// ad (optional): the draw's count and statistics planes; without it, or with both null, the launches are the plain ones
int launch_pathtrace_wavefront_spp(const PTParams* ps, const SppResolve& rs, hipStream_t s, const WfFork* fk = nullptr,
                                   const SppAdaptive* ad = nullptr, bool reuse_primary = false);
int launch_reproject(const ReprojParams& p, hipStream_t s);
int launch_variance(const VarianceParams& p, hipStream_t s);
int launch_atrous_exact(const AtrousParams& p, hipStream_t s);
int launch_atrous_fast(const AtrousParams& p, hipStream_t s);   // LDS-tiled (production)
int launch_atrous_step(const AtrousParams& p, hipStream_t s);   // step-specialised, texture-path taps
int launch_atrous_simple(const AtrousParams& p, hipStream_t s);
int launch_modulate(const ModulateParams& p, hipStream_t s);
// the modulate an a-trous draw with AtrousParams::mod set asks for, as its own launch (kernels that do not fuse it)
int launch_modulate_after(const AtrousParams& p, hipStream_t s);
int launch_output(const OutputParams& p, hipStream_t s);
int launch_taa(const TAAParams& p, hipStream_t s);
int launch_tile_sort(uint32_t* cost, int* perm, int ntiles, hipStream_t s);  // cost -> perm, clears cost
int launch_hdr_merge(const float4* hdr, const float4* cache, float4* out, int n, hipStream_t s);  // (hdr.xyz, cache.z)
// Point-light triangle bins of `nl` lights (sc.lights, 6 floats each) over sc's triangles with R x R cells per cube
// face: point_bins_bytes() bytes at `base`; *out describes them. Everything runs on s; nothing is read back.
size_t point_bins_bytes(int ntris, int nl, int R, int tight);
// tight != 0: a triangle is listed in the cells its projected polygon reaches (pb_overlap.h), 0: in every cell of
// the polygon's box (A/B).
constexpr int kPointBinsEntryBytes = 8;
int launch_point_bins_build(const SceneDev& sc, int nl, int R, int tight, void* base, PointBinsDev* out,
                            hipStream_t s);
// Moving point lights: light l's lists rebuilt in place around its position in sc.lights, the other
// lights' sections untouched; info[l][0] = 2 ("moved, bins pending": its rays walk); a light's sections in `base`.
int launch_point_bins_rebuild_light(const SceneDev& sc, int nl, int R, int tight, void* base, int l, hipStream_t s);
int launch_point_bins_mark_moved(const PointBinsDev& pb, int l, hipStream_t s);
void point_bins_sections(int ntris, int nl, int R, int tight, int l, size_t* hdr_off, size_t* ent_off);
// The verdict cache forgets the lights of `mask` (pc_forget, point_cache.h) on the n words of `plane`
// (kernels_lights.hip).
int launch_point_cache_forget(uint16_t* plane, size_t n, uint32_t mask, hipStream_t s);
// The environment's importance cache on the device (kernels_environment.hip, DESIGN.md "Environment edits").
// environment_expand: n RGB texels (3 floats each) to (R, G, B, 1). environment_scratch_floats: the floats of scratch a
// W x H build works in. launch_environment_cache: from the hdr texels, the cache texels (x, y, pdf, 1) of pts_hdr_cache
// and the merged plane (hdr.xyz, pdf), bit for bit; 1 <= W, H <= kEnvMaxSide. Everything runs on s.
constexpr int kEnvMaxSide = 8192;
int launch_environment_expand(const float* rgb, float4* hdr, int n, hipStream_t s);
size_t environment_scratch_floats(int W, int H);
int launch_environment_cache(const float4* hdr, float4* cache, float4* merged, float* scratch, int W, int H,
                             hipStream_t s);
}  // namespace ptk

namespace ptk {
// The tree shadow (any-hit) rays walk: bvh_any when present (same verdicts), else the reference tree.
__device__ __forceinline__ SceneDev anyhit_scene(const SceneDev& s) {
  SceneDev r = s;
  if (s.bvh_any) {
    r.bvh = s.bvh_any;
    r.root_ref = s.root_any;
  }
  return r;
}
__device__ __forceinline__ int sched_tile(const TileSched& t, int slot) { return t.perm ? t.perm[slot] : slot; }

struct TileBox {
  int tx0, tx1, ty0, ty1;
  __device__ int area() const { return (tx1 - tx0 + 1) * (ty1 - ty0 + 1); }
};
__device__ __forceinline__ TileBox tile_box(const Bins& b, int4 box) {
  return TileBox{box.x / kRTile, box.z / kRTile, (box.y - b.y0) / kRTile, (box.w - b.y0) / kRTile};
}
// Pixel box of projected extents (pixel coordinates of the centre rays), widened by `margin`, clipped to the band.
__device__ __forceinline__ int4 pixel_box(const Bins& b, float x0, float y0, float x1, float y1,
                                          int margin = kBoxMargin) {
  const float lim = 1.0e8f;  // keeps the float -> int conversion in range
  const int bx0 = (int)floorf(fmaxf(x0, -lim)) - margin, bx1 = (int)ceilf(fminf(x1, lim)) + margin;
  const int by0 = (int)floorf(fmaxf(y0, -lim)) - margin, by1 = (int)ceilf(fminf(y1, lim)) + margin;
  return make_int4(max(bx0, 0), max(by0, b.y0), min(bx1, b.W - 1), min(by1, b.y1 - 1));
}
// Sutherland-Hodgman against s * w + sgn * c[axis] >= 0 (homogeneous coordinates: x, y, w)
__device__ __forceinline__ int clip_plane(const float3* in, int n, float3* out, int axis, float sgn) {
  const float s = 1.01f;
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const float3 a = in[i], b = in[(i + 1) % n];
    const float da = s * a.z + sgn * (axis == 0 ? a.x : a.y), db = s * b.z + sgn * (axis == 0 ? b.x : b.y);
    if (da >= 0.0f) out[m++] = a;
    if ((da >= 0.0f) != (db >= 0.0f)) {
      const float t = da / (da - db);
      out[m++] = make_float3(a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z));
    }
  }
  return m;
}

// Screen box and nearest-t bound of a convex polygon given by n <= 8 vertices (x, y, w) in a frame whose centre
// rays have NDC ((2x+1)/W - 1, (2y+1)/H - 1) scaled by (sx, sy): clipped to the widened frustum first.
// Returns false when nothing of it lies in front of the camera inside the frustum.
__device__ __forceinline__ bool poly_box(const Bins& b, int H, float3* A, int n, float sx, float sy, int4* box,
                                         float* tmin, int margin = kBoxMargin) {
  float3 B[16];
  n = clip_plane(A, n, B, 0, 1.0f);
  n = clip_plane(B, n, A, 0, -1.0f);
  n = clip_plane(A, n, B, 1, 1.0f);
  n = clip_plane(B, n, A, 1, -1.0f);
  if (n <= 0) return false;
  float x0 = 3.0e38f, y0 = 3.0e38f, x1 = -3.0e38f, y1 = -3.0e38f, wmin = 3.0e38f;
  for (int k = 0; k < n; ++k) {
    if (!(A[k].z > 0.0f)) {  // on the camera plane: the whole band, no bound
      *box = make_int4(0, b.y0, b.W - 1, b.y1 - 1);
      *tmin = 0.0f;
      return true;
    }
    wmin = fminf(wmin, A[k].z);
    // pixel coordinate whose centre ray has this NDC: ndc = (2 x + 1) / W - 1
    const float px = ((A[k].x / (A[k].z * sx) + 1.0f) * (float)b.W - 1.0f) * 0.5f;
    const float py = ((A[k].y / (A[k].z * sy) + 1.0f) * (float)H - 1.0f) * 0.5f;
    if (!(px == px && py == py)) {
      *box = make_int4(0, b.y0, b.W - 1, b.y1 - 1);
      *tmin = 0.0f;
      return true;
    }
    x0 = fminf(x0, px); x1 = fmaxf(x1, px);
    y0 = fminf(y0, py); y1 = fmaxf(y1, py);
  }
  *box = pixel_box(b, x0, y0, x1, y1, margin);
  *tmin = wmin;
  return true;
}

// Records item i's box and bound and counts it into its tiles (small items) or queues it (large ones).
__device__ __forceinline__ void bins_count_item(const Bins& b, int i, int4 box, float tmin) {
  b.box[i] = box;
  b.tmin[i] = tmin;
  if (box.x > box.z || box.y > box.w) return;
  const TileBox tb = tile_box(b, box);
  if (tb.area() > kLargeTiles) {
    const int slot = atomicAdd(&b.ctr[0], 1);
    if (slot < b.large_cap) b.large[slot] = i;
    else atomicOr(&b.ctr[2], 1);
    return;
  }
  const int ntx = (b.W + kRTile - 1) / kRTile;
  for (int ty = tb.ty0; ty <= tb.ty1; ++ty)
    for (int tx = tb.tx0; tx <= tb.tx1; ++tx) atomicAdd(&b.tile_count[ty * ntx + tx], 1);
}
// Call with every lane of the wave active (steps = 0 for lanes without a ray).
__device__ __forceinline__ void sched_cost(const TileSched& t, int tile, uint32_t steps) {
  if (!t.cost) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) steps = max(steps, (uint32_t)__shfl_xor((int)steps, o));
  if ((threadIdx.x & 63) == 0 && steps) atomicMax(t.cost + tile, steps);
}
// GPU LBVH builder (kernels_bvh.hip): Triangle_encoded texels in, triangles in leaf order + BVHNode_encoded
// nodes out (the reference's upload formats, main.cpp:101-151). Scratch grows on demand and is reused.
struct LbvhWork {
  void* base = nullptr;
  size_t bytes = 0;
  static size_t need(int n);
};
// Triangle_encoded texels (device) -> tri_geom (4 float4) / tri_shade (9 float4) records, as get_scene decodes them
int decode_tris(const float* te, int n, float4* geom, float4* shade, hipStream_t s);
// Raster vertex list (18 floats per triangle) -> the G-buffer's geom (4 float4) / nrm (3 float4) records in the
// given leaf order (order[k] = original triangle index), as pt_raster_pass_bind builds them on the host
int decode_raster(const float* verts, const int* order, int n, float4* geom, float4* nrm, hipStream_t s);
// Object motion: disp (3 float4 per raster triangle, leaf order) = prev - cur of the n-triangle vertex lists at each
// record's original index (geom[4k].w), .w = 1 where the triangle moved
int raster_disp(const float4* geom, const float* prev, const float* cur, int n, float4* disp, hipStream_t s);
// Where a triangle record keeps its vertices: p1 at 0, p2 at o2, p3 at o3, records `stride` floats apart.
struct TriLayout {
  int stride, o2, o3;
};
constexpr TriLayout kTriEncoded{45, 3, 6};   // Triangle_encoded (Utils/Triangle.h:12-24)
constexpr TriLayout kRasterVerts{18, 6, 12};  // the raster vertex list (obj_loader.h:143-160)
// node_out needs room for 2n nodes (12 floats each); *nnodes = nodes written (dummy node 0 included).
// ploc_r > 0: the tree above the LBVH leaves is rebuilt by PLOC with search radius ploc_r. tri_out (45-float
// records only) may be null; order (may be null) receives the original index of each leaf-order position.
int lbvh_build(LbvhWork& w, const float* tri, TriLayout lay, int n, int leaf_n, int ploc_r, float* tri_out,
               float* node_out, int* order, int* nnodes, hipStream_t s);

// The walk trees of a tree lbvh_build wrote, derived on the device from its BVHNode_encoded texels (lbvh_trees):
// the packed binary tree (host_trees.cpp pack_bvh's records), the leaf list (upload_leaves') and the 4-wide tree
// (pack_wide's greedy collapse), bit for bit what those host functions make of the same texels.
struct LbvhTrees {
  void* base = nullptr;  // one allocation: bin | leaves | wide (the owner frees it)
  float4 *bin = nullptr, *leaves = nullptr, *wide = nullptr;
  int cap_bin = 0, cap_leaves = 0, cap_wide = 0;  // records each part has room for
  // what the device reports (one copy): root_ref, need (deepest interior level), leaves, root4, need4, 4-wide nodes,
  // NaN flag (a child box of the 4-wide tree has a NaN coordinate), [7] unused; packed binary nodes; error bits
  // (1: a child index out of range, 2: a record past its part's room, 4: the refit before the stage met a bad index)
  int dev_info[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  float stage_ms = 0.0f;  // device time of the stage
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint64_t version = 0;  // the node texture's version these trees were derived from (capi_geometry.hip)
  int nbin() const { return dev_info[8]; }
  int nleaves() const { return dev_info[2]; }
  int nwide() const { return dev_info[5]; }
};
// Launches the stage on s over `nodes` (nnodes x 12 floats on the device, dummy node 0, root node 1) and the copy of
// dev_info; nothing is read back before lbvh_trees_finish, which the caller runs after its next synchronisation of s
// (it fails when the texels were no tree). Only ever run on lbvh_build's own output. Scratch comes from w.
// refit_err (may be null): the error word of an lbvh_refit_nodes launched before on s; when set, the stage reports
// error bit 4 with its own (dev_info[9]) and lbvh_trees_finish fails.
int lbvh_trees_launch(LbvhWork& w, const float* nodes, int nnodes, LbvhTrees& out, hipStream_t s,
                      const int* refit_err = nullptr);
int lbvh_trees_finish(LbvhTrees& t);
void lbvh_trees_free(LbvhTrees& t);

// What a refit of a built tree needs beside its node texels (DESIGN.md "Refit"): the build's leaf order, a parent
// index per output node and the climb's arrival counters. One allocation, sized for the n triangles of the build
// (a tree over them has at most 2n nodes) and kept with the tree; reused by every refit.
struct LbvhRefit {
  void* base = nullptr;  // order[n] | parent[2n] | flags[2n] | err (the owner frees it: lbvh_refit_free)
  int *order = nullptr, *parent = nullptr, *flags = nullptr, *err = nullptr;
  int n = 0, nnodes = 0;  // triangles; output nodes (set by lbvh_refit_link)
};
int lbvh_refit_alloc(LbvhRefit& r, int n);  // no-op when r already holds room for exactly n triangles
void lbvh_refit_free(LbvhRefit& r);
// After lbvh_build(..., r.order, ...) wrote `nodes`: the parent links of its nnodes output nodes.
int lbvh_refit_link(LbvhRefit& r, const float* nodes, int nnodes, hipStream_t s);
// Recomputes every AA / BB of `nodes` in place for the moved triangles `tri` (r.n records of layout lay, in the order
// of the build's input); childs and leafInfo are only read. Leaf boxes fold their triangles in leaf order from the
// first, interior boxes are gmin / gmax (left, right): tests/lbvh_refit_ref.py. Index errors set *r.err.
int lbvh_refit_nodes(LbvhRefit& r, float* nodes, const float* tri, TriLayout lay, hipStream_t s);
// tri_out[p] = tri[r.order[p]] (Triangle_encoded records): the moved triangles in the build's leaf order
int lbvh_refit_reorder(const LbvhRefit& r, const float* tri, float* tri_out, hipStream_t s);

// Posed objects (DESIGN.md "Posed objects", tests/pose_ref.py): out = the rest-pose records placed by their object's
// matrix. mats holds kPoseMatFloats per object: the glm column-major mat4, then the cofactor columns a0, a1, a2 of
// its upper 3x3. Records of no object (objIndex outside [0, n_obj) or no integer) and of identity matrices are
// copied bit for bit.
constexpr int kPoseMatFloats = 25;
// n Triangle_encoded records (objIndex: float 42): positions and normals posed, every other float copied
int pose_tris_launch(const float* rest, int n, const float* mats, int n_obj, float* out, hipStream_t s);
// ntris raster triangles (3 vertices of pos3 + nrm3 each); obj: one int per triangle
int pose_raster_launch(const float* rest, const int* obj, int ntris, const float* mats, int n_obj, float* out,
                       hipStream_t s);

// Skinned objects (DESIGN.md "Skinned objects", tests/skin_ref.py): out = the rest-pose records with every corner
// placed by the blend of its four bones. bones / weights hold four entries per corner (3 corners per record or raster
// triangle); table holds kSkinBoneFloats per bone, 16-byte aligned: the rows (m[k], m[4+k], m[8+k], m[12+k]), k = 0..2,
// of the glm column-major mat4. Corners whose weights all compare == 0, or that name a bone >= n_bones, are copied
// bit for bit.
constexpr int kSkinBoneFloats = 12;
int skin_tris_launch(const float* rest, int n, const uint16_t* bones, const float* weights, const float* table,
                     int n_bones, float* out, hipStream_t s);
int skin_raster_launch(const float* rest, int ntris, const uint16_t* bones, const float* weights, const float* table,
                       int n_bones, float* out, hipStream_t s);

// Material edits (DESIGN.md "Material edits", tests/materials_ref.py): table holds kMaterialFloats per object for the
// objects first .. first + count - 1 (first + count <= 2^24); a record belongs to object o when its objIndex compares
// == (float)o. Records of no named object keep their bits.
constexpr int kMaterialFloats = 18;
// n tri_shade records (9 float4): new_shade = old_shade with the material floats (record floats 9 .. 26) replaced.
// new_shade may be old_shade.
int materials_shade_launch(const float4* old_shade, float4* new_shade, int n, const float* table, int first, int count,
                           hipStream_t s);
// n Triangle_encoded records (objIndex: float 42), floats 18 .. 35 replaced where they lie
int materials_records_launch(float* records, int n, const float* table, int first, int count, hipStream_t s);

}  // namespace ptk
#endif

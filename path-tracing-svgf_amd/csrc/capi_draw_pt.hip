// capi_draw_pt.hip — the path tracer's draws behind pt_pass_draw and pt_pass_draw_batch (capi.hip dispatches): the
// wavefront state of a pass, the scene cache (the kernels' records and trees of a (triangles, nodes) pair, decoded on
// first use), the point-light bins, the draw's PTParams from the pass's bindings, and the one-sample, multi-sample and
// batched draws. Also the tile rasterisers' scratch and the cost-ordered tile dispatch, which the G-buffer draw
// (capi_draw_svgf.hip) shares. Host code only, over the library state of capi_state.h.
#include <cstdio>
#include <type_traits>

#include "capi_state.h"
#include "glsl_builtins.h"
#include "host_trees.h"
#include "spp_params.h"

using namespace ptapi;
using namespace ptk;

namespace {

// Spill columns for a tree needing `need` stack entries (> the LDS stack): (need - kSpillKS + 1) entries per
// pixel of the band, allocated on first use and kept while the depth fits.
int wf_spill(WFBuffers& b, int need) {
  const int levels = need - kSpillKS + 1;
  const size_t m = b.n * (size_t)b.nb;  // columns of the batch's pixels (global pids)
  if (levels <= 0) {
    for (int f = 0; f < b.nb; ++f) {
      b.stb[f].spill = nullptr;
      b.stb[f].spill_stride = 0;
    }
    b.st = b.stb[0];
    return PT_OK;
  }
  if (!b.spill || b.spill_levels < levels || b.spill_cols != m) {
    if (b.spill) (void)hipFree(b.spill);
    b.spill = nullptr;
    if (hipMalloc((void**)&b.spill, (size_t)levels * m * sizeof(int)) != hipSuccess) return PT_ERR_HIP;
    b.spill_levels = levels;
    b.spill_cols = m;
  }
  for (int f = 0; f < b.nb; ++f) {  // frame f's local pid p is column f * n + p
    b.stb[f].spill = b.spill + (size_t)f * b.n;
    b.stb[f].spill_stride = m;
  }
  b.st = b.stb[0];
  return PT_OK;
}

// nsp: sample planes of an spp draw (0: none; such a draw has nb >= nsp frames of state, one per sample)
int wf_alloc(WFBuffers& b, int W, int rows, int nb = 1, int nsp = 0) {
  const size_t n = (size_t)W * (size_t)rows;
  if (b.base && b.n == n && b.nb == nb && b.nsp == nsp) return PT_OK;
  if (b.base) { (void)hipFree(b.base); b.base = nullptr; }
  const size_t m = n * (size_t)nb;  // pixels of the batch
  const size_t f4 = m * 16, al = 256;
  const size_t nl = (size_t)wf_list_capacity(W, rows) * 8;  // 8 list segments
  auto up = [&](size_t v) { return (v + al - 1) / al * al; };
  const size_t lists = up(nl * 4 * kLiveBins) * 2 + up(nl * 4 * (1 + kPointBins));
  // (the second up(m * 8) of int2: the primary hit plane hit0, 8 bytes per pixel; up(m * 2): the point-light verdict
  // plane pcache, 2 bytes per pixel)
  size_t total = up(f4) * 10 + up(m * 8) * 2 + up(m * 2) + up(m * 4) + up(m) * 2 + lists * nb + up(m * 8) + up(m * 4) +
                 up((size_t)nb * kWfCounters * 4) + (nsp ? up((size_t)nsp * n * 16) : 0);
  if (hipMalloc(&b.base, total) != hipSuccess) { b.base = nullptr; return PT_ERR_HIP; }
  b.gen++;
  char* c = (char*)b.base;
  for (int f = 0; f < nb; ++f) b.stb[f] = WFState{};
  // one per-pixel plane of `bpp` bytes per pixel, carved for the batch's m pixels: frame f's share starts f * n pixels in
  auto plane = [&](auto WFState::*mem, size_t bpp) {
    using T = std::remove_reference_t<decltype(b.st.*mem)>;
    for (int f = 0; f < nb; ++f) b.stb[f].*mem = (T)(c + (size_t)f * n * bpp);
    c += up(m * bpp);
  };
  for (auto mem : {&WFState::ray_o, &WFState::ray_d, &WFState::light, &WFState::red, &WFState::pend0, &WFState::pend1,
                   &WFState::pend2, &WFState::pend3, &WFState::sh_h, &WFState::sh_p})
    plane(mem, 16);
  plane(&WFState::hit, 8);
  plane(&WFState::hit0, 8);
  plane(&WFState::pcache, 2);
  plane(&WFState::seed, 4);
  plane(&WFState::occ_h, 1);
  plane(&WFState::occ_p, 1);
  plane(&WFState::straggler, 8);  // both shadow kinds of one bounce (a batch's: frame 0's pointer)
  plane(&WFState::strag_c, 4);    // bounce rays of one bounce
  int* counters = (int*)c; c += up((size_t)nb * kWfCounters * 4);  // contiguous: one memset per draw
  for (int f = 0; f < nb; ++f) {
    WFState& st = b.stb[f];
    st.counters = counters + (size_t)f * kWfCounters;
    st.list0 = (int*)c; c += up(nl * 4 * kLiveBins);
    st.list1 = (int*)c; c += up(nl * 4 * kLiveBins);
    st.shadow_list = (int*)c; c += up(nl * 4 * (1 + kPointBins));
  }
  b.spp = nsp ? (float4*)c : nullptr;
  b.st = b.stb[0];
  b.n = n;
  b.nb = nb;
  b.nsp = nsp;
  return PT_OK;
}

// cells per cube-face edge (uniform point_bins_r overrides: A/B). 128 since the lists hold 8-byte entries of the
// polygon's cells only: its lists are smaller than the 64's were before, and it measured faster
constexpr int kPointBinsR = 128;
// pass uniform primary_raster (pt_wf_setup): 2 = triangles binned to tiles (wf_primary_tri), 1 = reference leaves
constexpr int kPrimaryRasterDefault = 2;

// The triangle -> reference leaf map of a scene whose `leaves` were just built or rebuilt (on g.stream, after the
// work that wrote them).
static int build_tri_leaf(SceneGPU& sg, int ntris) {
  if (ntris > sg.tri_leaf_cap) {
    if (sg.tri_leaf) (void)hipFree(sg.tri_leaf);
    sg.tri_leaf = nullptr;
    sg.tri_leaf_cap = 0;
    HIPCHK(hipMalloc((void**)&sg.tri_leaf, (size_t)ntris * sizeof(int)));
    sg.tri_leaf_cap = ntris;
  }
  if (ntris <= 0) return PT_OK;
  const int rc = ptk::launch_tri_leaf_map(sg.leaves, sg.nleaves, sg.tri_leaf, ntris, g.stream);
  return rc ? hip_err((hipError_t)rc, "triangle leaf map") : PT_OK;
}

static int upload_leaves(const float* ne, size_t nnodes, SceneGPU& sg) {
  std::vector<Float4> lv;
  collect_leaves(ne, nnodes, lv);
  sg.nleaves = (int)(lv.size() / 2);
  // the triangle rasteriser tests a triangle once, under its one leaf's box: a tree whose leaf ranges overlap (the
  // reference would test the shared triangles once per leaf) keeps the leaf rasteriser (pt_wf_setup)
  std::vector<char> seen;
  sg.tri_shared = false;
  for (size_t l = 0; l < lv.size(); l += 2) {
    int ref;
    memcpy(&ref, &lv[l].w, 4);
    const int first = (-(ref + 1)) >> 4, n = (-(ref + 1)) & 15;
    if (first < 0) continue;
    if (seen.size() < (size_t)first + n) seen.resize((size_t)first + n, 0);
    for (int k = first; k < first + n; ++k) {
      sg.tri_shared = sg.tri_shared || seen[k];
      seen[k] = 1;
    }
  }
  return upload_vec(lv, &sg.leaves);
}

// A scene pt_bvh_build wrote (dynamic scenes): its triangles are decoded on the device (decode_tris: the host
// decode's built-ins, the same records), and its own tree (an LBVH, not the reference's SAH tree) serves every walk:
// the packed binary tree (also the any-hit tree), the leaf list and the greedy 4-wide form of that tree are the ones
// pt_bvh_build derived on the device (ptk::lbvh_trees_launch), borrowed from the node texture: a rebuild costs the
// GPU build with that stage and this decode, and nothing is packed on the host (DESIGN.md "Dynamic scenes").
int get_scene_lbvh(Texture* tris, Texture* nodes, SceneGPU& sg, SceneGPU** out) {
  const size_t ntris = tris->bytes / (45 * sizeof(float));
  const ptk::LbvhTrees* t = nodes->trees;
  if (!t || t->version != nodes->version) return err(PT_ERR_STATE, "GPU-built node buffer without its walk trees");
  // the reference walks with int stack[256] (path_tracing.frag:378); deeper trees are undefined there (pack_bvh)
  if (t->dev_info[1] >= kRefStack) return err(PT_ERR_FORMAT, "BVH deeper than the reference's stack[256]");
  drop_borrowed(sg);
  float4** own[4] = {&sg.bvh, &sg.bvh4, &sg.bvh_any, &sg.leaves};  // of a host-built scene these handles held before
  for (auto b : own)
    if (*b) { (void)hipFree(*b); *b = nullptr; }
  sg.lbvh = true;
  sg.bvh = sg.bvh_any = t->bin;
  sg.bvh4 = t->wide;
  sg.leaves = t->leaves;
  sg.nleaves = t->nleaves();
  sg.tri_shared = false;  // the LBVH's leaves are disjoint ranges of the Morton order
  const int root = t->dev_info[0];
  sg.stack_need = sg.need_any = t->dev_info[1];
  sg.root_any = root;
  sg.has4 = true;
  sg.nan4 = t->dev_info[6] != 0;
  sg.root4 = sg.root4c = t->dev_info[3];  // 0, or the leaf ref of a tree that is one leaf
  sg.need4 = t->dev_info[4];
  sg.fine_eye_limit = INFINITY;  // no fine boxes
  if (sg.geom) (void)hipFree(sg.geom);
  sg.geom = nullptr;
  free_shade(sg);
  const size_t shade_bytes = std::max<size_t>(ntris, 1) * 9 * sizeof(float4);
  HIPCHK(hipMalloc((void**)&sg.geom, std::max<size_t>(ntris, 1) * 4 * sizeof(float4)));
  HIPCHK(hipMalloc(&sg.shade.sb.buf, shade_bytes));
  sg.shade.sb.bytes = shade_bytes;
  TRY(materials_order(g.stream));  // the texels as every pt_materials_update so far left them
  HIPCHK((hipError_t)ptk::decode_tris((const float*)tris->dev, (int)ntris, sg.geom, (float4*)sg.shade.sb.buf,
                                      g.stream));
  HIPCHK(sg.shade.sb.mark_built(g.stream));  // for a pt_materials_update that follows: draws do not wait for it
  if (const int rc = build_tri_leaf(sg, (int)ntris)) return rc;
  sg.root_ref = root;
  sg.ntris = (int)ntris;
  sg.tri_ver = tris->version;
  sg.node_ver = nodes->version;
  *out = &sg;
  return PT_OK;
}

int get_scene(Texture* tris, uint32_t th, Texture* nodes, uint32_t nh, SceneGPU** out) {
  SceneGPU& sg = g.scenes[{th, nh}];
  if (sg.geom && sg.tri_ver == tris->version && sg.node_ver == nodes->version) {
    *out = &sg;
    return PT_OK;
  }
  using namespace glsl;
  size_t ntris = tris->host.size() / (45 * sizeof(float));
  size_t nnodes = nodes->host.size() / (12 * sizeof(float));
  if (tris->lbvh && nodes->lbvh) return get_scene_lbvh(tris, nodes, sg, out);
  drop_borrowed(sg);
  if (const int rc = refresh_host(tris)) return rc;  // a refitted buffer paired with a host-written one
  if (const int rc = refresh_host(nodes)) return rc;
  const float* te = (const float*)tris->host.data();
  std::vector<float4> geom(ntris * 4), shade(ntris * 9);
  for (size_t i = 0; i < ntris; ++i) {
    const float* f = te + i * 45;
    v3 p1 = mk(f[0], f[1], f[2]), p2 = mk(f[3], f[4], f[5]), p3 = mk(f[6], f[7], f[8]);
    v3 N = normalize(cross(sub(p2, p1), sub(p3, p1)));  // hitTriangle :227, same built-ins
    geom[4 * i + 0] = float4{p1.x, p1.y, p1.z, dot(N, p1)};
    geom[4 * i + 1] = float4{p2.x, p2.y, p2.z, 0.0f};
    geom[4 * i + 2] = float4{p3.x, p3.y, p3.z, 0.0f};
    geom[4 * i + 3] = float4{N.x, N.y, N.z, 0.0f};
    float4* s = &shade[9 * i];
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
  std::vector<Float4> bvh, bvh4;
  int root = 0, root4 = 0, need4 = 0, root4c = 0;
  std::string msg;
  int rc = pack_bvh((const float*)nodes->host.data(), (int)nnodes, bvh, &root, (int)ntris, &sg.stack_need, &msg);
  if (rc != PT_OK) return err(rc, msg);
  {  // optional: without it shadow and closest-hit rays walk the reference tree (binary, or its 4-wide form)
    std::vector<Float4> any;
    sg.has4 = false;
    float fine_mag = 0.0f;
    sg.fine_eye_limit = INFINITY;
    if (build_anyhit_tree((const float*)nodes->host.data(), (int)nnodes, (int)ntris, te, any, &sg.root_any,
                          &sg.need_any, &msg, &bvh4, &root4, &need4, &fine_mag, &root4c) == PT_OK) {
      if (fine_mag > 0.0f) sg.fine_eye_limit = kFineEyeReach * fine_mag;
      if (any.empty()) any.push_back(Float4{0, 0, 0, 0});
      if ((rc = upload_vec(any, &sg.bvh_any)) != PT_OK) return rc;
      if (bvh4.empty()) bvh4.push_back(Float4{0, 0, 0, 0});
      if ((rc = upload_vec(bvh4, &sg.bvh4)) != PT_OK) return rc;
      sg.has4 = true;
      sg.root4 = root4;
      sg.root4c = root4c;
      sg.nan4 = wide_has_nan(bvh4);
      sg.need4 = need4;
      if (getenv("PTSVGF_SCENE_INFO"))  // diagnostics: the walks' working set (DESIGN.md "The traversal in round 4")
        fprintf(stderr, "ptsvgf scene: %zu triangles (geometry %zu B, shading %zu B), reference tree %zu B, any-hit "
                        "tree %zu B, 4-wide tree %zu nodes = %zu B, stack need %d / %d / %d\n",
                (size_t)ntris, (size_t)ntris * 64, (size_t)ntris * 144, bvh.size() * sizeof(float4),
                any.size() * sizeof(float4), bvh4.size() / ptk::kWideStride, bvh4.size() * sizeof(float4),
                sg.stack_need, sg.need_any, need4);
    } else {
      for (float4** b : {&sg.bvh_any, &sg.bvh4})
        if (*b) { (void)hipFree(*b); *b = nullptr; }
      sg.need_any = sg.root_any = sg.need4 = sg.root4 = sg.root4c = 0;
    }
  }
  if ((rc = upload_leaves((const float*)nodes->host.data(), nnodes, sg)) != PT_OK) return rc;
  if ((rc = build_tri_leaf(sg, (int)ntris)) != PT_OK) return rc;
  if ((rc = upload_vec(geom, &sg.geom)) != PT_OK) return rc;
  free_shade(sg);
  {
    float4* sh = nullptr;
    if ((rc = upload_vec(shade, &sh)) != PT_OK) return rc;
    sg.shade.sb.buf = sh;
    sg.shade.sb.bytes = shade.size() * sizeof(float4);
  }
  if (bvh.empty()) bvh.push_back(Float4{0, 0, 0, 0});
  if ((rc = upload_vec(bvh, &sg.bvh)) != PT_OK) return rc;
  sg.root_ref = root;
  sg.ntris = (int)ntris;
  sg.tri_ver = tris->version;
  sg.node_ver = nodes->version;
  *out = &sg;
  return PT_OK;
}

}  // namespace

namespace ptapi {

int scene_of(Texture* tris, uint32_t th, Texture* nodes, uint32_t nh, SceneGPU** out) {
  return get_scene(tris, th, nodes, nh, out);
}

// Cost-ordered dispatch (TileSched): the launch records per-tile costs into o.cost and
// runs in the order the previous launch's costs gave (once one exists for this tile
// count); tile_order_finish then sorts the new costs for the next launch.
int tile_order_begin(Pass* p, int ntiles, TileSched* out) {
  TileOrder& o = p->order;
  memset(out, 0, sizeof(*out));
  if (ui(p, "tile_order", 1) == 0 || ntiles <= 0) return PT_OK;  // A/B switch: raster order
  if (o.n != ntiles) {
    if (o.cost) (void)hipFree(o.cost);
    if (o.perm) (void)hipFree(o.perm);
    o.cost = nullptr;
    o.perm = nullptr;
    o.n = 0;
    o.ordered = false;
    HIPCHK(hipMalloc((void**)&o.cost, (size_t)ntiles * 4));
    HIPCHK(hipMalloc((void**)&o.perm, (size_t)ntiles * 4));
    HIPCHK(hipMemsetAsync(o.cost, 0, (size_t)ntiles * 4, g.stream));
    o.n = ntiles;
  }
  out->cost = o.cost;
  out->perm = o.ordered ? o.perm : nullptr;
  out->perm_next = o.perm;
  out->ntiles = ntiles;
  return PT_OK;
}

int tile_order_finish(Pass* p, const TileSched& t) {
  if (!t.cost) return PT_OK;
  int rc = launch_tile_sort(p->order.cost, p->order.perm, p->order.n, g.stream);
  if (rc) return hip_err((hipError_t)rc, "tile order sort");
  p->order.ordered = true;
  return PT_OK;
}

// Scratch of a tile rasteriser (Bins, pt_device.h): allocated once per (items, band) size, its tile counts zeroed
// then (every later launch leaves them at zero: the scatter decrements each one it counted, an overflowed launch's
// fallback clears them); the counters are cleared per launch. `cap` > 0 lowers the pair list's capacity (tests).
int bins_for(RasterBins& b, int n, int W, int y0, int y1, int cap, Bins* out) {
  const int ntiles = ((W + kRTile - 1) / kRTile) * ((std::max(0, y1 - y0) + kRTile - 1) / kRTile);
  if (!b.base || b.ntris != n || b.ntiles != ntiles) {
    if (b.base) (void)hipFree(b.base);
    b = RasterBins{};
    const int pair_cap = (int)std::min<long long>(std::max<long long>(256LL * n, 1 << 22), 1 << 28);
    const int large_cap = std::max(n, 1);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_box = 0, o_tmin = o_box + up((size_t)std::max(n, 1) * 16),
                 o_cnt = o_tmin + up((size_t)std::max(n, 1) * 4), o_off = o_cnt + up((size_t)ntiles * 4),
                 o_pairs = o_off + up(((size_t)ntiles + 1) * 4), o_big = o_pairs + up((size_t)pair_cap * 4),
                 o_ctr = o_big + up((size_t)large_cap * 4), total = o_ctr + 256;
    HIPCHK(hipMalloc(&b.base, total));
    char* c = (char*)b.base;
    b.tri_box = (int4*)(c + o_box);
    b.tri_tmin = (float*)(c + o_tmin);
    b.tile_count = (int*)(c + o_cnt);
    b.tile_off = (int*)(c + o_off);
    b.pairs = (int*)(c + o_pairs);
    b.big = (int*)(c + o_big);
    b.ctr = (int*)(c + o_ctr);
    b.ntris = n;
    b.ntiles = ntiles;
    b.pair_cap = pair_cap;
    b.big_cap = large_cap;
    HIPCHK(hipMemsetAsync(b.tile_count, 0, (size_t)ntiles * 4, g.stream));
  }
  HIPCHK(hipMemsetAsync(b.ctr, 0, 16, g.stream));
  Bins& k = *out;
  k.n = n;
  k.box = b.tri_box;
  k.tmin = b.tri_tmin;
  k.tile_count = b.tile_count;
  k.tile_off = b.tile_off;
  k.pairs = b.pairs;
  k.pair_cap = cap > 0 ? std::min(b.pair_cap, cap) : b.pair_cap;
  k.large = b.big;
  k.large_cap = b.big_cap;
  k.ctr = b.ctr;
  k.W = W;
  k.y0 = y0;
  k.y1 = y1;
  return PT_OK;
}

}  // namespace ptapi

namespace {

// The int uniforms that the batched traversal launches take from the first pass of a batch, each with the default that
// holds when a pass never set it. Their readers (pt_params, pt_wf_setup, wf_fork) and the batch's agreement check
// (draw_pathtrace_batch) read them through these, so the check compares the value the draw uses.
struct Switch {
  const char* name;
  int dflt;
};
constexpr Switch kWideBvh{"wide_bvh", 1};
constexpr Switch kLbvhWide{"lbvh_wide", 1};
constexpr Switch kShadowBudget{"shadow_budget", 0};
constexpr Switch kClosestBudget{"closest_budget", 0};
constexpr Switch kTraceRefill{"trace_refill", 0};
constexpr Switch kRefillWaves{"refill_waves", 0};
constexpr Switch kRefillGrid{"refill_grid", 0};
constexpr Switch kListGrid{"list_grid", 0};
constexpr Switch kShadeFold{"shade_fold", 1};
constexpr Switch kTraceFork{"trace_fork", 0};
constexpr Switch kBatchSame[] = {kTraceRefill, kShadowBudget, kClosestBudget, kWideBvh,  kLbvhWide,
                                 kRefillWaves, kTraceFork,    kRefillGrid,    kListGrid, kShadeFold};
int sw(Pass* p, const Switch& s) { return ui(p, s.name, s.dflt); }

// uniform point_bins (default kPointBinsDefault; 0 for a scene built on the device: point_bins_for): 1 = the
// wavefront path tracer decides point-light shadow rays by the lights' triangle bins (wf_shadow_point_bins), 0 = they
// walk the tree with the HDR rays. Same bits either way.
constexpr int kPointBinsDefault = 1;
// uniform point_bins_settle: the path-tracing draws a moved light must stand before its lists are rebuilt (0: at the
// first draw after the move). 8 is a placeholder: the measured break-even of walking against rebuilding is about 27
// frames, with a spread too wide to adopt (DESIGN.md "Moving point lights").
constexpr int kPointBinsSettle = 8;
// The point-light bins of a path-tracing draw (PTParams::point_bins / pbins), built or rebuilt on the draw's stream
// when stale. Off (the rays walk) without 1 .. kPointBins lights all present in the lights buffer, or when a triangle
// sits in two leaves (the condition that keeps primary_raster at 2: tri_leaf names one leaf per triangle).
int point_bins_for(Pass* p, SceneGPU* sg, Texture* lt, uint32_t lh, PTParams& k, DrawReads& reads) {
  k.point_bins = 0;
  const int nl = k.pointLightSize;
  // A scene rebuilt on the device (pt_bvh_build) pays the bins' build with every rebuild, which costs about a frame
  // (DESIGN.md): there the default is 0. An explicit point_bins wins. (One frame at a time the bins measured slower,
  // so the renderer sets 0 then, beside its other settings that depend on the frames in flight.)
  const int dflt = sg->lbvh ? 0 : kPointBinsDefault;
  if (!ui(p, "point_bins", dflt) || ui(p, "pt_kernel", 0) != 0 || nl < 1 || nl > ptk::kPointBins ||
      !k.scene.lights || nl > k.scene.nlights_buf || !sg->tri_leaf || sg->tri_shared || !sg->leaves || sg->ntris <= 0)
    return PT_OK;
  const int R = std::min(ptk::kPointBinsMaxR, std::max(4, ui(p, "point_bins_r", kPointBinsR)));
  // point_bins_tight (default 1): list a triangle in the cells its projected polygon reaches; 0: in every cell of
  // the polygon's box (A/B; same verdicts, longer lists)
  const int tight = ui(p, "point_bins_tight", 1) ? 1 : 0;
  PointBinsGPU& m = sg->pbins;
  // the lights texture of the last build at a newer version, by pt_lights_update alone (only it keeps stamps): the
  // lights whose position stamp is newer are stale one by one, below; anything else rebuilds every light's lists
  const bool same_but_lights = m.sb.buf && m.tri_ver == sg->tri_ver && m.node_ver == sg->node_ver &&
                               m.ntris == sg->ntris && m.light_handle == lh && m.nl == nl && m.R == R && m.tight == tight;
  const bool updated = same_but_lights && reads.light_stamps && reads.light_count >= nl &&
                       (m.light_dev != lt->dev || m.light_ver != lt->version);
  const bool stale = !same_but_lights || (!updated && (m.light_dev != lt->dev || m.light_ver != lt->version));
  auto stamp_of = [&](int l) { return reads.light_stamps && l < reads.light_count ? reads.light_stamps[l] : 0; };
  if (stale) {
    const size_t need = ptk::point_bins_bytes(sg->ntris, nl, R, tight);
    HIPCHK(m.sb.renew(need));
    const int rc = ptk::launch_point_bins_build(k.scene, nl, R, tight, m.sb.buf, &m.dev, g.stream);
    if (rc) return hip_err((hipError_t)rc, "point-light bins build");
    HIPCHK(m.sb.mark_built(g.stream));
    m.tri_ver = sg->tri_ver;
    m.node_ver = sg->node_ver;
    m.ntris = sg->ntris;
    m.light_handle = lh;
    m.light_dev = lt->dev;
    m.light_ver = lt->version;
    m.nl = nl;
    m.R = R;
    m.tight = tight;
    for (int l = 0; l < ptk::kPointBins; ++l) {
      m.per_light[l] = ptk::LightBinsState{};
      m.per_light[l].built = m.per_light[l].seen = stamp_of(l);
    }
    if (getenv("PTSVGF_SCENE_INFO"))
      fprintf(stderr, "ptsvgf point-light bins: %d lights, R = %d, %zu B allocated (headers %zu B per light)\n", nl, R,
              need, (size_t)(6 * R * R + 1) * sizeof(int2));
  }
  TRY(read_shared(reads, m.sb));
  // Moving lights (DESIGN.md "Moving point lights"), once per draw and light (lights_key.h light_bins_step): a light
  // that moved is marked (info[l][0] = 2: its rays walk) and, once it has stood for point_bins_settle draws, gets its
  // lists rebuilt, alone and in place. Both write what the draws in flight on other streams read, so this stream
  // first waits for their recorded reads; draws issued later wait for this write's event as for a build. No host wait.
  if (same_but_lights && (updated || m.light_ver == lt->version)) {
    const int settle = std::max(0, ui(p, "point_bins_settle", kPointBinsSettle));
    bool wrote = false;
    for (int l = 0; l < nl; ++l) {
      const int act = ptk::light_bins_step(m.per_light[l], stamp_of(l), settle);
      if (act != ptk::kLbMark && act != ptk::kLbRebuild) continue;
      if (!wrote)
        for (auto& u : m.sb.uses)
          if (u.first != g.stream) HIPCHK(hipStreamWaitEvent(g.stream, u.second, 0));
      wrote = true;
      const int rc = act == ptk::kLbMark
                         ? ptk::launch_point_bins_mark_moved(m.dev, l, g.stream)
                         : ptk::launch_point_bins_rebuild_light(k.scene, nl, R, tight, m.sb.buf, l, g.stream);
      if (rc) return hip_err((hipError_t)rc, "point-light bins of a moved light");
    }
    if (wrote) HIPCHK(m.sb.mark_built(g.stream));
    m.light_dev = lt->dev;
    m.light_ver = lt->version;
  }
  k.point_bins = 1;
  k.pbins = m.dev;
  return PT_OK;
}

// ------------------------------------------------------------- draw calls ---
// PTParams of a path-tracing pass's draw from its uniforms, samplers and attachments (the wavefront state aside).
int pt_params(Pass* p, PTParams& k, SceneGPU*& sg, DrawReads& reads) {
  reads = DrawReads{};
  memset(&k, 0, sizeof(k));
  k.W = p->W;
  k.H = p->H;
  rows_of(p, &k.y0, &k.y1);
  TRY(att_plane(p, 0, &k.color));
  TRY(att_plane(p, 1, &k.emission));
  TRY(att_plane(p, 2, &k.albedo));
  uint32_t th, nh, lh;
  Texture* tt = sampler(p, "triangles", &th);
  Texture* nt = sampler(p, "nodes", &nh);
  Texture* lt = sampler(p, "pointLights", &lh);
  if (!tt || tt->target != PT_TEXTURE_BUFFER || !nt || nt->target != PT_TEXTURE_BUFFER)
    return err(PT_ERR_MISSING_TEXTURE, "path_tracing needs the 'triangles' and 'nodes' texture buffers");
  TRY(get_scene(tt, th, nt, nh, &sg));
  k.scene.tri_geom = sg->geom;
  k.scene.tri_shade = (const float4*)sg->shade.sb.buf;
  // pt_materials_update wrote it, on another stream; this version is read until noted
  if (sg->shade.edited()) TRY(read_shared(reads, sg->shade.sb));
  k.scene.bvh = sg->bvh;
  k.scene.root_ref = sg->root_ref;
  k.stack_need = sg->stack_need;
  const Uniform* e = U(p, "eye", 5);
  if (e) memcpy(k.eye, e->f, 12);
  // the any-hit / closest-hit SAH trees hold fine boxes padded for eyes within sg->fine_eye_limit (refine_leaves): an
  // eye further out walks the reference tree, whose boxes are the reference's own
  const bool eye_near = fabsf(k.eye[0]) <= sg->fine_eye_limit && fabsf(k.eye[1]) <= sg->fine_eye_limit &&
                        fabsf(k.eye[2]) <= sg->fine_eye_limit;
  // lbvh_wide (default kLbvhWide's): a scene pt_bvh_build wrote is walked through the 4-wide tree its device stage
  // derived (same bits; DESIGN.md "Dynamic scenes"); 0 = its binary tree alone, as before that stage existed. Its
  // any-hit tree is that same binary tree, so it is bound only for the 4-wide walk.
  const bool wide_on = sg->has4 && !(PT_WIDE_SIGNED && sg->nan4) && sw(p, kWideBvh) && (!sg->lbvh || sw(p, kLbvhWide));
  if (ui(p, "shadow_tree", 1) && eye_near && (!sg->lbvh || wide_on)) {  // A/B switch: 0 = shadow rays walk the reference tree
    k.scene.bvh_any = sg->bvh_any;
    k.scene.root_any = sg->root_any;
    k.stack_need = std::max(k.stack_need, sg->need_any);
  }
  // wide_bvh = 1 (default): the traversal kernels walk the 4-wide form of the any-hit tree: 28 % fewer node + triangle
  // visits, same bits. With the library built without the SLP vectorizer: 4K 197.7 / 198.9 -> 203.9 / 203.3 fps,
  // surface view 65.4 / 65.2 -> 67.3 / 67.1 (profiles/r03/wide_ab.log; with SLP it measured no faster)
  k.scene.bvh4 = (k.scene.bvh_any && wide_on) ? sg->bvh4 : nullptr;
  k.scene.root4 = sg->root4;
  k.scene.root4c = sg->root4c;
  k.scene.ntris = sg->ntris;
  k.scene.leaves = sg->leaves;
  k.scene.nleaves = sg->nleaves;
  k.scene.tri_leaf = sg->tri_leaf;
  if (lt && lt->target == PT_TEXTURE_BUFFER) {
    k.scene.lights = (const float*)lt->dev;
    k.scene.nlights_buf = (int)(lt->bytes / (6 * sizeof(float)));
    reads.light_handle = lh;
    reads.light_ver = lt->version;
    if (lt->lights) {  // pt_lights_update wrote it: this version's copy runs on another stream, and is read until noted
      TRY(read_shared(reads, lt->lights->sb));
      reads.light_stamps = lt->lights->pos_stamp.data();
      reads.light_count = (int)lt->lights->pos_stamp.size();
    }
  }
  // uniform sampler2DArray material_array (path_tracing.frag:331-364); unbound -> fetches read 0
  Texture* ma = sampler(p, "material_array");
  if (ma && ma->target == PT_TEXTURE_2D_ARRAY && ma->dev) {
    k.scene.texarr = (const uint32_t*)ma->dev;
    k.scene.tex_w = ma->W;
    k.scene.tex_h = ma->H;
    k.scene.tex_layers = ma->layers;
  }
  k.scene.use_normal_map = ui(p, "use_normal_map", 0);
  uint32_t hmh = 0, hch = 0;
  Texture* hm = sampler(p, "hdrMap", &hmh);
  Texture* hc = sampler(p, "hdrCache", &hch);
  if (!hm || !hc || !hm->dev || !hc->dev) return err(PT_ERR_MISSING_TEXTURE, "path_tracing needs hdrMap and hdrCache");
  k.hdr = Tex{(const float4*)hm->dev, hm->W, hm->H};
  reads.hdr_handle = hmh;
  reads.hdr_ver = hm->version;
  reads.cache_handle = hch;
  reads.cache_ver = hc->version;
  k.cache = Tex{(const float4*)hc->dev, hc->W, hc->H};
  k.hdr_pdf = Tex{nullptr, 0, 0};
  // pt_environment_update wrote them: the version's build runs on another stream, and is read until noted
  EnvVersions* ev = hm->env;
  if (ev && ev->sb.buf) TRY(read_shared(reads, ev->sb));
  if (hc->env && hc->env != ev && hc->env->sb.buf) TRY(read_shared(reads, hc->env->sb));  // (another pair's)
  // the pair as its last update left it (two whole 2-D textures of one size): the merged plane is the version's third
  const bool env_pair = ev && ev == hc->env && ev->sb.buf && hm->dev == ev->sb.buf &&
                        hc->dev == (const char*)ev->sb.buf + ev->plane() && ev->vh == hm->version &&
                        ev->vc == hc->version;
  // A/B switch hdr_merge (default 1): the NEE's radiance and pdf fetches at one direction from one merged texture
  if (ui(p, "hdr_merge", 1) && env_pair) {
    k.hdr_pdf = Tex{(const float4*)((const char*)ev->sb.buf + 2 * ev->plane()), hm->W, hm->H};
  } else if (ui(p, "hdr_merge", 1) && hm != hc && hm->W == hc->W && hm->H == hc->H && hm->target == PT_TEXTURE_2D &&
             hc->target == PT_TEXTURE_2D && hm->rows == hm->H && hc->rows == hc->H) {
    // Built on the draw's stream, read by the path tracers of every frame in flight on other streams (SharedBuf).
    // Staleness follows Texture::version, which uploads bump; a texture wrapped around external device memory
    // (pt_texture2d_wrap) is not tracked, so new contents there must be re-bound (a new handle) to be merged.
    HdrMerged& m = g.hdr_merged[{hmh, hch}];
    const bool stale = !m.sb.buf || m.W != hm->W || m.H != hm->H || m.hdr_dev != hm->dev || m.cache_dev != hc->dev ||
                       m.vh != hm->version || m.vc != hc->version;
    if (stale) {
      if (m.sb.buf && (m.W != hm->W || m.H != hm->H)) {  // a new size (rarer still): the old buffers go once idle
        HIPCHK(hipDeviceSynchronize());
        free_hdr_merged(m);
      }
      HIPCHK(m.sb.renew((size_t)hm->W * hm->H * sizeof(float4)));
      m.W = hm->W;
      m.H = hm->H;
      const int rc = ptk::launch_hdr_merge((const float4*)hm->dev, (const float4*)hc->dev, (float4*)m.sb.buf, m.W * m.H,
                                           g.stream);
      if (rc) return hip_err((hipError_t)rc, "hdr merge");
      HIPCHK(m.sb.mark_built(g.stream));
      m.hdr_dev = hm->dev;
      m.cache_dev = hc->dev;
      m.vh = hm->version;
      m.vc = hc->version;
    }
    TRY(read_shared(reads, m.sb));
    k.hdr_pdf = Tex{(const float4*)m.sb.buf, m.W, m.H};
  }
  k.hdrResolution = ui(p, "hdrResolution", hm->W);
  k.pointLightSize = ui(p, "pointLightSize", 0);
  TRY(point_bins_for(p, sg, lt, lh, k, reads));
  pt_counter_params(k, uu(p, "frameCounter", 0));  // and the bounces' Sobol points (spp_params.h)
  const Uniform* cr = U(p, "cameraRotate", 6);
  if (cr) memcpy(k.camRot, cr->f, 64);
  else { k.camRot[0] = k.camRot[5] = k.camRot[10] = k.camRot[15] = 1.0f; }
  k.accumulate = ui(p, "accumulate", 0);
  k.clamp_threshold = uf(p, "clamp_threshold", 0.0f);
  k.max_depth = ui(p, "max_tracing_depth", 0);
  if (k.max_depth > 4) return err(PT_ERR_ARG, "max_tracing_depth > 4 indexes past the 8 Sobol dimensions (:463)");
  k.aspect_corrected = ui(p, "aspect_corrected", 0);
  k.prune = ui(p, "prune", 1);
  // A/B switch: 1 = wavefront closest-hit rays walk bvh_any (ties re-walked on the reference tree)
  k.closest_tree = (k.prune && k.scene.bvh_any) ? ui(p, "closest_tree", 1) : 0;
  if (k.accumulate) {
    Texture* lf = sampler(p, "lastFrame");
    if (lf) TRY(plane_of(lf, p, &k.last, "lastFrame"));
  }
  // optional primary-ray bound from this frame's G-buffer (wf_primary), result-preserving
  Texture* hp = bound_sampler(p, "gWorldPos");
  Texture* hn = bound_sampler(p, "gNormalAndLinearZ");
  if (hp && hn && ui(p, "primary_bound", 1)) {
    TRY(plane_of(hp, p, &k.hint_pos, "gWorldPos"));
    TRY(plane_of(hn, p, &k.hint_nd, "gNormalAndLinearZ"));
    // the set's compact bound plane (written by the G-buffer draw, draw_raster) replaces the two-plane read when it
    // was formed for this pass's eye; bound_plane = 0 keeps the two-plane read (A/B, tests). A set without one
    // (adopted or uploaded planes, a draw without bound_eye) reads the two planes.
    if (!k.hint_pos.aux || !ui(p, "bound_plane", 1) || memcmp(hp->aux_eye, k.eye, sizeof(k.eye)) != 0)
      k.hint_pos.aux = nullptr;
  }
  // tile subset (PTParams::tile_stride): this pass traces every tile_stride-th 16 x 16 tile of the band
  k.tile_stride = ui(p, "tile_stride", 1);
  k.tile_offset = ui(p, "tile_offset", 0);
  if (wf_subset_tiles(k.W, std::max(0, k.y1 - k.y0), k.tile_stride, k.tile_offset) < 0)
    return err(PT_ERR_ARG, "tile_offset must lie in [0, tile_stride)");
  return PT_OK;
}

// The wavefront-side fields of a path-tracing pass's PTParams: its wavefront state `st` (its own, or its frame's
// share of a batch's), counters, budgets, refill, cost-ordered tiles and the primary rasteriser's bins.
// key / reuse (a draw of one pass: both, or neither): the primary-hit cache's key of this draw, and whether it may skip
// the stage.
int pt_wf_setup(Pass* p, PTParams& k, SceneGPU* sg, const WFState& st, ptk::PrimaryKey* key = nullptr,
                bool* reuse = nullptr) {
    k.wf = st;
    if (k.wf.spill) k.point_bins = 0;  // deep trees keep the walk (launch_wavefront<.., DEEP>)
    k.wf.row_cost = p->row_cost;
    k.wf.stats = p->stats;
    k.wf.stats_n = p->stats_n;
    // > 0: shadow rays past this many visits finish in the wave-cooperative walk (A/B switch; off: with frames
    // in flight it measured slower)
    k.wf.shadow_budget = (uint32_t)sw(p, kShadowBudget);
    // > 0: bounce rays past this many visits finish in the wave-cooperative closest-hit walk (refill kernel only)
    k.wf.closest_budget = (uint32_t)sw(p, kClosestBudget);
    // percent of the bounce / shadow lists traced by lane-refill waves: 75 pays with frames in flight (the renderer
    // sets it then), 0 (default) keeps the shortest single-frame latency
    k.refill = std::min(100, std::max(0, sw(p, kTraceRefill)));
    k.refill_waves = std::max(0, sw(p, kRefillWaves));
    k.refill_grid = std::max(0, sw(p, kRefillGrid));
    k.list_grid = std::max(0, sw(p, kListGrid));
    // 1: paths end in place (no wf_finalize, no wf_finish between two shades); 0 keeps those launches (A/B, tests)
    k.shade_fold = sw(p, kShadeFold) != 0;
    const int ntiles = wf_subset_tiles(k.W, std::max(0, k.y1 - k.y0), k.tile_stride, k.tile_offset);  // wf_primary's grid
    TRY(tile_order_begin(p, ntiles, &k.tiles));
    // primary rays by tile-binned rasterisation: 1 = of the reference leaves, 2 = of the triangles; 0 = the per-pixel
    // walk. The items are binned to every tile of the band, a tile subset rasterises its own tiles
    const int pr = ui(p, "primary_raster", kPrimaryRasterDefault);
    // (the triangle rasteriser packs pixel coordinates into 16 bits)
    const bool tri = pr == 2 && !sg->tri_shared && k.W <= 65536 && k.H <= 65536;
    k.primary_raster = pr ? (tri ? 2 : 1) : 0;
    const int pair_cap = ui(p, "raster_pair_cap", 0);
    if (reuse) {
      // the primary-hit cache: a draw whose key equals that of the pass's last stage skips the stage, and with it the
      // bins' scratch (DESIGN.md "Static view"). The stage runs whenever its counters are asked for.
      *key = primary_key(p, k, sg, pair_cap);
      const bool bypass = p->stats || p->row_cost || ui(p, "primary_cache", 1) == 0;
      *reuse = ptk::primary_cache_hit(p->pcache, *key, bypass);
      if (*reuse) return PT_OK;
    }
    if (pr) TRY(bins_for(p->bins, tri ? sg->ntris : sg->nleaves, k.W, k.y0, k.y1, pair_cap, &k.leaf_bins));
    return PT_OK;
}

// The side stream and events of path-tracing draws issued on `s` (uniform trace_fork = 1), created on first use: one
// per draw stream, so frames in flight on different streams do not queue behind each other's shadow walks. An entry
// lives until its stream is released (pt_stream_release, which the host's stream pool calls when a renderer gives a
// stream back: ptsvgf.renderer.release_stream) or pt_shutdown, so a handle value a new stream reuses starts afresh.
const ptk::WfFork* wf_fork(Pass* p, hipStream_t s, int* rc) {
  *rc = PT_OK;
  if (!sw(p, kTraceFork)) return nullptr;
  auto it = g.forks.find(s);
  if (it != g.forks.end()) return &it->second;
  ptk::WfFork f{};
  // the side stream runs on the draw stream's CUs (pt_stream_create_cu_masked): a CU mask that keeps CUs free of the
  // traversal launches must hold for the forked walk too
  hipError_t e = hipSuccess;
  int ncu = 0;
  uint32_t mask[16] = {};
  bool masked = false;
  if (s && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, g.device) == hipSuccess && ncu > 0 &&
      ncu <= 512 && hipExtStreamGetCUMask(s, (uint32_t)((ncu + 31) / 32), mask) == hipSuccess)
    for (int i = 0; i < ncu; ++i) masked = masked || !((mask[i / 32] >> (i % 32)) & 1u);
  // and at the draw stream's queue priority (pt_stream_create_priority)
  int prio = 0;
  if (s) (void)hipStreamGetPriority(s, &prio);
  if (masked) e = hipExtStreamCreateWithCUMask(&f.side, (uint32_t)((ncu + 31) / 32), mask);
  else e = hipStreamCreateWithPriority(&f.side, hipStreamNonBlocking, prio);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&f.fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&f.join, hipEventDisableTiming);
  if (e != hipSuccess) {
    if (f.side) (void)hipStreamDestroy(f.side);
    if (f.fork) (void)hipEventDestroy(f.fork);
    *rc = hip_err(e, "trace_fork side stream");
    return nullptr;
  }
  return &(g.forks[s] = f);
}

// Samples per pixel of a path-tracing pass's draw (int uniform spp, default 1): 1 .. kMaxBatch, checked before
// anything is launched or bound for the draw.
int pass_spp(Pass* p, int* spp) {
  *spp = ui(p, "spp", 1);
  if (*spp >= 1 && *spp <= kMaxBatch) return PT_OK;
  return err(PT_ERR_ARG, "spp must lie in 1 .. 8 (samples per pixel per draw)");
}

// An spp draw (spp = n > 1): the n samples as the frames of a batch over one primary hit (launch_wavefront).
int draw_pathtrace_spp(Pass* p, PTParams& k, SceneGPU* sg, int n) {
  const int rows = std::max(0, k.y1 - k.y0);
  // state for every sample; a pass that also heads frame batches keeps one size for both uses
  const int nb = std::max(n, std::min(kMaxBatch, ui(p, "trace_batch", 1)));
  TRY(wf_alloc(p->wf, k.W, rows, nb, n));
  if (wf_spill(p->wf, k.stack_need) != PT_OK) return err(PT_ERR_HIP, "spill stack allocation failed");
  ptk::PrimaryKey key;
  bool reuse = false;  // sample 0's stage is the draw's: the cache serves it as it serves a one-sample draw
  TRY(pt_wf_setup(p, k, sg, p->wf.stb[0], &key, &reuse));
  PTParams ks[kMaxBatch];
  for (int s = 0; s < n; ++s) spp_sample_params(k, n, s, p->wf.stb[s], p->wf.spp, &ks[s]);
  ptk::SppResolve rs{};
  rs.n = n;
  rs.samples = p->wf.spp;
  rs.stride = p->wf.n;
  rs.color = k.color;
  rs.last = k.last;
  rs.accumulate = k.accumulate;
  rs.frameCounter = k.frameCounter;
  rs.W = k.W;
  rs.y0 = k.y0;
  rs.y1 = k.y1;
  rs.tile_stride = k.tile_stride;
  rs.tile_offset = k.tile_offset;
  if (p->sample_moments && (!k.emission.p || !k.albedo.p))
    return err(PT_ERR_ARG, "sample moments need the pass's emission and albedo attachments");
  const ptk::SppAdaptive ad{p->sample_counts, p->sample_stats, p->sample_moments, k.emission, k.albedo};
  int rc;
  const ptk::WfFork* fk = wf_fork(p, g.stream, &rc);
  if (rc) return rc;
  // (the samples would share one verdict word: the cache is bypassed; sample 0's stage still serves the primary cache)
  static_view_off(p, ptk::kFhrSpp, true);
  rc = launch_pathtrace_wavefront_spp(ks, rs, g.stream, fk, &ad, reuse);
  primary_cache_note(p, key, reuse, rc == 0);
  if (!rc && k.tiles.cost) p->order.ordered = true;
  return rc ? hip_err((hipError_t)rc, "pathtrace spp launch") : PT_OK;
}

}  // namespace

namespace ptapi {

int draw_pathtrace(Pass* p) {
  int spp;
  TRY(pass_spp(p, &spp));
  if (spp > 1 && ui(p, "pt_kernel", 0) != 0)
    return err(PT_ERR_ARG, "spp > 1 needs the wavefront path tracer (pt_kernel = 0)");
  // the count, statistics and moments planes hold whole frames in global rows; a band partition's planes do not
  if (spp > 1 && (p->sample_counts || p->sample_stats || p->sample_moments) && band_partition(p->W, p->H))
    return err(PT_ERR_STATE, "sample counts / statistics / moments cannot be bound under a pt_set_band partition");
  PTParams k;
  SceneGPU* sg = nullptr;
  DrawReads reads;
  StaticView sv;
  sv.before(p);  // (pt_params' att_plane makes the attachments' stamps fresh)
  TRY(pt_params(p, k, sg, reads));
  int rc;
  if (spp > 1) {
    TRY(draw_pathtrace_spp(p, k, sg, spp));
    return note_reads(reads);
  }
  if (ui(p, "pt_kernel", 0) == 1) {  // 1: single megakernel (kernels_pt.hip), kept for A/B
    if (k.tile_stride != 1) return err(PT_ERR_ARG, "tile subsets need the wavefront path tracer");
    if (k.stack_need >= kStack)
      return err(PT_ERR_ARG, "the megakernel (pt_kernel=1) walks a 32-entry LDS stack; this BVH is deeper: use the "
                             "wavefront path tracer (pt_kernel=0, the default)");
    static_view_off(p, ptk::kFhrMegakernel, false);  // (it sorts the pass's tile order by its own costs)
    rc = launch_pathtrace(k, g.stream);
  } else {                            // 0: wavefront (kernels_wavefront.hip, kernels_wf_*.hip), production
    TRY(wf_alloc(p->wf, k.W, std::max(0, k.y1 - k.y0)));
    if (wf_spill(p->wf, k.stack_need) != PT_OK) return err(PT_ERR_HIP, "spill stack allocation failed");
    TRY(pt_wf_setup(p, k, sg, p->wf.st, &sv.key, &sv.reuse));
    const ptk::WfFork* fk = wf_fork(p, g.stream, &rc);
    if (rc) return rc;
    TRY(sv.setup(p, k, sg, reads));
    rc = sv.forget ? ptk::launch_point_cache_forget(k.wf.pcache, p->wf.n, sv.forget, g.stream) : 0;
    if (!rc) rc = launch_pathtrace_wavefront(k, g.stream, fk, sv.reuse);
    sv.finish(p, k, reads, rc);
    if (!rc && k.tiles.cost) p->order.ordered = true;
  }
  if (rc) return hip_err((hipError_t)rc, "pathtrace launch");
  return note_reads(reads);
}

// pt_pass_draw_batch: the frames of several path-tracing passes in one wavefront run whose list-driven traversals
// trace every frame's rays per launch. The first pass owns the shared state, sized for its "trace_batch" frames.
int draw_pathtrace_batch(Pass** ps, int n) {
  Pass* h = ps[0];
  PTParams k[kMaxBatch];
  DrawReads reads[kMaxBatch];
  SceneGPU* sg = nullptr;
  for (int b = 0; b < n; ++b) {  // before the first pass's parameters launch or bind anything
    int spp;
    TRY(pass_spp(ps[b], &spp));
    if (spp > 1) return err(PT_ERR_ARG, "a pass with spp > 1 cannot be part of a batch: its samples are its batch");
  }
  for (int b = 0; b < n; ++b) {
    SceneGPU* sb = nullptr;
    TRY(pt_params(ps[b], k[b], sb, reads[b]));
    if (b == 0) sg = sb;
    // the batched traversal launches take their lane-refill share and visit budgets from passes[0] (pt_wf_setup
    // sets k[b].refill and the budgets from these uniforms later): every pass of the batch must agree on them, each
    // compared at its effective value (kBatchSame: the default its reader applies when a pass never set it)
    bool agree = true;
    for (const Switch& u : kBatchSame) agree = agree && sw(ps[b], u) == sw(ps[0], u);
    if (sb != sg || k[b].W != k[0].W || k[b].y0 != k[0].y0 || k[b].y1 != k[0].y1 || k[b].max_depth != k[0].max_depth ||
        k[b].scene.bvh_any != k[0].scene.bvh_any || !agree)
      return err(PT_ERR_ARG, "a path-tracing batch needs one scene, size, band, depth and traversal settings");
    // a tile subset (tile_stride / tile_offset) is batched as a whole frame is, provided every frame traces the same
    // subset: the per-frame launches (primaries, bounce-0 shade, finalize) are sized by that subset's tile count
    if (ui(ps[b], "pt_kernel", 0) != 0 || k[b].accumulate || k[b].tile_stride != k[0].tile_stride ||
        k[b].tile_offset != k[0].tile_offset)
      return err(PT_ERR_ARG, "a path-tracing batch needs the wavefront path tracer, one tile subset, no accumulation");
  }
  const int cap = std::max(n, std::min(kMaxBatch, ui(h, "trace_batch", n)));
  TRY(wf_alloc(h->wf, k[0].W, std::max(0, k[0].y1 - k[0].y0), cap));
  if (wf_spill(h->wf, k[0].stack_need) != PT_OK) return err(PT_ERR_HIP, "spill stack allocation failed");
  // A batch always runs the stage, into the head pass's planes, and sorts every pass's tile order: no pass keeps a key
  // that claims a plane or an order this draw changed. Each counts as a draw that ran the stage.
  for (int b = 0; b < n; ++b) static_view_off(ps[b], ptk::kFhrBatch, false);
  for (int b = 0; b < n; ++b) TRY(pt_wf_setup(ps[b], k[b], sg, h->wf.stb[b]));
  // the batched shadow launches read frame 0's point-light bins for every frame: frames that do not share them (other
  // lights, another pointLightSize) all walk
  bool same_bins = true;
  for (int b = 1; b < n; ++b)
    same_bins = same_bins && k[b].point_bins == k[0].point_bins && k[b].pbins.hdr == k[0].pbins.hdr &&
                k[b].pbins.nl == k[0].pbins.nl;
  for (int b = 0; b < n && !same_bins; ++b) k[b].point_bins = 0;
  int rc;
  const ptk::WfFork* fk = wf_fork(h, g.stream, &rc);
  if (rc) return rc;
  rc = launch_pathtrace_wavefront_batch(k, n, g.stream, fk);
  for (int b = 0; b < n && !rc; ++b) {
    if (k[b].tiles.cost) ps[b]->order.ordered = true;
    ps[b]->pcache.runs++;
  }
  if (rc) return hip_err((hipError_t)rc, "pathtrace batch launch");
  for (int b = 0; b < n; ++b) TRY(note_reads(reads[b]));
  return PT_OK;
}

}  // namespace ptapi

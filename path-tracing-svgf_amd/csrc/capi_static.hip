// capi_static.hip — the static view's host-side bookkeeping (DESIGN.md "Static view", parts 1 to 4): the key builders
// of static_key.h's keys, what a path-tracing draw does with the primary-hit cache, the verdict cache and the keep
// mode (StaticView), the static background's quiet-tile sets and per-draw decision (BgDraw), and the diagnostics of
// include/ptsvgf_debug_static.h, _background.h and _firsthit.h. Host code only, over the library state of
// capi_state.h; the draws that use it are those of capi_draw_pt.hip and capi_draw_svgf.hip.
#include "../../include/ptsvgf_debug_background.h"
#include "../../include/ptsvgf_debug_firsthit.h"
#include "../../include/ptsvgf_debug_static.h"
#include "capi_state.h"

using namespace ptapi;
using namespace ptk;

namespace ptapi {

// The key of what the primary stage of the draw `k` of pass p reads (static_key.h; k complete but for leaf_bins,
// which is scratch): the view, the rows and tiles, the walk settings as the draw uses them, the scene and the trees
// bound from it, the plane the stage writes and the tile order it sorts. Not in it: frameCounter (the stage does not
// read it) and the G-buffer hint planes (the bound only prunes the walk; DESIGN.md "The primary's bound as one float").
ptk::PrimaryKey primary_key(const Pass* p, const PTParams& k, const SceneGPU* sg, int pair_cap) {
  PrimaryKey q{};
  for (int i = 0; i < 3; ++i) q.w[kPkEye0 + i] = key_bits(k.eye[i]);
  for (int i = 0; i < 16; ++i) q.w[kPkCamRot0 + i] = key_bits(k.camRot[i]);
  q.w[kPkW] = key_bits(k.W);
  q.w[kPkH] = key_bits(k.H);
  q.w[kPkY0] = key_bits(k.y0);
  q.w[kPkY1] = key_bits(k.y1);
  q.w[kPkBandW] = key_bits(g.band_w);
  q.w[kPkBandH] = key_bits(g.band_h);
  q.w[kPkBandY0] = key_bits(g.band_y0);
  q.w[kPkBandY1] = key_bits(g.band_y1);
  q.w[kPkBandRow0] = key_bits(g.band_row0);
  q.w[kPkBandRows] = key_bits(g.band_rows);
  q.w[kPkTileStride] = key_bits(k.tile_stride);
  q.w[kPkTileOffset] = key_bits(k.tile_offset);
  q.w[kPkAspectCorrected] = key_bits(k.aspect_corrected);
  q.w[kPkPrune] = key_bits(k.prune);
  q.w[kPkClosestTree] = key_bits(k.closest_tree);
  q.w[kPkPrimaryRaster] = key_bits(k.primary_raster);
  q.w[kPkScene] = key_bits((const void*)sg);
  q.w[kPkTriVer] = sg->tri_ver;
  q.w[kPkNodeVer] = sg->node_ver;
  q.w[kPkNtris] = key_bits(sg->ntris);
  q.w[kPkTriGeom] = key_bits((const void*)k.scene.tri_geom);
  q.w[kPkBvh] = key_bits((const void*)k.scene.bvh);
  q.w[kPkRootRef] = key_bits(k.scene.root_ref);
  q.w[kPkBvhAny] = key_bits((const void*)k.scene.bvh_any);
  q.w[kPkRootAny] = key_bits(k.scene.root_any);
  q.w[kPkBvh4] = key_bits((const void*)k.scene.bvh4);
  q.w[kPkRoot4] = key_bits(k.scene.root4);
  q.w[kPkRoot4c] = key_bits(k.scene.root4c);
  q.w[kPkLeaves] = key_bits((const void*)k.scene.leaves);
  q.w[kPkNleaves] = key_bits(k.scene.nleaves);
  q.w[kPkTriLeaf] = key_bits((const void*)k.scene.tri_leaf);
  q.w[kPkStackNeed] = key_bits(k.stack_need);
  q.w[kPkSpill] = key_bits((const void*)k.wf.spill);
  q.w[kPkPairCap] = key_bits(pair_cap);
  q.w[kPkPlane] = key_bits((const void*)k.wf.hit0);
  q.w[kPkPlaneGen] = p->wf.gen;
  q.w[kPkTileCost] = key_bits((const void*)k.tiles.cost);
  q.w[kPkTilePerm] = key_bits((const void*)k.tiles.perm_next);
  return q;
}

// The key of a draw of the rasterize pass p over the triangles of src (static_key.h), read from the state as it is
// now: before a draw it is compared with the key taken after the pass's last completed draw. Returns false when an
// attachment is missing (the draw then reports it).
bool gbuf_key(Pass* p, const Pass* src, ptk::GbufKey* out) {
  GbufKey q{};
  if (p->att.size() < 4) return false;
  int y0, y1;
  rows_of(p, &y0, &y1);
  q.w[kGkW] = key_bits(p->W);
  q.w[kGkH] = key_bits(p->H);
  q.w[kGkY0] = key_bits(y0);
  q.w[kGkY1] = key_bits(y1);
  q.w[kGkBandW] = key_bits(g.band_w);
  q.w[kGkBandH] = key_bits(g.band_h);
  q.w[kGkBandY0] = key_bits(g.band_y0);
  q.w[kGkBandY1] = key_bits(g.band_y1);
  q.w[kGkBandRow0] = key_bits(g.band_row0);
  q.w[kGkBandRows] = key_bits(g.band_rows);
  for (int i = 0; i < 4; ++i) {
    const Texture* t = tex_of(p->att[i]);
    if (!t) return false;
    q.w[kGkAtt0 + 4 * i] = p->att[i];
    q.w[kGkAtt0 + 4 * i + 1] = key_bits((const void*)t->dev);
    q.w[kGkAtt0 + 4 * i + 2] = t->version;
    q.w[kGkAtt0 + 4 * i + 3] = t->raster_stamp;
  }
  const Texture *wt = tex_of(p->att[0]), *fwt = tex_of(p->att[3]);
  q.w[kGkFwAux] = key_bits((const void*)fwt->aux);
  q.w[kGkFwAuxValid] = fwt->aux_valid;
  q.w[kGkBoundAux] = key_bits((const void*)wt->aux);
  q.w[kGkBoundAuxValid] = wt->aux_valid;
  for (int i = 0; i < 3; ++i) q.w[kGkAuxEye0 + i] = key_bits(wt->aux_eye[i]);
  if (const Uniform* be = U(p, "bound_eye", 5)) {
    q.w[kGkBoundEyeSet] = 1;
    for (int i = 0; i < 3; ++i) q.w[kGkBoundEye0 + i] = key_bits(be->f[i]);
  }
  const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // (draw_raster's defaults)
  const Uniform *uv = U(p, "view", 6), *up = U(p, "projection", 6), *upv = U(p, "pre_viewproj", 6);
  for (int i = 0; i < 16; ++i) {
    q.w[kGkView0 + i] = key_bits(uv ? uv->f[i] : I[i]);
    q.w[kGkProj0 + i] = key_bits(up ? up->f[i] : I[i]);
    q.w[kGkPreViewProj0 + i] = key_bits(upv ? upv->f[i] : I[i]);
  }
  const RasterScene& rs = src->raster;
  const bool motion = rs.disp && rs.ntris > 0 && ui(p, "object_motion", 1) != 0;
  q.w[kGkDisp] = key_bits((const void*)(motion ? rs.disp : nullptr));
  q.w[kGkMode] = key_bits(ui(p, "gbuffer_mode", 1));
  q.w[kGkPairCap] = key_bits(ui(p, "raster_pair_cap", 0));
  q.w[kGkTileFlags] = key_bits(ui(p, "atrous_tile_flags", 1));
  q.w[kGkTfRows0] = key_bits(ui(p, "atrous_rows_begin", -1));
  q.w[kGkTfRows1] = key_bits(ui(p, "atrous_rows_end", -1));
  q.w[kGkTflags] = key_bits((const void*)fwt->tflags);
  q.w[kGkTflagsCap] = fwt->tflags_cap;
  q.w[kGkTflagsVer] = fwt->tflags_ver;
  q.w[kGkTflagsY0] = key_bits(fwt->tflags_y0);
  q.w[kGkTflagsY1] = key_bits(fwt->tflags_y1);
  q.w[kGkSource] = p->raster_src;
  q.w[kGkSceneVer] = rs.version;
  *out = q;
  return true;
}

// PTSVGF_STATIC_REUSE=0 in the environment forces every reuse_static off (A/B)
static bool reuse_static_env_off() {
  static const bool env_off = [] {
    const char* e = getenv("PTSVGF_STATIC_REUSE");
    return e && atoi(e) == 0;
  }();
  return env_off;
}
// reuse_static (int uniform of a rasterize pass, default 0): the caller states that nothing outside the library writes
// this pass's attachments between its draws. PTSVGF_STATIC_REUSE=0 in the environment forces it off (A/B).
bool reuse_static_on(Pass* p) {
  return !reuse_static_env_off() && ui(p, "reuse_static", 0) != 0;
}

// ---- what a path-tracing draw does with the caches (StaticView, capi_state.h). First, after the launch of a draw that
// pt_wf_setup gave a key: the primary-hit cache's state and counts
void primary_cache_note(Pass* p, const ptk::PrimaryKey& key, bool reused, bool ok) {
  if (reused) {
    if (ok) p->pcache.reuses++;
    return;  // (a failed launch wrote nothing into hit0)
  }
  p->busy_valid = false;  // the busy-tile list is that of the stage before this one
  p->pcache.valid = ok;
  if (ok) {
    p->pcache.key = key;
    p->pcache.runs++;
  }
}

// The bounce-0 point-light verdict cache of a one-sample wavefront draw (DESIGN.md "Static view, part 2"), after
// pt_wf_setup: the cache's key of this draw (the primary key and what the bounce-0 shadow ray reads beyond it) and the
// draw's mode, into k.point_cache. The draw's caller notes the outcome (ptk::point_cache_note).
// *forgets: the draw uses the cache after forgetting the lights of *forget (the mask may be 0: a colour-only update).
static LightsKey point_cache_mode_for(Pass* p, PTParams& k, const PrimaryKey& pkey, bool stage_reused,
                                      const DrawReads& reads, bool* forgets, uint32_t* forget) {
  LightsKey q = key_headed<LightsKey>(pkey);
  q.w[kLkLightHandle] = reads.light_handle;
  q.w[kLkLightDev] = key_bits((const void*)k.scene.lights);
  q.w[kLkLightVer] = reads.light_ver;
  q.w[kLkPointLightSize] = key_bits(k.pointLightSize);
  q.w[kLkNlightsBuf] = key_bits(k.scene.nlights_buf);
  q.w[kLkPointBins] = key_bits(k.point_bins);
  q.w[kLkPointBinsDev] = key_bits((const void*)(k.point_bins ? k.pbins.hdr : nullptr));
  q.w[kLkPlane] = key_bits((const void*)k.wf.pcache);
  // (the counters of shadow_point_rays must stay what they are when statistics are asked for; launch_wavefront
  // engages the cache only where its shades are folded, `shade_fold && max_depth > 0`: a draw of no bounce launches
  // no shade at all, so it must not count as the draw that reset the plane)
  const bool fold = k.shade_fold && k.max_depth > 0;
  const bool bypass = ui(p, "point_cache", 1) == 0 || p->stats || p->row_cost || k.pointLightSize < 1 ||
                      k.pointLightSize > kPcLights || k.wf.spill || !fold;
  // a lights buffer that pt_lights_update moved on forgets the moved lights' bits instead of resetting every word
  // (lights_key.h); a texture without stamps (never updated) has no lights to name: it resets as ever
  *forget = 0;
  bool fg = false;
  k.point_cache = point_cache_mode_lights(p->lcache, q, stage_reused, bypass, &fg);
  if (fg && !reads.light_stamps) {
    k.point_cache = kPcReset;
    fg = false;
  }
  *forgets = fg;
  if (fg) *forget = lights_moved_mask(reads.light_stamps, std::min(reads.light_count, (int)kPcLights),
                                      p->lcache.key.w[kLkLightVer]);
  return q;
}

// The key of the draw's miss texels (static_key.h MissKey), of a one-sample draw
static MissKey miss_key_of(const PTParams& k, const PrimaryKey& key, const DrawReads& reads) {
  MissKey m = key_headed<MissKey>(primary_content(key));
  m.w[kMkHdrHandle] = reads.hdr_handle;
  m.w[kMkHdrDev] = key_bits((const void*)k.hdr.p);
  m.w[kMkHdrVer] = reads.hdr_ver;
  m.w[kMkHdrW] = key_bits(k.hdr.W);
  m.w[kMkHdrH] = key_bits(k.hdr.H);
  m.w[kMkCacheHandle] = reads.cache_handle;
  m.w[kMkCacheDev] = key_bits((const void*)k.cache.p);
  m.w[kMkCacheVer] = reads.cache_ver;
  m.w[kMkMerged] = k.hdr_pdf.p != nullptr;
  m.w[kMkClamp] = key_bits(k.clamp_threshold);
  m.w[kMkAccumulate] = key_bits(k.accumulate);
  m.w[kMkMaxDepth] = key_bits(k.max_depth);
  m.w[kMkShadeFold] = k.shade_fold;
  m.w[kMkSpp] = 1;
  return m;
}
// The static background (DESIGN.md "Static view, part 3"), after a one-sample wavefront draw of the whole frame without
// accumulation: the colour attachment's miss texels are the content of the draw's MissKey (static_key.h), whichever
// slot's plane this is; the texture also remembers the draw's primary content and whose hit0 holds its primary hits,
// for the quiet-tile flags. Any other path-tracing draw leaves the stamp att_plane made: fresh.
static void bg_note_colour(Pass* p, const PTParams& k, const PrimaryKey& key, const DrawReads& reads) {
  Texture* ct = tex_of(p->att[0]);
  if (!ct || k.accumulate || k.y0 != 0 || k.y1 != k.H || k.tile_stride != 1 || band_partition(k.W, k.H) ||
      ct->row0 != 0 || ct->rows != k.H || !k.wf.hit0)
    return;
  const PrimaryKey pc = primary_content(key);
  const MissKey m = miss_key_of(k, key, reads);
  ct->bg = BgStamp{g.bg_miss.of(m.w, kMkWords, &g.bg_serial), kBgWhole};
  ct->bg_prim = g.bg_prim.of(pc.w, kPkWords, &g.bg_serial);
  ct->bg_pass = p;
  ct->bg_pass_gen = p->wf.gen;
}

// The bounce-0 shade's keep mode (DESIGN.md "Static view, part 4") of a one-sample wavefront draw.
// What the three attachments say before the draw: read before pt_params, whose att_plane renews all of it.
void StaticView::before(Pass* p) {
  Texture* t[3] = {nullptr, nullptr, nullptr};
  for (size_t i = 0; i < 3 && i < p->att.size(); ++i) t[i] = tex_of(p->att[i]);
  if (t[0]) colour = t[0]->bg;
  if (t[1]) emission = t[1]->first_hit;
  if (t[2]) albedo = t[2]->first_hit;
}
// After pt_wf_setup: the draw's mode, and for a draw that is not bypassed the content id of its FirstHitKey in *first.
// A kept draw gets k.busy, the pass's busy-tile list, built here on the draw's stream when the primary stage ran since
// it was last built; in the verdict cache's reset mode the words of the pixels the kept draw does not visit are
// cleared here instead (a fresh word is 0).
static int first_hit_mode_for(Pass* p, PTParams& k, const SceneGPU* sg, const PrimaryKey& key, bool stage_reused,
                              const DrawReads& reads, const StaticView& before, uint64_t* first) {
  *first = 0;
  uint32_t bypass = 0;
  auto by = [&](bool c, int r) { if (c) bypass |= 1u << r; };
  bool whole = k.y0 == 0 && k.y1 == k.H && !band_partition(k.W, k.H);
  for (int i = 0; i < 3; ++i) {
    const Texture* t = tex_of(p->att[i]);
    whole = whole && t && t->row0 == 0 && t->rows == k.H;
  }
  by(ui(p, "reuse_static", 0) == 0, kFhrUniform);
  by(reuse_static_env_off(), kFhrEnv);
  by(p->stats || p->row_cost, kFhrStats);
  by(k.tile_stride != 1, kFhrTiles);
  by(!whole, kFhrRows);
  by(k.wf.spill != nullptr, kFhrDeep);
  by(!k.shade_fold, kFhrUnfolded);
  by(k.max_depth <= 0, kFhrDepth0);
  by(k.accumulate != 0, kFhrAccumulate);
  uint64_t miss = 0;
  if (!bypass) {
    const MissKey m = miss_key_of(k, key, reads);
    miss = g.bg_miss.of(m.w, kMkWords, &g.bg_serial);
    FirstHitKey f = key_headed<FirstHitKey>(primary_content(key));
    f.w[kFkTriShade] = key_bits((const void*)k.scene.tri_shade);
    // the texture version the records were decoded at with the count of pt_materials_update calls since the library
    // began (neither comes near 2^32): a retired version taken again has the same pointer and other contents
    f.w[kFkTriShadeVer] = sg->tri_ver + (sg->shade_ver << 32);
    uint32_t mh = 0;
    const Texture* ma = sampler(p, "material_array", &mh);
    if (k.scene.texarr && ma) {
      f.w[kFkMatHandle] = mh;
      f.w[kFkMatDev] = key_bits((const void*)k.scene.texarr);
      f.w[kFkMatVer] = ma->version;
      f.w[kFkMatW] = key_bits(k.scene.tex_w);
      f.w[kFkMatH] = key_bits(k.scene.tex_h);
      f.w[kFkMatLayers] = key_bits(k.scene.tex_layers);
    }
    *first = g.bg_first.of(f.w, kFkWords, &g.bg_serial);
  }
  p->fh_mode = first_hit_mode(bypass, stage_reused, before.colour, before.emission, before.albedo, miss, *first,
                              &p->fh_reason);
  if (p->fh_mode != kFhKeep) return PT_OK;
  const int ntiles = wf_subset_tiles(k.W, k.H, 1, 0);
  if (p->busy_n != ntiles) {
    if (p->busy) (void)hipFree(p->busy);
    p->busy = nullptr;
    p->busy_n = 0;
    p->busy_valid = false;
    HIPCHK(hipMalloc((void**)&p->busy, busy_tiles_ints(ntiles) * sizeof(int)));
    p->busy_n = ntiles;
  }
  if (!p->busy_valid) {
    const int rc = launch_busy_tiles(k, p->busy, g.stream);
    if (rc) return hip_err((hipError_t)rc, "busy-tile list");
    p->busy_valid = true;
  }
  if (k.point_cache == kPcReset) HIPCHK(hipMemsetAsync(k.wf.pcache, 0, p->wf.n * sizeof(uint16_t), g.stream));
  k.busy = p->busy;
  return PT_OK;
}
// after the launch of a draw first_hit_mode_for gave a mode: a draw that was not bypassed has left emission and albedo
// holding the content `first` (bg_note_colour stamps the colour); a failed one leaves what att_plane left: nothing
static void first_hit_note(Pass* p, uint64_t first, bool ok) {
  if (!ok || p->fh_mode == ptk::kFhOff) return;
  if (Texture* t = tex_of(p->att[1])) t->first_hit = first;
  if (Texture* t = tex_of(p->att[2])) t->first_hit = first;
  if (p->fh_mode == ptk::kFhKeep) p->fh_kept++;
}
int StaticView::setup(Pass* p, PTParams& k, const SceneGPU* sg, const DrawReads& reads) {
  lkey = point_cache_mode_for(p, k, key, reuse, reads, &forgets, &forget);
  return first_hit_mode_for(p, k, sg, key, reuse, reads, *this, &first);
}
void StaticView::finish(Pass* p, const PTParams& k, const DrawReads& reads, int rc) {
  primary_cache_note(p, key, reuse, rc == 0);
  first_hit_note(p, first, rc == 0);
  point_cache_note_lights(p->lcache, lkey, k.point_cache, forgets, rc == 0);
  p->lcache_last_mode = k.point_cache;
  p->lcache_last_forgot = forget;
  if (!rc) bg_note_colour(p, k, key, reads);
}
void static_view_off(Pass* p, int reason, bool keep_primary) {
  if (!keep_primary) p->pcache.valid = false;
  p->lcache.valid = false;
  p->lcache_last_mode = 0;
  p->fh_mode = kFhOff;
  p->fh_reason = reason;
}

// ---- the static background of the SVGF chain (DESIGN.md "Static view, part 3"; static_key.h has the rules)
// static_background (int uniform of a reproject, variance or a-trous pass, default 0): the caller states that nothing
// outside the library writes the pass's textures. PTSVGF_STATIC_BACKGROUND=0 in the environment forces it off (A/B).
static bool bg_env_off() {
  static const bool off = [] {
    const char* e = getenv("PTSVGF_STATIC_BACKGROUND");
    return e && atoi(e) == 0;
  }();
  return off;
}
bool bg_whole(const Texture* t, int H) { return t && t->row0 == 0 && t->rows == H; }
static QuietSet* bg_set_of(uint64_t id) {
  if (id)
    for (QuietSet& q : g.bg_sets)
      if (q.id == id) return &q;
  return nullptr;
}
// What bypasses every SVGF draw alike: the switch, the environment, a row subset or band.
int bg_bypass(Pass* p, int y0, int y1) {
  if (ui(p, "static_background", 0) == 0) return PT_BG_R_UNIFORM;
  if (bg_env_off()) return PT_BG_R_ENV;
  if (y0 != 0 || y1 != p->H || band_partition(p->W, p->H)) return PT_BG_R_ROWS;
  return PT_BG_R_NONE;
}
// Builds set `id` for the colour plane ct and the depth-fwidth attachment ft of a W x H frame, on the draw's stream:
// from ft's compact plane and the primary plane of the pass that wrote ct, if it still holds that draw's hits.
int bg_build_set(uint64_t id, const Texture* ct, const Texture* ft, int W, int H, bool* built) {
  *built = false;
  Pass* pp = nullptr;
  for (auto& kv : g.passes)
    if (kv.second.get() == ct->bg_pass) pp = kv.second.get();
  if (!pp || pp->wf.gen != ct->bg_pass_gen || !pp->pcache.valid || !pp->wf.st.hit0 || !ft->aux || !ft->aux_valid)
    return PT_OK;
  const ptk::PrimaryKey pc = ptk::primary_content(pp->pcache.key);
  if (g.bg_prim.of(pc.w, ptk::kPkWords, &g.bg_serial) != ct->bg_prim) return PT_OK;
  QuietSet& q = g.bg_sets[g.bg_next];
  g.bg_next = (g.bg_next + 1) % kQuietSets;
  // the oldest set's allocation is taken again: draws issued on this stream have read it by the time the build runs;
  // draws on other streams are waited for (a set goes out of use kQuietSets views later, so this is rare)
  if (q.flags && (q.mixed || q.last_stream != g.stream)) HIPCHK(hipDeviceSynchronize());
  q.id = 0;
  const size_t off16 = ptk::atrous_flag_bytes(W, 0, H), n16 = (size_t)((W + 15) / 16) * ((H + 15) / 16);
  const size_t offc = (off16 + n16 + 3) / 4 * 4, need = offc + 6 * sizeof(uint32_t);
  if (q.cap < need) {
    if (q.flags) (void)hipFree(q.flags);
    q.flags = nullptr;
    q.cap = 0;
    HIPCHK(hipMalloc((void**)&q.flags, need));
    q.cap = need;
  }
  const int rc = ptk::launch_quiet_flags(ft->aux, ft->row0, pp->wf.st.hit0, W, H, q.flags, q.flags + off16,
                                         (uint32_t*)(q.flags + offc), g.stream);
  if (rc) return hip_err((hipError_t)rc, "quiet-tile flags");
  q.id = id;
  q.gbuf = ft->bg_gbuf;
  q.W = W;
  q.H = H;
  q.off16 = off16;
  q.off_counts = offc;
  q.last_stream = g.stream;
  q.mixed = false;
  *built = true;
  return PT_OK;
}
// One SVGF draw's decision (BgDraw, capi_state.h)
void BgDraw::pair(const Texture* i, Texture* o, bool modulated) {
  if (i && i->bg_off && !in_off) in_off = i->bg_off;
  in[npairs] = i ? i->bg : ptk::BgStamp{};
  was[npairs] = o ? o->bg : ptk::BgStamp{};
  out[npairs] = o;
  mod[npairs++] = modulated;
}
void BgDraw::decide() {
  qs = bg_set_of(set);
  if (!qs) set = 0;
  if (!reason && in_off) reason = in_off;  // the chain was bypassed above this draw
  if (reason) return;
  if (!set) {
    reason = PT_BG_R_NO_SET;
    return;
  }
  skip = true;
  for (int i = 0; i < npairs; ++i) skip = skip && ptk::bg_pair_quiet(in[i], was[i], set, mod[i]);
  if (!skip) reason = PT_BG_R_STAMPS;
}
void BgDraw::finish(Pass* p, int shape, bool ok) {
  const bool off = reason >= PT_BG_R_UNIFORM && reason <= PT_BG_R_NO_PLANE;
  for (int i = 0; i < npairs; ++i)
    if (out[i]) {
      out[i]->bg = ptk::bg_copy(in[i], ok && !off ? set : 0, mod[i], &g.bg_serial);
      out[i]->bg_off = off ? reason : 0;
    }
  if (qs && skip) {
    qs->mixed = qs->mixed || qs->last_stream != g.stream;
    qs->last_stream = g.stream;
  }
  p->bg_mode = off ? PT_BG_OFF : skip ? PT_BG_SKIP : PT_BG_ARMED;
  p->bg_reason = reason;
  p->bg_set = off ? 0 : set;
  p->bg_shape = shape;
}
// The set of a variance or a-trous draw: the one its input's stamp holds for, provided it was built for the G-buffer
// content of this draw's depth-fwidth attachment and the frame's size.
uint64_t bg_set_from_input(const Texture* in, const Texture* ft, int W, int H) {
  const QuietSet* q = in && in->bg.id ? bg_set_of(in->bg.scope) : nullptr;
  return q && ft->bg_gbuf && q->gbuf == ft->bg_gbuf && q->W == W && q->H == H ? q->id : 0;
}
// gNormalAndLinearZ and gNormalDepthFwidth are attachments of one G-buffer draw, and the compact plane is there: the
// kernels' background tests (nd.w == 1, the compact plane's sign) then agree with the flags' content
bool bg_one_gbuffer(const Texture* nd, const Texture* ft) {
  return nd && ft && ft->aux && ft->aux_valid && ft->raster_stamp != 0 && nd->raster_stamp == ft->raster_stamp;
}

}  // namespace ptapi

extern "C" {

int pt_debug_stage_counts(uint32_t pass, uint64_t* runs, uint64_t* reuses) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  const int kind = g.programs[p->program];
  if (kind != PK_PATHTRACE && kind != PK_RASTER)
    return err(PT_ERR_ARG, "pt_debug_stage_counts: a path-tracing or a rasterize pass");
  if (runs) *runs = kind == PK_PATHTRACE ? p->pcache.runs : p->gcache.runs;
  if (reuses) *reuses = kind == PK_PATHTRACE ? p->pcache.reuses : p->gcache.reuses;
  return PT_OK;
}

// The argument check of every entry point that takes keys as words: two keys (or one, twice), the output, and the
// word count against `expect`, that of the key's kind (negative: the error of static_words, passed on).
static int key_args(const char* who, const void* a, const void* b, const void* out, int words, int expect) {
  if (expect < 0) return expect;
  if (!a || !b || !out) return err(PT_ERR_ARG, std::string(who) + ": null argument");
  if (words != expect) return err(PT_ERR_ARG, std::string(who) + ": not the key's word count");
  return PT_OK;
}
// the word count of the kinds pt_debug_static_key_* serve
static int static_words(const char* who, int kind) {
  if (kind != 0 && kind != 1) return err(PT_ERR_ARG, std::string(who) + ": kind 0 (primary) or 1 (G-buffer)");
  return kind == 0 ? (int)ptk::kPkWords : (int)ptk::kGkWords;
}

int pt_debug_static_key_words(int kind) { return static_words("pt_debug_static_key_words", kind); }

int pt_debug_static_key_diff(int kind, const uint64_t* a, const uint64_t* b, int words, int* field) {
  TRY(key_args("pt_debug_static_key_diff", a, b, field, words, static_words("pt_debug_static_key_diff", kind)));
  *field = ptk::key_words_diff(a, b, words);
  return PT_OK;
}

int pt_debug_static_key_hit(int kind, const uint64_t* last, int last_valid, const uint64_t* now, int words, int enabled,
                            int* hit) {
  TRY(key_args("pt_debug_static_key_hit", last, now, hit, words, static_words("pt_debug_static_key_hit", kind)));
  if (kind == 0) {
    ptk::PrimaryCache c;
    c.key = ptk::key_from<ptk::PrimaryKey>(last);
    c.valid = last_valid != 0;
    *hit = ptk::primary_cache_hit(c, ptk::key_from<ptk::PrimaryKey>(now), !enabled) ? 1 : 0;
  } else {
    ptk::GbufCache c;
    c.key = ptk::key_from<ptk::GbufKey>(last);
    c.valid = last_valid != 0;
    *hit = ptk::gbuf_cache_hit(c, ptk::key_from<ptk::GbufKey>(now), enabled != 0) ? 1 : 0;
  }
  return PT_OK;
}

// ---- the static background of the SVGF chain (DESIGN.md "Static view, part 3")
int pt_debug_bg_counts(uint32_t pass, int* mode, int* reason, uint64_t* skipped, uint64_t* total) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (mode) *mode = p->bg_mode;
  if (reason) *reason = p->bg_reason;
  if (skipped) *skipped = 0;
  if (total) *total = 0;
  if (p->bg_mode == PT_BG_OFF) return PT_OK;
  const int S = 1 << p->bg_shape, nx = ptk::atrous_tile_nx(S), tj = ptk::atrous_tile_tj(S);
  const uint64_t n = p->bg_shape == 5 ? (uint64_t)((p->W + 15) / 16) * ((p->H + 15) / 16)
                                      : (uint64_t)((p->W + 64 * nx - 1) / (64 * nx)) * ((p->H + S * tj - 1) / (S * tj)) * S;
  if (total) *total = n;
  const QuietSet* q = bg_set_of(p->bg_set);
  if (p->bg_mode != PT_BG_SKIP || !q || !skipped) return PT_OK;
  uint32_t busy[6];
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(busy, q->flags + q->off_counts, sizeof(busy), hipMemcpyDeviceToHost));
  *skipped = n - busy[p->bg_shape];
  return PT_OK;
}

int pt_debug_bg_stamp(uint32_t tex, uint64_t* id, uint64_t* scope) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  const Texture* t = tex_of(tex);
  if (!t) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  if (id) *id = t->bg.id;
  if (scope) *scope = t->bg.scope;
  return PT_OK;
}

int pt_debug_bg_poke_hit0(uint32_t pass, int x, int y, int tri, float t) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_PATHTRACE || !p->wf.st.hit0)
    return err(PT_ERR_STATE, "pt_debug_bg_poke_hit0: a path-tracing pass that has drawn with the wavefront path tracer");
  if (x < 0 || x >= p->W || y < 0 || (size_t)y * p->W + x >= p->wf.n)
    return err(PT_ERR_ARG, "pt_debug_bg_poke_hit0: pixel outside the rows the pass drew");
  int2 v;
  v.x = tri;
  memcpy(&v.y, &t, sizeof(t));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(p->wf.st.hit0 + (size_t)y * p->W + x, &v, sizeof(v), hipMemcpyHostToDevice));
  // the plane is no longer what the stage wrote: the busy-tile list and the first-hit records were derived from that
  p->busy_valid = false;
  for (size_t i = 1; i < 3 && i < p->att.size(); ++i)
    if (Texture* at = tex_of(p->att[i])) at->first_hit = 0;
  return PT_OK;
}

// ---- the bounce-0 shade's keep mode (DESIGN.md "Static view, part 4")
int pt_debug_firsthit_last(uint32_t pass, int* mode, int* reason, uint64_t* kept) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_PATHTRACE) return err(PT_ERR_ARG, "pt_debug_firsthit_last: a path-tracing pass");
  if (mode) *mode = p->fh_mode;
  if (reason) *reason = p->fh_reason;
  if (kept) *kept = p->fh_kept;
  return PT_OK;
}

int pt_debug_firsthit_busy(uint32_t pass, int* busy, int* tiles) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_PATHTRACE) return err(PT_ERR_ARG, "pt_debug_firsthit_busy: a path-tracing pass");
  if (!busy || !tiles) return err(PT_ERR_ARG, "pt_debug_firsthit_busy: null argument");
  *busy = -1;
  *tiles = ptk::wf_subset_tiles(p->W, p->H, 1, 0);
  if (!p->busy || !p->busy_valid) return PT_OK;
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(busy, p->busy, sizeof(int), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_debug_firsthit_record(uint32_t tex, uint64_t* id) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  const Texture* t = tex_of(tex);
  if (!t) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  if (!id) return err(PT_ERR_ARG, "pt_debug_firsthit_record: null argument");
  *id = t->first_hit;
  return PT_OK;
}

int pt_debug_firsthit_key_words(void) { return (int)ptk::kFkWords; }

int pt_debug_firsthit_key_diff(const uint64_t* a, const uint64_t* b, int words, int* field) {
  TRY(key_args("pt_debug_firsthit_key_diff", a, b, field, words, ptk::kFkWords));
  *field = ptk::key_words_diff(a, b, words);
  return PT_OK;
}

int pt_debug_firsthit_key_id(const uint64_t* key, int words, uint64_t* id) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(key_args("pt_debug_firsthit_key_id", key, key, id, words, ptk::kFkWords));
  *id = g.bg_first.of(key, words, &g.bg_serial);
  return PT_OK;
}

int pt_debug_firsthit_decide(uint32_t bypass, int stage_reused, uint64_t colour_id, uint64_t colour_scope,
                             uint64_t emission, uint64_t albedo, uint64_t miss, uint64_t first, int* mode, int* reason) {
  if (!mode || !reason) return err(PT_ERR_ARG, "pt_debug_firsthit_decide: null argument");
  *mode = ptk::first_hit_mode(bypass, stage_reused != 0, ptk::BgStamp{colour_id, colour_scope}, emission, albedo, miss,
                              first, reason);
  return PT_OK;
}

int pt_debug_bg_fresh(uint64_t* serial, uint64_t* id, uint64_t* scope) {
  if (!serial || !id || !scope) return err(PT_ERR_ARG, "pt_debug_bg_fresh: null argument");
  const ptk::BgStamp s = ptk::bg_fresh(serial);
  *id = s.id;
  *scope = s.scope;
  return PT_OK;
}

int pt_debug_bg_copy(uint64_t in_id, uint64_t in_scope, uint64_t set, int modulated, uint64_t* serial, uint64_t* id,
                     uint64_t* scope) {
  if (!serial || !id || !scope) return err(PT_ERR_ARG, "pt_debug_bg_copy: null argument");
  const ptk::BgStamp s = ptk::bg_copy(ptk::BgStamp{in_id, in_scope}, set, modulated != 0, serial);
  *id = s.id;
  *scope = s.scope;
  return PT_OK;
}

int pt_debug_bg_pair_quiet(uint64_t in_id, uint64_t in_scope, uint64_t out_id, uint64_t out_scope, uint64_t set,
                           int modulated, int* quiet) {
  if (!quiet) return err(PT_ERR_ARG, "pt_debug_bg_pair_quiet: null argument");
  *quiet = ptk::bg_pair_quiet(ptk::BgStamp{in_id, in_scope}, ptk::BgStamp{out_id, out_scope}, set, modulated != 0) ? 1 : 0;
  return PT_OK;
}

int pt_debug_bg_quiet_set(uint64_t* state, uint64_t prim, uint64_t gbuf, uint64_t* serial, uint64_t* set, int* build) {
  if (!state || !serial || !set || !build) return err(PT_ERR_ARG, "pt_debug_bg_quiet_set: null argument");
  ptk::QuietChoice c;
  c.prim = state[0];
  c.gbuf = state[1];
  c.set = state[2];
  bool b = false;
  *set = ptk::quiet_set_for(c, prim, gbuf, serial, &b);
  *build = b ? 1 : 0;
  state[0] = c.prim;
  state[1] = c.gbuf;
  state[2] = c.set;
  return PT_OK;
}

int pt_debug_bg_miss_key_words(void) { return (int)ptk::kMkWords; }

int pt_debug_bg_miss_key_diff(const uint64_t* a, const uint64_t* b, int words, int* field) {
  TRY(key_args("pt_debug_bg_miss_key_diff", a, b, field, words, ptk::kMkWords));
  *field = ptk::key_words_diff(a, b, words);
  return PT_OK;
}

int pt_debug_bg_miss_key_id(const uint64_t* key, int words, uint64_t* id) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(key_args("pt_debug_bg_miss_key_id", key, key, id, words, ptk::kMkWords));
  *id = g.bg_miss.of(key, words, &g.bg_serial);
  return PT_OK;
}

int pt_debug_bg_key_content(int kind, const uint64_t* key, int words, uint64_t source, uint64_t* out) {
  TRY(key_args("pt_debug_bg_key_content", key, key, out, words, static_words("pt_debug_bg_key_content", kind)));
  if (kind == 0) {
    const ptk::PrimaryKey k = ptk::primary_content(ptk::key_from<ptk::PrimaryKey>(key));
    memcpy(out, k.w, sizeof(k.w));
  } else {
    const ptk::GbufKey k = ptk::gbuf_content(ptk::key_from<ptk::GbufKey>(key), source);
    memcpy(out, k.w, sizeof(k.w));
  }
  return PT_OK;
}

// ---- the bounce-0 point-light verdict cache (DESIGN.md "Static view, part 2")
static int point_cache_pass(const char* who, uint32_t pass, Pass** out) {
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_PATHTRACE) return err(PT_ERR_ARG, std::string(who) + ": a path-tracing pass");
  if (!p->wf.base) return err(PT_ERR_STATE, std::string(who) + ": the pass has not drawn with the wavefront path tracer");
  *out = p;
  return PT_OK;
}

int pt_debug_point_cache_counts(uint32_t pass, uint64_t* served, uint64_t* queued) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p;
  TRY(point_cache_pass("pt_debug_point_cache_counts", pass, &p));
  HIPCHK(hipDeviceSynchronize());
  int c[ptk::kWfCtr];  // bounce 0's counters of frame 0
  HIPCHK(hipMemcpy(c, p->wf.st.counters, sizeof(c), hipMemcpyDeviceToHost));
  uint64_t q = 0;
  for (int i = 0; i < 8 * ptk::kPointBins; ++i) q += (uint64_t)c[ptk::kCtrPoint + i];
  uint64_t sv = 0;
  for (int i = 0; i < 8; ++i) sv += (uint64_t)c[ptk::kCtrPcServed + i];
  if (served) *served = sv;
  if (queued) *queued = q;
  return PT_OK;
}

int pt_debug_point_cache_read(uint32_t pass, uint16_t* words, size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p;
  TRY(point_cache_pass("pt_debug_point_cache_read", pass, &p));
  if (!words || n != p->wf.n) return err(PT_ERR_ARG, "pt_debug_point_cache_read: one word per pixel of the pass's rows");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(words, p->wf.st.pcache, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_debug_point_cache_write(uint32_t pass, const uint16_t* words, size_t n) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p;
  TRY(point_cache_pass("pt_debug_point_cache_write", pass, &p));
  if (!words || n != p->wf.n) return err(PT_ERR_ARG, "pt_debug_point_cache_write: one word per pixel of the pass's rows");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(p->wf.st.pcache, words, n * sizeof(uint16_t), hipMemcpyHostToDevice));
  return PT_OK;
}

int pt_debug_point_cache_mode(uint32_t pass, int* mode, int* valid) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_PATHTRACE) return err(PT_ERR_ARG, "pt_debug_point_cache_mode: a path-tracing pass");
  if (mode) *mode = p->lcache_last_mode;
  if (valid) *valid = p->lcache.valid ? 1 : 0;
  return PT_OK;
}

int pt_debug_point_cache_word(int op, uint32_t word, int arg, uint32_t* out) {
  if (!out) return err(PT_ERR_ARG, "pt_debug_point_cache_word: null argument");
  if ((op == 0 || op == 2) && (arg < 0 || arg >= ptk::kPcLights))
    return err(PT_ERR_ARG, "pt_debug_point_cache_word: a light index in 0 .. 3");
  switch (op) {
    case 0: *out = (uint32_t)ptk::pc_lookup(word, arg); break;
    case 1: *out = (uint32_t)ptk::pc_pending(word); break;
    case 2: *out = ptk::pc_mark_pending(word, arg); break;
    case 3: *out = ptk::pc_resolve(word, arg != 0); break;
    case 5: *out = ptk::pc_forget(word, (uint32_t)arg); break;  // (4 stays no op: it has always been refused)
    default: return err(PT_ERR_ARG, "pt_debug_point_cache_word: op 0 (look-up) .. 3 (resolve), 5 (forget)");
  }
  return PT_OK;
}

int pt_debug_point_cache_key_words(void) { return (int)ptk::kLkWords; }

int pt_debug_point_cache_key_diff(const uint64_t* a, const uint64_t* b, int words, int* field) {
  TRY(key_args("pt_debug_point_cache_key_diff", a, b, field, words, ptk::kLkWords));
  *field = ptk::key_words_diff(a, b, words);
  return PT_OK;
}

int pt_debug_point_cache_key_mode(const uint64_t* last, int last_valid, const uint64_t* now, int words, int stage_reused,
                                  int enabled, int* mode) {
  TRY(key_args("pt_debug_point_cache_key_mode", last, now, mode, words, ptk::kLkWords));
  ptk::PointCache c;
  c.key = ptk::key_from<ptk::LightsKey>(last);
  c.valid = last_valid != 0;
  *mode = ptk::point_cache_mode(c, ptk::key_from<ptk::LightsKey>(now), stage_reused != 0, !enabled);
  return PT_OK;
}

}  // extern "C"

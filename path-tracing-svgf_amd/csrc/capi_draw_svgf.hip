// capi_draw_svgf.hip — the draws of pt_pass_draw that are not the path tracer's (capi.hip dispatches): the G-buffer
// draw (draw_raster) and the SVGF chain, one function per pass kind (reproject, variance, a-trous, modulate, output,
// TAA, blit, save) under draw_svgf's switch. The static background's decisions are capi_static.hip's (BgDraw); what
// the three kinds that skip quiet tiles share of its prologue is here. Host code only, over capi_state.h.
#include "../../include/ptsvgf_debug_background.h"
#include "capi_state.h"

using namespace ptapi;
using namespace ptk;

namespace {

int copy_plane(Texture* dst, Texture* src, Pass* p, int y0, int y1) {
  if (!src || !dst || !src->dev || !dst->dev) return err(PT_ERR_MISSING_TEXTURE, "copy: unbound texture");
  if (src->W != dst->W || src->H != dst->H) return err(PT_ERR_ARG, "copy: size mismatch");
  (void)p;
  int a = std::max(y0, std::max(src->row0, dst->row0));
  int b = std::min(y1, std::min(src->row0 + src->rows, dst->row0 + dst->rows));
  if (b > a) {
    size_t rowb = (size_t)src->W * 16;
    HIPCHK(hipMemcpyAsync((char*)dst->dev + (size_t)(a - dst->row0) * rowb,
                          (char*)src->dev + (size_t)(a - src->row0) * rowb, (size_t)(b - a) * rowb,
                          hipMemcpyDeviceToDevice, g.stream));
  }
  tex_written(dst);
  if (src->aux_valid && src->aux) {  // keep the compact side plane in step with its texture
    if (!dst->aux) HIPCHK(hipMalloc((void**)&dst->aux, (size_t)dst->W * dst->rows * 4));
    if (b > a) {
      size_t rb = (size_t)src->W * 4;
      HIPCHK(hipMemcpyAsync((char*)dst->aux + (size_t)(a - dst->row0) * rb, (char*)src->aux + (size_t)(a - src->row0) * rb,
                            (size_t)(b - a) * rb, hipMemcpyDeviceToDevice, g.stream));
    }
    dst->aux_valid = true;
    memcpy(dst->aux_eye, src->aux_eye, sizeof(dst->aux_eye));
  }
  return PT_OK;
}

// The compact side plane of a G-buffer attachment (Texture::aux), allocated on first use: the rows no draw has reached
// read `fill`.
int aux_plane(Texture* t, uint32_t fill, float** out) {
  if (!t->aux) {
    const size_t n = (size_t)t->W * t->rows;
    HIPCHK(hipMalloc((void**)&t->aux, n * 4));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)t->aux, fill, n, g.stream));
  }
  *out = t->aux;
  return PT_OK;
}

}  // namespace

namespace ptapi {

// The tile flags of a draw of p over rows [k.y0, k.y1): the rows the a-trous passes draw ("atrous_rows_begin" /
// "_end", e.g. a band's ghost-zone margin), default the G-buffer's own rows; they must lie inside them (a tile's flag is
// marked by the G-buffer pixels it holds). Allocates and zeroes them on the fwidth texture; k.tflags null when off.
int gbuf_flags(Pass* p, Texture* fwt, GBufParams& k) {
  k.tf_y0 = ui(p, "atrous_rows_begin", -1) >= 0 ? ui(p, "atrous_rows_begin", -1) : k.y0;
  k.tf_y1 = ui(p, "atrous_rows_end", -1) >= 0 ? ui(p, "atrous_rows_end", -1) : k.y1;
  if (k.tf_y0 < k.y0 || k.tf_y1 > k.y1 || k.tf_y0 > k.tf_y1)
    return err(PT_ERR_ARG, "atrous_rows_begin / _end outside the G-buffer's rows");
  if (ui(p, "atrous_tile_flags", 1) && k.tf_y1 > k.tf_y0) {
    const size_t nb = ptk::atrous_flag_bytes(k.W, k.tf_y0, k.tf_y1);
    if (fwt->tflags_cap < nb) {
      if (fwt->tflags) (void)hipFree(fwt->tflags);
      fwt->tflags = nullptr;
      fwt->tflags_cap = 0;
      HIPCHK(hipMalloc((void**)&fwt->tflags, nb));
      fwt->tflags_cap = nb;
    }
    HIPCHK(hipMemsetAsync(fwt->tflags, 0, nb, g.stream));
    k.tflags = fwt->tflags;
    for (int si = 0; si < 5; ++si) k.tf_off[si] = (int)ptk::atrous_flag_offset(si, k.W, k.tf_y0, k.tf_y1);
    fwt->tflags_ver = fwt->version;
    fwt->tflags_y0 = k.tf_y0;
    fwt->tflags_y1 = k.tf_y1;
  } else {
    fwt->tflags_ver = 0;
  }
  return PT_OK;
}

int draw_raster(Pass* p) {
  Pass* src = p->raster_src ? pass_of(p->raster_src) : p;
  if (!src) return err(PT_ERR_STATE, "raster pass shares the triangles of a destroyed pass");
  if (src != p && src->raster_src)  // the source became a sharer itself: its own raster scene is stale
    return err(PT_ERR_STATE, "raster pass shares the triangles of a pass that now shares another pass's");
  const RasterScene& rs = src->raster;
  if (!rs.geom && rs.ntris > 0) return err(PT_ERR_STATE, "raster pass not bound");
  // Static view: the G-buffer is a function of what the key holds. When this draw's key equals the one
  // taken after the pass's last completed draw, the four attachments, both compact planes and the tile flags already
  // hold what it would write: nothing is launched and no version moves. A motion bound is cleared and reduced per
  // draw, so a pass with one always draws. The planes were written by an earlier draw of this pass, perhaps on
  // another stream: what lets a draw overwrite a set (its earlier readers are done) lets this one leave it as it is.
  ptk::GbufKey now;
  if (reuse_static_on(p) && !p->motion_max && gbuf_key(p, src, &now) && ptk::gbuf_cache_hit(p->gcache, now, true)) {
    p->gcache.reuses++;
    return PT_OK;
  }
  p->gcache.valid = false;
  GBufParams k;
  memset(&k, 0, sizeof(k));
  k.W = p->W;
  k.H = p->H;
  rows_of(p, &k.y0, &k.y1);
  TRY(att_plane(p, 0, &k.world));
  TRY(att_plane(p, 1, &k.normal_depth));
  TRY(att_plane(p, 2, &k.motion));
  TRY(att_plane(p, 3, &k.fwidth));
  Texture* fwt = tex_of(p->att[3]);
  TRY(aux_plane(fwt, 0, &k.fwidth_aux));  // rows no draw has reached read 0 (pt_texture_readback_aux returns the whole plane)
  // the a-trous per-tile surface flags of this G-buffer, marked by the G-buffer kernels as they write the pixels
  TRY(gbuf_flags(p, fwt, k));
  // vec3 uniform bound_eye (the origin of this frame's primary rays): the draw also writes the primary rasterisers'
  // pruning bound of every pixel into the world attachment's compact plane, 4 bytes instead of their 32 of texels
  Texture* wt = tex_of(p->att[0]);
  const Uniform* be = U(p, "bound_eye", 5);
  if (be) {
    TRY(aux_plane(wt, 0x7f800000, &k.bound_aux));  // rows no draw has reached hold "no bound" (+inf)
    memcpy(k.bound_eye, be->f, sizeof(k.bound_eye));
  }
  k.geom = rs.geom;
  k.nrm = rs.nrm;
  // object motion: the source's displacement records, unless this pass's int uniform object_motion is 0
  if (rs.disp && rs.ntris > 0 && ui(p, "object_motion", 1) != 0) k.disp = rs.disp;
  k.bvh = rs.bvh;
  k.root_ref = rs.root_ref;
  k.stack_need = rs.stack_need;
  float V[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, P[16], PV[16];
  memcpy(P, V, 64);
  memcpy(PV, V, 64);
  if (const Uniform* u = U(p, "view", 6)) memcpy(V, u->f, 64);
  if (const Uniform* u = U(p, "projection", 6)) memcpy(P, u->f, 64);
  if (const Uniform* u = U(p, "pre_viewproj", 6)) memcpy(PV, u->f, 64);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) k.invR[r * 3 + c] = V[r * 4 + c];
  for (int r = 0; r < 3; ++r)
    k.eye[r] = -((k.invR[r * 3] * V[12] + k.invR[r * 3 + 1] * V[13]) + k.invR[r * 3 + 2] * V[14]);
  k.P00 = P[0];
  k.P11 = P[5];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
      k.M[c * 4 + r] = ((P[0 * 4 + r] * V[c * 4 + 0] + P[1 * 4 + r] * V[c * 4 + 1]) + P[2 * 4 + r] * V[c * 4 + 2]) +
                       P[3 * 4 + r] * V[c * 4 + 3];
  memcpy(k.PV, PV, 64);
  if (rs.ntris == 0) k.root_ref = -1;  // empty leaf
  if (p->motion_max) {
    HIPCHK(hipMemsetAsync(p->motion_max, 0, sizeof(uint32_t), g.stream));
    k.motion_max = p->motion_max;
  }
  const int ntiles = ((k.W + 15) / 16) * ((std::max(0, k.y1 - k.y0) + 15) / 16);  // gbuffer_kernel's grid
  if (ui(p, "gbuffer_mode", 1) == 1) {  // tile-binned rasterisation (default); the ray cast on list overflow
    TRY(bins_for(p->bins, rs.ntris, k.W, k.y0, k.y1, ui(p, "raster_pair_cap", 0), &k.bins));
    int rc = launch_gbuffer_raster(k, g.stream);
    if (rc) return hip_err((hipError_t)rc, "gbuffer raster launch");
  } else {  // A/B: the ray cast with cost-ordered tiles
    TRY(tile_order_begin(p, ntiles, &k.tiles));
    int rc = launch_gbuffer(k, g.stream);
    if (rc) return hip_err((hipError_t)rc, "gbuffer launch");
    TRY(tile_order_finish(p, k.tiles));
  }
  fwt->aux_valid = true;
  if (k.bound_aux) {
    wt->aux_valid = true;
    memcpy(wt->aux_eye, k.bound_eye, sizeof(wt->aux_eye));
  }
  // the draw is complete: its serial on what it wrote, and the key of the state it leaves
  const uint64_t serial = ++g.raster_serial;
  for (int i = 0; i < 4; ++i) tex_of(p->att[i])->raster_stamp = serial;
  p->gcache.valid = gbuf_key(p, src, &p->gcache.key);
  p->gcache.runs++;
  // the static background (DESIGN.md "Static view, part 3"): which pixels of this set are background is a function of
  // the key's content, whichever set's planes these are (an elided draw leaves the id as it leaves the planes)
  if (p->gcache.valid && k.y0 == 0 && k.y1 == k.H && !band_partition(k.W, k.H) && fwt->row0 == 0 && fwt->rows == k.H) {
    const ptk::GbufKey c = ptk::gbuf_content(p->gcache.key, ptk::key_bits((const void*)src));
    fwt->bg_gbuf = g.bg_gbuf.of(c.w, ptk::kGkWords, &g.bg_serial);
  }
  return PT_OK;
}

}  // namespace ptapi

namespace {

// ---------------------------------------------------------------- the SVGF chain ---
// One function per pass kind: a draw of pass p over the rows [y0, y1). Each returns a library error as it meets one,
// and leaves its kernel launch's result (a hipError_t) in *launch for draw_svgf.

// the header every params struct of the chain starts with
template <class K>
void draw_header(Pass* p, int y0, int y1, K* k) {
  memset(k, 0, sizeof(*k));
  k->W = p->W;
  k->H = p->H;
  k->y0 = y0;
  k->y1 = y1;
}

// the plane of the sampler `name` (texture unit 0 when the pass never bound it)
int in_plane(Pass* p, const char* name, Plane* out) { return plane_of(sampler(p, name), p, out, name); }

// The static background (DESIGN.md "Static view, part 3"): what the three kinds that skip quiet tiles share, in three
// steps, because the first unmet condition is the draw's reason and each kind ranks conditions of its own between them.
// Every texture of `whole` stores the whole frame;
void bg_need_whole(BgDraw& bg, int H, std::initializer_list<const Texture*> whole) {
  bool all = true;
  for (const Texture* t : whole) all = all && bg_whole(t, H);
  bg.need(all, PT_BG_R_ROWS);
}
// gNormalAndLinearZ and the depth-fwidth plane ft are attachments of one G-buffer draw;
void bg_need_one_gbuffer(BgDraw& bg, Pass* p, const Texture* ft) {
  bg.need(bg_one_gbuffer(sampler(p, "gNormalAndLinearZ"), ft), PT_BG_R_NO_PLANE);
}
// the decision, and the flags of the set the draw skips by (null: it draws every tile).
const unsigned char* bg_decide(BgDraw& bg) {
  bg.decide();
  return bg.skip ? bg.qs->flags : nullptr;
}

int draw_reproject(Pass* p, int y0, int y1, int* launch) {
  BgDraw bg;
  bg.reason = bg_bypass(p, y0, y1);
  ReprojParams k;
  draw_header(p, y0, y1, &k);
  TRY(in_plane(p, "gMotion", &k.motion));
  TRY(in_plane(p, "gColor", &k.color));
  TRY(in_plane(p, "gAlbedo", &k.albedo));
  TRY(in_plane(p, "gEmission", &k.emission));
  TRY(in_plane(p, "gPrevIllum", &k.prev_illum));
  TRY(in_plane(p, "gPrevMoments_HistoryLength", &k.prev_moments));
  TRY(in_plane(p, "gNormalAndLinearZ", &k.nd));
  TRY(in_plane(p, "gPrevNormalAndLinearZ", &k.prev_nd));
  TRY(in_plane(p, "gNormalDepthFwidth", &k.fwidth));
  const Texture *ct = sampler(p, "gColor"), *pm = sampler(p, "gPrevMoments_HistoryLength");
  const Texture* ft = sampler(p, "gNormalDepthFwidth");
  if (p->att.size() >= 2) {  // (the stamps as the draw finds them: att_plane makes the outputs' fresh)
    bg.pair(ct, tex_of(p->att[0]), false);
    bg.pair(pm, tex_of(p->att[1]), false);
  }
  TRY(att_plane(p, 0, &k.out_illum));
  TRY(att_plane(p, 1, &k.out_moments));
  k.inv_w = uf(p, "inv_screen_width", 0.0f);
  k.inv_h = uf(p, "inv_screen_height", 0.0f);
  k.depth_thr = uf(p, "depth_threshold", 0.0f);
  k.normal_thr = uf(p, "normal_threshold", 0.0f);
  k.block = ui(p, "reproj_block", 1);  // A/B (0: lin per tap): the same texels either way
  // optional: the moments plane of the draw that wrote gColor (pt_pass_set_sample_moments)
  if (Texture* sm = bound_sampler(p, "gSampleMoments")) TRY(plane_of(sm, p, &k.sm, "gSampleMoments"));
  // static background: the set of this draw's (primary content, G-buffer content) pair, built by the second draw
  // that meets the pair; every other case forgets the pair, so no set outlives a bypass
  bg.need(!k.sm.p, PT_BG_R_SAMPLE_MOMENTS);
  bg_need_whole(bg, p->H, {ct, ft, bg.out[0], bg.out[1], pm});
  bg_need_one_gbuffer(bg, p, ft);
  bg.need(ct->bg_prim && ft->bg_gbuf, PT_BG_R_NO_CONTENT);
  bool build = false;
  // (a pass with the switch off takes no part: it leaves the choice to the passes that have it on)
  if (bg.reason != PT_BG_R_UNIFORM && bg.reason != PT_BG_R_ENV)
    bg.set = ptk::quiet_set_for(g.bg_choice, bg.reason ? 0 : ct->bg_prim, bg.reason ? 0 : ft->bg_gbuf, &g.bg_serial,
                                &build);
  if (build) {
    bool built = false;
    TRY(bg_build_set(bg.set, ct, ft, k.W, k.H, &built));
    if (!built) {  // (no primary plane to read: PT_BG_R_NO_PLANE, and the next draw tries again)
      g.bg_choice.set = bg.set = 0;
      bg.reason = PT_BG_R_NO_PLANE;
    }
  }
  bg.in_off = 0;  // (the head of the chain: what bypassed the last frame's draws does not bind this one)
  if (const unsigned char* quiet = bg_decide(bg)) k.busy16 = quiet + bg.qs->off16;
  *launch = launch_reproject(k, g.stream);
  bg.finish(p, 5, *launch == 0);
  return PT_OK;
}

int draw_variance(Pass* p, int y0, int y1, int* launch) {
  BgDraw bg;
  bg.reason = bg_bypass(p, y0, y1);
  VarianceParams k;
  draw_header(p, y0, y1, &k);
  TRY(in_plane(p, "gIllumination", &k.illum));
  TRY(in_plane(p, "gMoments_HistoryLength", &k.moments));
  TRY(in_plane(p, "gNormalAndLinearZ", &k.nd));
  TRY(in_plane(p, "gNormalDepthFwidth", &k.fwidth));
  const Texture *it = sampler(p, "gIllumination"), *ft = sampler(p, "gNormalDepthFwidth");
  if (!p->att.empty()) bg.pair(it, tex_of(p->att[0]), false);
  TRY(att_plane(p, 0, &k.out));
  k.phi_color = uf(p, "gPhiColor", 0.0f);
  k.phi_normal = uf(p, "gPhiNormal", 0.0f);
  if (Texture* sm = bound_sampler(p, "gSampleMoments")) TRY(plane_of(sm, p, &k.sm, "gSampleMoments"));
  bg.need(!k.sm.p, PT_BG_R_SAMPLE_MOMENTS);
  bg_need_whole(bg, p->H, {it, ft, bg.out[0]});
  bg_need_one_gbuffer(bg, p, ft);
  if (!bg.reason) bg.set = bg_set_from_input(it, ft, k.W, k.H);
  if (const unsigned char* quiet = bg_decide(bg)) k.busy16 = quiet + bg.qs->off16;
  *launch = launch_variance(k, g.stream);
  bg.finish(p, 5, *launch == 0);
  return PT_OK;
}

// The a-trous kernel of a draw: the pass's "exact" wins, then "atrous_variant" picks (0: production). A variant no
// kernel answers to runs the production kernel as the A/B kernels run: without tile flags, its modulate launched after.
enum AtrousKernel { kAtTiled, kAtSimple, kAtStep, kAtExact, kAtTiledPlain };
AtrousKernel atrous_kernel(Pass* p) {
  if (ui(p, "exact", 0)) return kAtExact;  // bit-exact form (tests)
  switch (ui(p, "atrous_variant", 0)) {
    case 0: return kAtTiled;   // LDS-tiled (production)
    case 1: return kAtSimple;  // A/B: generic
    case 2: return kAtStep;    // A/B: step kernel
    default: return kAtTiledPlain;
  }
}

// The tile flags of the depth-fwidth texture ft for a-trous draws over the rows [y0, y1): derived from its compact
// plane once per version of the texture and rows
int atrous_flags(Texture* ft, const Plane& fwidth, int W, int y0, int y1) {
  const size_t nb = ptk::atrous_flag_bytes(W, y0, y1);
  if (ft->tflags_cap < nb) {
    if (ft->tflags) (void)hipFree(ft->tflags);
    ft->tflags = nullptr;
    ft->tflags_cap = 0;
    HIPCHK(hipMalloc((void**)&ft->tflags, nb));
    ft->tflags_cap = nb;
    ft->tflags_ver = 0;
  }
  if (ft->tflags_ver != ft->version || ft->tflags_y0 != y0 || ft->tflags_y1 != y1) {
    const int frc = ptk::atrous_tile_flags(fwidth, W, y0, y1, ft->tflags, g.stream);
    if (frc) return hip_err((hipError_t)frc, "a-trous tile flags");
    ft->tflags_ver = ft->version;
    ft->tflags_y0 = y0;
    ft->tflags_y1 = y1;
  }
  return PT_OK;
}

int draw_atrous(Pass* p, int y0, int y1, int* launch) {
  BgDraw bg;
  bg.reason = bg_bypass(p, y0, y1);
  AtrousParams k;
  draw_header(p, y0, y1, &k);
  TRY(in_plane(p, "gIllumination", &k.illum));
  TRY(in_plane(p, "gNormalAndLinearZ", &k.nd));
  TRY(in_plane(p, "gNormalDepthFwidth", &k.fwidth));
  const Texture* it = sampler(p, "gIllumination");
  Texture* ft = sampler(p, "gNormalDepthFwidth");
  const bool fuse = ui(p, "fuse_modulate", 0) != 0;
  if (!p->att.empty()) bg.pair(it, tex_of(p->att[0]), false);
  if (fuse && p->att.size() >= 2) bg.pair(it, tex_of(p->att[1]), true);
  TRY(att_plane(p, 0, &k.out));
  if (k.out.p == k.illum.p) return err(PT_ERR_ARG, "a-trous output aliases its input (GL feedback loop)");
  k.step = ui(p, "gStepSize", 1);
  k.phi_color = uf(p, "gPhiColor", 0.0f);
  k.phi_normal = uf(p, "gPhiNormal", 0.0f);
  // production tiled kernel: per-tile surface flags, derived once per G-buffer from its depth-fwidth plane
  const int si = k.step == 1 ? 0 : k.step == 2 ? 1 : k.step == 4 ? 2 : k.step == 8 ? 3 : k.step == 16 ? 4 : -1;
  const AtrousKernel kernel = atrous_kernel(p);
  if (kernel == kAtTiled && ui(p, "atrous_tile_flags", 1) && k.fwidth.aux && si >= 0 && y1 > y0) {
    TRY(atrous_flags(ft, k.fwidth, k.W, y0, y1));
    k.tile_any = ft->tflags + ptk::atrous_flag_offset(si, k.W, y0, y1);
  }
  // fused modulate (fast driver, last iteration): "fuse_modulate" = 1, colour attachment 1 = the modulate target,
  // gAlbedo / gEmission bound; the production kernel writes it from its epilogue, the others launch modulate after
  if (fuse) {
    TRY(in_plane(p, "gAlbedo", &k.albedo));
    TRY(in_plane(p, "gEmission", &k.emission));
    TRY(att_plane(p, 1, &k.mod));
    for (const Plane* q : {&k.albedo, &k.emission, &k.mod})
      if (y0 < std::max(0, q->row0) || y1 > std::min(p->H, q->row0 + q->rows))
        return err(PT_ERR_ARG, "fused modulate: a plane does not store the draw's rows");
    if (k.mod.p == k.illum.p || k.mod.p == k.out.p) return err(PT_ERR_ARG, "fused modulate target aliases the a-trous planes");
  }
  // static background: only the tiled kernel with this draw's own tile flags skips (k.tile_any set: the production
  // variant, a step of 1 .. 16, the compact plane), and only over whole-frame planes, which is also what makes
  // launch_atrous_fast choose it (same_geometry)
  bg_need_whole(bg, p->H, {it, ft, bg.out[0], sampler(p, "gNormalAndLinearZ")});
  if (bg.npairs == 2) bg_need_whole(bg, p->H, {bg.out[1]});  // (the fused modulate's target)
  bg.need(k.fwidth.aux, PT_BG_R_NO_PLANE);
  bg.need(k.tile_any, PT_BG_R_KERNEL);
  bg_need_one_gbuffer(bg, p, ft);
  if (!bg.reason) bg.set = bg_set_from_input(it, ft, k.W, k.H);
  if (const unsigned char* quiet = bg_decide(bg)) k.busy = quiet + ptk::atrous_flag_offset(si, k.W, 0, k.H);
  switch (kernel) {
    case kAtExact: *launch = launch_atrous_exact(k, g.stream); break;
    case kAtSimple: *launch = launch_atrous_simple(k, g.stream); break;
    case kAtStep: *launch = launch_atrous_step(k, g.stream); break;
    default: *launch = launch_atrous_fast(k, g.stream);
  }
  if (*launch == 0 && k.mod.p && kernel != kAtTiled) *launch = launch_modulate_after(k, g.stream);
  bg.finish(p, si < 0 ? 0 : si, *launch == 0);
  return PT_OK;
}

int draw_modulate(Pass* p, int y0, int y1, int* launch) {
  ModulateParams k;
  draw_header(p, y0, y1, &k);
  TRY(in_plane(p, "gAlbedo", &k.albedo));
  TRY(in_plane(p, "gEmission", &k.emission));
  TRY(in_plane(p, "gIllumination", &k.illum));
  TRY(in_plane(p, "gNormalAndLinearZ", &k.nd));
  TRY(att_plane(p, 0, &k.out));
  *launch = launch_modulate(k, g.stream);
  return PT_OK;
}

int draw_output(Pass* p, int y0, int y1, int* launch) {
  OutputParams k;
  draw_header(p, y0, y1, &k);
  TRY(in_plane(p, "texPass0", &k.in));
  if (p->att.empty()) return PT_OK;  // default framebuffer: nothing to keep
  TRY(att_plane(p, 0, &k.out));
  *launch = launch_output(k, g.stream);
  return PT_OK;
}

int draw_taa(Pass* p, int y0, int y1, int* launch) {
  TAAParams k;
  draw_header(p, y0, y1, &k);
  TRY(in_plane(p, "currentColor", &k.cur));
  TRY(in_plane(p, "previousColor", &k.prev));
  TRY(in_plane(p, "velocityTexture", &k.vel));
  TRY(in_plane(p, "normal_depth", &k.nd));
  TRY(att_plane(p, 0, &k.out));
  k.frameCounter = uu(p, "frameCounter", 0);
  *launch = launch_taa(k, g.stream);
  return PT_OK;
}

int draw_blit(Pass* p, int y0, int y1) {
  if (p->att.empty()) return err(PT_ERR_ARG, "bilt pass without attachment");
  return copy_plane(tex_of(p->att[0]), sampler(p, "in_texture"), p, y0, y1);
}

int draw_save(Pass* p, int y0, int y1) {
  const char* names[5] = {"texPass0", "texPass1", "texPass2", "accColor", "taaOutput"};
  for (int i = 0; i < 5 && i < (int)p->att.size(); ++i)
    TRY(copy_plane(tex_of(p->att[i]), sampler(p, names[i]), p, y0, y1));
  return PT_OK;
}

}  // namespace

namespace ptapi {

int draw_svgf(Pass* p, int kind) {
  int y0, y1;
  rows_of(p, &y0, &y1);
  int launch = 0;  // the kind's kernel launch: a hipError_t
  switch (kind) {
    case PK_REPROJECT: TRY(draw_reproject(p, y0, y1, &launch)); break;
    case PK_VARIANCE: TRY(draw_variance(p, y0, y1, &launch)); break;
    case PK_ATROUS: TRY(draw_atrous(p, y0, y1, &launch)); break;
    case PK_MODULATE: TRY(draw_modulate(p, y0, y1, &launch)); break;
    case PK_OUTPUT: TRY(draw_output(p, y0, y1, &launch)); break;
    case PK_TAA: TRY(draw_taa(p, y0, y1, &launch)); break;
    case PK_BLIT: TRY(draw_blit(p, y0, y1)); break;
    case PK_SAVE: TRY(draw_save(p, y0, y1)); break;
  }
  return launch ? hip_err((hipError_t)launch, "kernel launch") : PT_OK;
}

}  // namespace ptapi


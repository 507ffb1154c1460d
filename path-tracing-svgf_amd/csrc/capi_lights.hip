// capi_lights.hip — point lights that move (DESIGN.md "Moving point lights"): pt_lights_update and the diagnostics of
// include/ptsvgf_debug_lights.h. The buffer's device versions are a Versions (capi_state.h). The per-light
// consequences are drawn where the draws are issued (capi_draw_pt.hip's point_bins_for, capi_static.hip's
// point_cache_mode_for) from the position stamps kept here; the rules themselves are lights_key.h's.
#include "../../include/ptsvgf_debug_lights.h"
#include "capi_state.h"

using namespace ptapi;

namespace ptapi {

void free_lights(Texture* t) {
  LightVersions* v = t->lights;
  if (!v) return;
  (void)hipDeviceSynchronize();  // its readers may run on any stream
  v->free();                     // (the current version is t->dev)
  delete v;
  t->lights = nullptr;
  t->dev = nullptr;
}

}  // namespace ptapi

extern "C" {

int pt_lights_update(uint32_t lights_tex, int first, int count, const float* pos_rgb6) {
  if (!pos_rgb6 || first < 0 || count < 0) return err(PT_ERR_ARG, "pt_lights_update: null data or a negative range");
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(lights_tex);
  if (!t || t->target != PT_TEXTURE_BUFFER) return err(PT_ERR_INVALID_HANDLE, "pt_lights_update: not a texture buffer");
  const size_t lb = 6 * sizeof(float);
  const int nl = (int)(t->bytes / lb);
  if (first > nl || count > nl - first) return err(PT_ERR_ARG, "pt_lights_update: the range lies outside the buffer");
  if (count == 0) return PT_OK;
  if (!t->owned || !t->dev || t->host.size() != t->bytes || t->lbvh || t->trees || t->refit)
    return err(PT_ERR_STATE, "pt_lights_update: not a lights buffer pt_texbuffer_create made");
  if (!t->lights) {
    t->lights = new LightVersions();
    t->lights->pos_stamp.assign((size_t)nl, 0);
  }
  LightVersions& v = *t->lights;
  hipStream_t up = v.stream();
  if (!up) return hip_err(hipGetLastError(), "pt_lights_update: the copies' stream");
  // a version nothing in flight reads (on failure the texture keeps pointing where it pointed)
  if (const hipError_t e = v.next(t->dev, t->bytes))
    return hip_err(e, "pt_lights_update: a new version of the lights buffer");
  void* stage = v.stage(t->bytes);
  if (!stage) return hip_err(hipGetLastError(), "pt_lights_update: pinned staging");
  const uint64_t ver = t->version + 1;
  for (int i = 0; i < count; ++i) {
    uint8_t* dst = t->host.data() + (size_t)(first + i) * lb;
    const uint8_t* src = (const uint8_t*)(pos_rgb6 + 6 * (size_t)i);
    if (memcmp(dst, src, 3 * sizeof(float)) != 0) v.pos_stamp[(size_t)(first + i)] = ver;  // bitwise: -0 != +0
    memcpy(dst, src, lb);
  }
  memcpy(stage, t->host.data(), t->bytes);
  // on a stream of its own, so that a draw waits for this copy (its event: pt_params) and not for whatever else the
  // stream that happened to be current has queued; no host wait anywhere
  HIPCHK(hipMemcpyAsync(v.sb.buf, stage, t->bytes, hipMemcpyHostToDevice, up));
  HIPCHK(v.sb.mark_built(up));
  t->dev = v.sb.buf;
  t->version = ver;
  return PT_OK;
}

// ------------------------------------------------------------ diagnostics (ptsvgf_debug_lights.h) ---
int pt_debug_lights_moved_mask(const uint64_t* pos_stamps, int nl, uint64_t since, uint32_t* mask) {
  if (!pos_stamps || !mask || nl < 0) return err(PT_ERR_ARG, "pt_debug_lights_moved_mask: null argument");
  *mask = ptk::lights_moved_mask(pos_stamps, nl, since);
  return PT_OK;
}

int pt_debug_lights_settle(const uint64_t* stamps, int ndraws, int settle, int* actions) {
  if (!stamps || !actions || ndraws < 0) return err(PT_ERR_ARG, "pt_debug_lights_settle: null argument");
  ptk::LightBinsState s;
  for (int i = 0; i < ndraws; ++i) actions[i] = ptk::light_bins_step(s, stamps[i], settle);
  return PT_OK;
}

int pt_debug_lights_key_mode(const uint64_t* last, int last_valid, const uint64_t* now, int words, int stage_reused,
                             int enabled, int* mode, int* forget) {
  if (!last || !now || !mode || !forget) return err(PT_ERR_ARG, "pt_debug_lights_key_mode: null argument");
  if (words != (int)ptk::kLkWords) return err(PT_ERR_ARG, "pt_debug_lights_key_mode: not the key's word count");
  ptk::PointCache c;
  c.key = ptk::key_from<ptk::LightsKey>(last);
  c.valid = last_valid != 0;
  bool f = false;
  *mode = ptk::point_cache_mode_lights(c, ptk::key_from<ptk::LightsKey>(now), stage_reused != 0, !enabled, &f);
  *forget = f ? 1 : 0;
  return PT_OK;
}

int pt_debug_lights_key_field(int which) {
  switch (which) {
    case 0: return (int)ptk::kLkLightHandle;
    case 1: return (int)ptk::kLkLightDev;
    case 2: return (int)ptk::kLkLightVer;
    case 3: return (int)ptk::kLkPointBins;
    case 4: return (int)ptk::kLkPointBinsDev;
    default: return err(PT_ERR_ARG, "pt_debug_lights_key_field: 0 .. 4");
  }
}

int pt_debug_lights_state(uint32_t lights_tex, uint64_t* version, uint64_t* pos_stamps, int cap, int* device_versions) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(lights_tex);
  if (!t || t->target != PT_TEXTURE_BUFFER) return err(PT_ERR_INVALID_HANDLE, "pt_debug_lights_state: not a texture buffer");
  if (version) *version = t->version;
  const int nl = (int)(t->bytes / (6 * sizeof(float)));
  for (int l = 0; pos_stamps && l < cap; ++l)
    pos_stamps[l] = (t->lights && l < nl) ? t->lights->pos_stamp[(size_t)l] : 0;
  if (device_versions) *device_versions = (t->lights && t->lights->edited()) ? t->lights->count() : 1;
  return PT_OK;
}

int pt_debug_point_cache_forgotten(uint32_t pass, uint32_t* mask) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_PATHTRACE)
    return err(PT_ERR_ARG, "pt_debug_point_cache_forgotten: a path-tracing pass");
  if (!mask) return err(PT_ERR_ARG, "pt_debug_point_cache_forgotten: null argument");
  *mask = p->lcache_last_forgot;
  return PT_OK;
}

int pt_debug_point_bins_read(uint32_t tri_tex, uint32_t node_tex, int light, int32_t* hdr, size_t hdr_cap,
                             uint32_t* ent, size_t ent_cap, int* entries) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto it = g.scenes.find({tri_tex, node_tex});
  if (it == g.scenes.end() || !it->second.pbins.sb.buf)
    return err(PT_ERR_STATE, "pt_debug_point_bins_read: no point-light bins built for this scene");
  const PointBinsGPU& m = it->second.pbins;
  if (light < 0 || light >= m.nl) return err(PT_ERR_ARG, "pt_debug_point_bins_read: no such light");
  HIPCHK(hipDeviceSynchronize());
  int f[ptk::kPointBinsInfo];
  HIPCHK(hipMemcpy(f, m.dev.info + light * ptk::kPointBinsInfo, sizeof(f), hipMemcpyDeviceToHost));
  const int n = f[0] ? 0 : std::min(std::max(f[1], 0), m.dev.cap);  // no usable lists: nothing to read
  if (entries) *entries = f[0] ? -1 : n;
  const size_t n1 = (size_t)6 * m.R * m.R + 1;
  size_t ho = 0, eo = 0;
  ptk::point_bins_sections(m.ntris, m.nl, m.R, m.tight, light, &ho, &eo);
  if (hdr) {
    if (hdr_cap < 2 * n1) return err(PT_ERR_ARG, "pt_debug_point_bins_read: hdr needs 2 ints per cell and 2 more");
    HIPCHK(hipMemcpy(hdr, (const char*)m.sb.buf + ho, n1 * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  if (ent && n > 0) {
    if (ent_cap < 2 * (size_t)n) return err(PT_ERR_ARG, "pt_debug_point_bins_read: ent needs 2 words per entry");
    HIPCHK(hipMemcpy(ent, (const char*)m.sb.buf + eo, (size_t)n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return PT_OK;
}

}  // extern "C"

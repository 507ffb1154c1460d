// capi_environment.hip — the environment edited in place (DESIGN.md "Environment edits"): pt_environment_update and the
// diagnostic of include/ptsvgf_debug_environment.h. The (hdrMap, hdrCache) pair's device versions are a Versions with
// a second set-aside buffer (EnvVersions, capi_state.h); the importance cache is built on the device
// (kernels_environment.hip). The draws read a version where they bind the pair (capi_draw_pt.hip's pt_params).
#include "../../include/ptsvgf_debug_environment.h"
#include "capi_state.h"

using namespace ptapi;

namespace ptapi {

void free_environment(Texture* t) {
  EnvVersions* v = t->env;
  if (!v) return;
  (void)hipDeviceSynchronize();  // the builds' stream, and the versions' readers on any stream
  Texture* pair[2] = {tex_of(v->hdr_handle), tex_of(v->cache_handle)};
  void* first[2] = {v->take_first(), v->first_cache};
  for (int i = 0; i < 2; ++i) {
    Texture* p = pair[i];
    if (!p || p->env != v) continue;
    if (first[i]) {  // its texels lie in a version: back into the buffer the texture was created with
      (void)hipMemcpy(first[i], p->dev, v->plane(), hipMemcpyDeviceToDevice);
      p->dev = first[i];
      first[i] = nullptr;
    }
    p->env = nullptr;
  }
  for (void* f : first)
    if (f) (void)hipFree(f);
  v->free();
  if (v->scratch) (void)hipFree(v->scratch);
  if (v->src_done) (void)hipEventDestroy(v->src_done);
  delete v;
}

}  // namespace ptapi

extern "C" {

int pt_environment_update(uint32_t hdr_tex, uint32_t cache_tex, const void* rgb, int width, int height, int on_device) {
  if (!rgb) return err(PT_ERR_ARG, "pt_environment_update: null data");
  if (hdr_tex == cache_tex) return err(PT_ERR_ARG, "pt_environment_update: hdr_tex and cache_tex are one texture");
  if (width < 1 || height < 1 || width > ptk::kEnvMaxSide || height > ptk::kEnvMaxSide)
    return err(PT_ERR_ARG, "pt_environment_update: width and height lie in 1 .. 8192");
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* th = tex_of(hdr_tex);
  Texture* tc = tex_of(cache_tex);
  if (!th || !tc || th->target != PT_TEXTURE_2D || tc->target != PT_TEXTURE_2D)
    return err(PT_ERR_INVALID_HANDLE, "pt_environment_update: not a 2-D texture");
  if (!th->owned || !tc->owned || !th->dev || !tc->dev)
    return err(PT_ERR_STATE, "pt_environment_update: a wrapped texture has no versions");
  if (th->rows != th->H || tc->rows != tc->H || th->row0 != 0 || tc->row0 != 0)
    return err(PT_ERR_STATE, "pt_environment_update: a texture that stores a band of its rows");
  if (width != th->W || height != th->H || width != tc->W || height != tc->H)
    return err(PT_ERR_ARG, "pt_environment_update: not both textures' size (a new size: pt_texture2d_upload)");
  // (a texture that was updated with another partner: that pair's versions go first. It waits for the device; rare)
  if (th->env != tc->env || (th->env && th->env->hdr_handle != hdr_tex)) {
    free_environment(th);
    free_environment(tc);
  }
  const int n = width * height;
  EnvVersions* v = th->env;
  if (!v) {
    std::unique_ptr<EnvVersions> nv(new EnvVersions());
    nv->hdr_handle = hdr_tex;
    nv->cache_handle = cache_tex;
    nv->W = width;
    nv->H = height;
    HIPCHK(hipMalloc((void**)&nv->scratch, ptk::environment_scratch_floats(width, height) * sizeof(float)));
    v = th->env = tc->env = nv.release();  // (what it lacks still is had below, or by the next update)
  }
  hipStream_t up = v->stream();
  if (!up) return hip_err(hipGetLastError(), "pt_environment_update: the builds' stream");
  if (!v->src_done) HIPCHK(hipEventCreateWithFlags(&v->src_done, hipEventDisableTiming));
  // a version nothing in flight reads; the first update sets both textures' own buffers aside
  const size_t plane = v->plane();
  const bool created = !v->edited();
  if (const hipError_t e = v->next(th->dev, 3 * plane))
    return hip_err(e, "pt_environment_update: a new version of the environment");
  if (created) v->first_cache = tc->dev;
  float4* hdr = (float4*)v->sb.buf;
  float4* cache = (float4*)((char*)v->sb.buf + plane);
  float4* merged = (float4*)((char*)v->sb.buf + 2 * plane);
  int rc = 0;
  if (on_device) {
    // consumed on the current stream, in its order; everything else runs on the builds' stream behind that
    rc = ptk::launch_environment_expand((const float*)rgb, hdr, n, g.stream);
    if (rc) return hip_err((hipError_t)rc, "pt_environment_update: expand");
    HIPCHK(hipEventRecord(v->src_done, g.stream));
    HIPCHK(hipStreamWaitEvent(up, v->src_done, 0));
  } else {
    const size_t bytes = (size_t)n * 3 * sizeof(float);
    void* stage = v->stage(bytes);  // W x H RGB texels
    if (!stage) return hip_err(hipGetLastError(), "pt_environment_update: pinned staging");
    memcpy(stage, rgb, bytes);
    // the RGB texels pass through the version's cache plane, which the last kernel of the build overwrites
    HIPCHK(hipMemcpyAsync(cache, stage, bytes, hipMemcpyHostToDevice, up));
    rc = ptk::launch_environment_expand((const float*)cache, hdr, n, up);
    if (rc) return hip_err((hipError_t)rc, "pt_environment_update: expand");
  }
  rc = ptk::launch_environment_cache(hdr, cache, merged, v->scratch, width, height, up);
  if (rc) return hip_err((hipError_t)rc, "pt_environment_update: cache");
  HIPCHK(v->sb.mark_built(up));
  th->dev = hdr;
  tc->dev = cache;
  tex_written(th);
  tex_written(tc);
  v->vh = th->version;
  v->vc = tc->version;
  return PT_OK;
}

int pt_debug_environment_state(uint32_t hdr_tex, uint64_t* version, int* device_versions, int* staging_slots) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(hdr_tex);
  if (!t || t->target != PT_TEXTURE_2D) return err(PT_ERR_INVALID_HANDLE, "pt_debug_environment_state: not a 2-D texture");
  const EnvVersions* v = t->env;
  if (version) *version = t->version;
  if (device_versions) *device_versions = (v && v->edited()) ? v->count() : 1;
  if (staging_slots) *staging_slots = v ? (int)v->staging.size() : 0;
  return PT_OK;
}

}  // extern "C"

// capi.hip — implementation of include/ptsvgf.h: the GL-plumbing-shaped C ABI
// (Utils/render_pass.h:82-182, Utils/shader.h:21-67, Utils/help_func.h:22-32)
// over HIP device memory and the gfx950 kernels: the object model (handles, textures, passes, uniforms, streams) and
// the pt_* entry points over it. pt_pass_draw and pt_pass_draw_batch only dispatch: the path tracer's draws are in
// capi_draw_pt.hip, the G-buffer's and the SVGF chain's in capi_draw_svgf.hip. The entry points of geometry that moves
// (builds, refits, raster binds, poses) are in capi_geometry.hip, those of lights that move in capi_lights.hip, those
// of materials edited in place in capi_materials.hip, and the static view's bookkeeping (keys, caches, quiet-tile
// sets; the draws call into it) in capi_static.hip; capi_state.h holds what they share.
//
// GL semantics kept:
//  * RenderPass uniforms are set by name; an unknown name is silently ignored;
//  * set_texture_uniform binds to the pass's next texture slot; a sampler that
//    was never bound reads texture unit 0, i.e. the texture most recently bound
//    to slot 0 by any pass (GL's global unit state);
//  * draw() is ordered after every previous draw (one in-order HIP stream);
//  * scene texture buffers are decoded once per (buffer, version) into the
//    kernels' SoA records (pt_device.h) on first use, like a driver upload.
#include <cstdio>
#include <algorithm>
#include <cstring>

#include "../../include/ptsvgf_debug_pointbins.h"
#include "../../include/ptsvgf_scene.h"
#include "capi_state.h"
#include "host_trees.h"
#include "pb_overlap.h"

static thread_local std::string g_err;

// the state and helpers capi_state.h declares
namespace ptapi {

Lib g;
std::recursive_mutex g_mu;
ptk::LbvhWork g_lbvh;

int err(int code, const std::string& m) {
  g_err = m;
  return code;
}
int hip_err(hipError_t e, const char* what) {
  return err(PT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

Texture* tex_of(uint32_t h) {
  auto it = g.textures.find(h);
  return it == g.textures.end() ? nullptr : it->second.get();
}
Pass* pass_of(uint32_t h) {
  auto it = g.passes.find(h);
  return it == g.passes.end() ? nullptr : it->second.get();
}

int ensure_init() {
  if (g.init) return PT_OK;
  return err(PT_ERR_STATE, "pt_init() has not been called");
}

// The host mirror of a texbuffer pt_bvh_refit wrote in place is lazy: the refit pays no copy, and whoever reads
// t->host's contents calls this first (pt_debug_lbvh_trees source 1, get_scene's host decode; pt_texture_readback
// reads the device copy, and get_scene_lbvh only the sizes, which a refit keeps).
int refresh_host(Texture* t) {
  if (!t->host_stale) return PT_OK;
  HIPCHK(hipDeviceSynchronize());
  t->host.resize(t->bytes);
  if (t->bytes) HIPCHK(hipMemcpy(t->host.data(), t->dev, t->bytes, hipMemcpyDeviceToHost));
  t->host_stale = false;
  return PT_OK;
}

// -------------------------------------------------------------- bindings ---
const Uniform* U(Pass* p, const char* name, int type) {
  auto it = p->uni.find(name);
  if (it == p->uni.end()) return nullptr;
  return it->second.type == type ? &it->second : nullptr;
}
int ui(Pass* p, const char* n, int def) {
  auto it = p->uni.find(n);
  if (it == p->uni.end()) return def;
  if (it->second.type == 2 || it->second.type == 4) return it->second.i;
  if (it->second.type == 3) return (int)it->second.u;
  return def;
}
Texture* sampler(Pass* p, const char* name, uint32_t* handle) {
  auto it = p->tex.find(name);
  uint32_t h = it != p->tex.end() ? it->second : g.unit0;
  if (handle) *handle = h;
  return tex_of(h);
}

// pt_set_band holds a partition of W x H frames: a band or stored rows that are not the whole frame
bool band_partition(int W, int H) {
  return g.band_h > 0 && W == g.band_w && H == g.band_h &&
         (g.band_y0 != 0 || g.band_y1 != H || g.band_row0 != 0 || g.band_rows != H);
}

void rows_of(Pass* p, int* y0, int* y1) {
  if (p->y_begin >= 0) {
    *y0 = p->y_begin;
    *y1 = p->y_end;
  } else if (g.band_h > 0 && p->W == g.band_w && p->H == g.band_h) {
    *y0 = g.band_y0;
    *y1 = g.band_y1;
  } else {
    *y0 = 0;
    *y1 = p->H;
  }
}

float uf(Pass* p, const char* n, float def) {
  const Uniform* u = U(p, n, 1);
  return u ? u->f[0] : def;
}
uint32_t uu(Pass* p, const char* n, uint32_t def) {
  auto it = p->uni.find(n);
  if (it == p->uni.end()) return def;
  if (it->second.type == 3) return it->second.u;
  if (it->second.type == 2 || it->second.type == 4) return (uint32_t)it->second.i;
  return def;
}

// A sampler the host bound by name (no texture-unit-0 fallback): optional inputs with no GL counterpart.
Texture* bound_sampler(Pass* p, const char* name) {
  auto it = p->tex.find(name);
  return it != p->tex.end() ? tex_of(it->second) : nullptr;
}

int plane_of(Texture* t, Pass* p, ptk::Plane* out, const char* what) {
  if (!t || t->target != PT_TEXTURE_2D || !t->dev)
    return err(PT_ERR_MISSING_TEXTURE, std::string("pass needs 2-D texture '") + what + "'");
  if (t->W != p->W || t->H != p->H)
    return err(PT_ERR_ARG, std::string("texture '") + what + "' size differs from the pass size");
  out->p = (float4*)t->dev;
  out->aux = t->aux_valid ? t->aux : nullptr;
  out->W = t->W;
  out->row0 = t->row0;
  out->rows = t->rows;
  return PT_OK;
}
int att_plane(Pass* p, int k, ptk::Plane* out) {
  if ((int)p->att.size() <= k) return err(PT_ERR_ARG, "pass has too few color attachments");
  Texture* t = tex_of(p->att[k]);
  int rc = plane_of(t, p, out, "color attachment");
  if (rc != PT_OK) return rc;
  tex_written(t);  // (a draw into it by any pass)
  return PT_OK;
}

// drops a merged environment: its buffers (the caller has synchronised the streams that read them) and events
void free_hdr_merged(HdrMerged& m) {
  m.sb.free();
  m = HdrMerged{};
}

// the trees a GPU-built scene borrowed from its node texture are that texture's to free (free_trees)
void drop_borrowed(SceneGPU& sg) {
  if (!sg.lbvh) return;
  sg.bvh = sg.bvh4 = sg.bvh_any = sg.leaves = nullptr;
  sg.lbvh = false;
}

}  // namespace ptapi

using namespace ptapi;

namespace {

using namespace ptk;

std::string basename_of(const char* p) {
  std::string s(p ? p : "");
  size_t k = s.find_last_of("/\\");
  return k == std::string::npos ? s : s.substr(k + 1);
}

// drops a scene's point-light bins (the caller has synchronised the streams that read them)
void free_point_bins(PointBinsGPU& m) {
  m.sb.free();
  m = PointBinsGPU{};
}

void free_scene(SceneGPU& sg) {
  if (sg.pbins.sb.any()) (void)hipDeviceSynchronize();  // its readers may run on any stream
  free_point_bins(sg.pbins);
  drop_borrowed(sg);
  free_shade(sg);
  float4** bufs[5] = {&sg.geom, &sg.bvh, &sg.bvh4, &sg.bvh_any, &sg.leaves};
  for (auto b : bufs) {
    if (*b) (void)hipFree(*b);
    *b = nullptr;
  }
  if (sg.tri_leaf) (void)hipFree(sg.tri_leaf);
  sg.tri_leaf = nullptr;
  sg.tri_leaf_cap = 0;
}

// what a texture holds on the device (pt_texture_destroy, pt_shutdown: nothing in flight reads it)
void free_texture(Texture* t) {
  free_lights(t);       // every version of an updated lights buffer (dev is one of them)
  free_environment(t);  // of an updated environment: both textures get their own buffers back
  if (t->owned && t->dev) (void)hipFree(t->dev);
  if (t->aux) (void)hipFree(t->aux);
  if (t->tflags) (void)hipFree(t->tflags);
  free_trees(t);  // (pt_texture_destroy drops the scenes that borrowed them)
  free_refit(t);
}

// Every SharedBuf that lives: the merged environments, every scene's point-light bins and shade versions, every
// texture's light and environment versions (a pair's twice: both textures hold it). Whatever keeps one adds it here.
template <class F>
void each_shared(F f) {
  for (auto& kv : g.hdr_merged) f(kv.second.sb);
  for (auto& kv : g.scenes) {
    f(kv.second.pbins.sb);
    f(kv.second.shade.sb);
  }
  for (auto& kv : g.textures) {
    if (kv.second->lights) f(kv.second->lights->sb);
    if (kv.second->env) f(kv.second->env->sb);
  }
}

// the stored rows of a new w x h image of 2-D texture t: the band's under a pt_set_band of that size, else all
void store_rows(Texture* t, int w, int h) {
  const bool band = g.band_h > 0 && w == g.band_w && h == g.band_h;
  t->W = w;
  t->H = h;
  t->row0 = band ? g.band_row0 : 0;
  t->rows = band ? g.band_rows : h;
  t->bytes = (size_t)w * t->rows * 16;
}

// what a pass holds on the device (pt_pass_destroy, pt_shutdown: nothing in flight reads it)
void free_pass(Pass* p) {
  if (p->raster.geom) (void)hipFree(p->raster.geom);
  if (p->raster.nrm) (void)hipFree(p->raster.nrm);
  if (p->raster.disp) (void)hipFree(p->raster.disp);
  if (p->raster.bvh) (void)hipFree(p->raster.bvh);
  free_raster_refit(p->raster);
  if (p->bins.base) (void)hipFree(p->bins.base);
  if (p->wf.base) (void)hipFree(p->wf.base);
  if (p->wf.spill) (void)hipFree(p->wf.spill);
  if (p->order.cost) (void)hipFree(p->order.cost);
  if (p->order.perm) (void)hipFree(p->order.perm);
  if (p->busy) (void)hipFree(p->busy);
  if (p->ev0) (void)hipEventDestroy(p->ev0);
  if (p->ev1) (void)hipEventDestroy(p->ev1);
}

Uniform* set_u(uint32_t pass, const char* name, int type, int* rc) {
  *rc = ensure_init();
  if (*rc != PT_OK) return nullptr;
  Pass* p = pass_of(pass);
  if (!p) { *rc = err(PT_ERR_INVALID_HANDLE, "invalid pass"); return nullptr; }
  if (!name) { *rc = err(PT_ERR_ARG, "null uniform name"); return nullptr; }
  Uniform& u = p->uni[name];
  u.type = type;
  return &u;
}

// The gMotion and gNormalAndLinearZ textures of pt_sample_counts_derive / _pool (`fn`: the entry point's name, as the
// messages carry it): two whole-frame 2-D textures of one size.
int sample_count_planes(const char* fn, uint32_t motion_tex, uint32_t nd_tex, Texture** mt_out, Texture** nt_out) {
  Texture* mt = tex_of(motion_tex);
  Texture* nt = tex_of(nd_tex);
  const std::string f(fn);
  if (!mt || !nt || mt->target != PT_TEXTURE_2D || nt->target != PT_TEXTURE_2D || !mt->dev || !nt->dev)
    return err(PT_ERR_MISSING_TEXTURE, f + " needs the 2-D textures gMotion and gNormalAndLinearZ");
  if (mt->W != nt->W || mt->H != nt->H) return err(PT_ERR_ARG, f + ": textures of different sizes");
  if (band_partition(mt->W, mt->H) || mt->row0 != 0 || nt->row0 != 0 || mt->rows != mt->H || nt->rows != nt->H)
    return err(PT_ERR_STATE, f + ": not under a pt_set_band partition");
  *mt_out = mt;
  *nt_out = nt;
  return PT_OK;
}

// pt_pass_draw / pt_pass_draw_batch: `draw` between the two events of pass p when pt_set_profiling is on (a draw that
// fails leaves the pass's last timing as it was)
template <class Draw>
int timed_draw(Pass* p, Draw draw) {
  if (g.profiling) {
    if (!p->ev0) { HIPCHK(hipEventCreate(&p->ev0)); HIPCHK(hipEventCreate(&p->ev1)); }
    HIPCHK(hipEventRecord(p->ev0, g.stream));
  }
  TRY(draw());
  if (g.profiling) {
    HIPCHK(hipEventRecord(p->ev1, g.stream));
    p->timed = true;
  }
  return PT_OK;
}

}  // namespace

// ================================================================= C ABI ===
extern "C" {

int pt_tree_check(const float* node_enc, int nnodes, const float* tri_enc, int ntris, int collapse, int treelet,
                  double* out, int nout) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  std::string msg;
  const int rc = tree_check(node_enc, nnodes, tri_enc, ntris, collapse, treelet, out, nout, &msg);
  return rc ? err(rc, msg) : PT_OK;
}

const char* pt_last_error(void) { return g_err.c_str(); }
int pt_version(void) { return 1; }

int pt_init(int device) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (g.init) return PT_OK;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return err(PT_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return err(PT_ERR_ARG, "device index out of range");
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&g.own, hipStreamNonBlocking));
  if (PT_WIDE_SIGNED) {
    const int sub = ptk::subnormal_probe(g.own);
    if (sub != 1) {
      (void)hipStreamDestroy(g.own);
      g.own = nullptr;
      return sub == 0 ? err(PT_ERR_STATE, "walk kernels flush f32 subnormals: PT_WIDE_SIGNED needs them kept")
                      : err(PT_ERR_HIP, "subnormal probe failed");
    }
  }
  g.stream = g.own;
  g.device = device;
  g.init = true;
  return PT_OK;
}

int pt_shutdown(void) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (!g.init) return PT_OK;
  (void)hipDeviceSynchronize();
  for (auto& kv : g.textures) free_texture(kv.second.get());
  for (auto& kv : g.passes) free_pass(kv.second.get());
  for (auto& kv : g.poses) free_pose(*kv.second);
  for (auto& kv : g.scenes) free_scene(kv.second);
  free_materials();
  free_rays();
  for (auto& kv : g.hdr_merged) free_hdr_merged(kv.second);
  g.hdr_merged.clear();
  for (QuietSet& q : g.bg_sets)
    if (q.flags) (void)hipFree(q.flags);
  for (auto& kv : g.forks) {
    (void)hipEventDestroy(kv.second.fork);
    (void)hipEventDestroy(kv.second.join);
    (void)hipStreamDestroy(kv.second.side);
  }
  g.forks.clear();
  if (g_lbvh.base) (void)hipFree(g_lbvh.base);
  g_lbvh = ptk::LbvhWork{};
  if (g.own) (void)hipStreamDestroy(g.own);
  g = Lib();
  return PT_OK;
}

int pt_set_stream(void* s) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  // s is used as given: NULL is the HIP default (null) stream, which is torch's default stream.
  g.stream = (hipStream_t)s;
  return PT_OK;
}

int pt_stream_release(void* s) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  hipStream_t st = (hipStream_t)s;
  if (st == g.own) return err(PT_ERR_ARG, "the library's own stream is not released");
  auto it = g.forks.find(st);
  if (it != g.forks.end()) {  // its side stream's work was joined into st; wait for that side stream only
    (void)hipStreamSynchronize(it->second.side);
    (void)hipEventDestroy(it->second.fork);
    (void)hipEventDestroy(it->second.join);
    (void)hipStreamDestroy(it->second.side);
    g.forks.erase(it);
  }
  // the stream's last reads of every shared buffer: done before the entry goes
  each_shared([st](SharedBuf& sb) { sb.forget(st); });
  if (g.stream == st) g.stream = g.own;
  return PT_OK;
}

int pt_stream_create_cu_masked(uint32_t words, const uint32_t* mask, void** out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!mask || !out || words == 0) return err(PT_ERR_ARG, "CU mask and output needed");
  hipStream_t s = nullptr;
  HIPCHK(hipExtStreamCreateWithCUMask(&s, words, mask));  // (the size counts uint32 words)
  *out = (void*)s;
  return PT_OK;
}

int pt_stream_create_priority(int priority, void** out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!out) return err(PT_ERR_ARG, "output needed");
  int least = 0, greatest = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  // numerically lower = higher priority; clamp into [greatest, least]
  priority = std::min(std::max(priority, std::min(least, greatest)), std::max(least, greatest));
  hipStream_t s = nullptr;
  HIPCHK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority));
  *out = (void*)s;
  return PT_OK;
}

int pt_stream_priority_range(int* least, int* greatest) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!least || !greatest) return err(PT_ERR_ARG, "null output");
  HIPCHK(hipDeviceGetStreamPriorityRange(least, greatest));
  return PT_OK;
}

int pt_stream_destroy(void* s) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!s) return err(PT_ERR_ARG, "null stream");
  TRY(pt_stream_release(s));
  HIPCHK(hipStreamSynchronize((hipStream_t)s));
  HIPCHK(hipStreamDestroy((hipStream_t)s));
  return PT_OK;
}

int pt_device_cus(int* n) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!n) return err(PT_ERR_ARG, "null output");
  HIPCHK(hipDeviceGetAttribute(n, hipDeviceAttributeMultiprocessorCount, g.device));
  return PT_OK;
}

int pt_use_own_stream(void) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  g.stream = g.own;
  return PT_OK;
}

int pt_sync(void) {
  TRY(ensure_init());
  HIPCHK(hipStreamSynchronize(g.stream));
  return PT_OK;
}

int pt_set_band(int fw, int fh, int y0, int y1, int row0, int rows) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  if (fw <= 0 || fh <= 0 || y0 < 0 || y1 > fh || y0 >= y1 || row0 < 0 || rows <= 0 || row0 + rows > fh ||
      row0 > y0 || row0 + rows < y1)
    return err(PT_ERR_ARG, "pt_set_band: inconsistent band");
  g.band_w = fw; g.band_h = fh; g.band_y0 = y0; g.band_y1 = y1; g.band_row0 = row0; g.band_rows = rows;
  return PT_OK;
}

int pt_set_profiling(int on) {
  g.profiling = on != 0;
  return PT_OK;
}

int pt_program_create(const char* frag, const char* vert, uint32_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!out) return err(PT_ERR_ARG, "null out pointer");
  std::string f = basename_of(frag), v = basename_of(vert);
  static const std::map<std::string, int> kinds = {
      {"path_tracing.frag", PK_PATHTRACE}, {"svgf_reproject.frag", PK_REPROJECT},
      {"svgf_variance.frag", PK_VARIANCE}, {"svgf_Atrous.frag", PK_ATROUS},
      {"svgf_modulate.frag", PK_MODULATE}, {"bilt.frag", PK_BLIT},
      {"save_frame_data.frag", PK_SAVE},   {"output_pass.frag", PK_OUTPUT},
      {"taa.frag", PK_TAA},                {"rasterize_frag.frag", PK_RASTER}};
  auto it = kinds.find(f);
  if (it == kinds.end()) return err(PT_ERR_UNKNOWN_PROGRAM, "no HIP kernel for fragment shader '" + f + "'");
  const char* want = it->second == PK_RASTER ? "rasterize_vert.vert" : "vert.vert";
  if (v != want) return err(PT_ERR_UNKNOWN_PROGRAM, "'" + f + "' must be linked with '" + want + "'");
  uint32_t h = g.next++;
  g.programs[h] = it->second;
  *out = h;
  return PT_OK;
}

static int new_texture(std::unique_ptr<Texture> t, uint32_t* out) {
  uint32_t h = g.next++;
  g.textures[h] = std::move(t);
  *out = h;
  return PT_OK;
}

int pt_texture2d_create(int w, int h, uint32_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (w <= 0 || h <= 0 || !out) return err(PT_ERR_ARG, "pt_texture2d_create: bad size");
  auto t = std::make_unique<Texture>();
  store_rows(t.get(), w, h);
  HIPCHK(hipMalloc(&t->dev, t->bytes));
  HIPCHK(hipMemsetAsync(t->dev, 0, t->bytes, g.stream));  // GL leaves it undefined; the build zeroes
  return new_texture(std::move(t), out);
}

int pt_texture2d_wrap(void* ptr, int w, int h, uint32_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!ptr || w <= 0 || h <= 0 || !out) return err(PT_ERR_ARG, "pt_texture2d_wrap: bad argument");
  auto t = std::make_unique<Texture>();
  store_rows(t.get(), w, h);
  t->dev = ptr;
  t->owned = false;
  return new_texture(std::move(t), out);
}

int pt_texture2d_upload(uint32_t tex, int w, int h, uint32_t fmt, const float* data) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(tex);
  if (!t || t->target != PT_TEXTURE_2D) return err(PT_ERR_INVALID_HANDLE, "invalid 2-D texture");
  if (!data) return err(PT_ERR_ARG, "null data");
  if (fmt != PT_RGB32F && fmt != PT_RGBA32F && fmt != PT_RGB && fmt != PT_RGBA)
    return err(PT_ERR_FORMAT, "upload format must be RGB32F or RGBA32F");
  int nch = (fmt == PT_RGB32F || fmt == PT_RGB) ? 3 : 4;
  // a texture pt_environment_update wrote: a new size ends the pair's versions; else the copy below writes the
  // current version's plane where it lies, after the build that wrote it
  if (t->env && (w != t->W || h != t->H)) free_environment(t);
  if (t->env && t->env->sb.buf) HIPCHK(t->env->sb.wait_built(g.stream));
  if (w != t->W || h != t->H) {  // glTexImage2D respecifies the image
    if (t->owned && t->dev) HIPCHK(hipFree(t->dev));
    if (!t->owned) return err(PT_ERR_ARG, "cannot resize a wrapped texture");
    if (t->aux) (void)hipFree(t->aux);  // sized for the old image
    t->aux = nullptr;
    store_rows(t, w, h);
    HIPCHK(hipMalloc(&t->dev, t->bytes));
  }
  std::vector<float4> buf((size_t)w * t->rows);
  for (int r = 0; r < t->rows; ++r) {
    const float* src = data + ((size_t)(t->row0 + r) * w) * nch;
    for (int x = 0; x < w; ++x) {
      const float* q = src + (size_t)x * nch;
      buf[(size_t)r * w + x] = float4{q[0], q[1], q[2], nch == 4 ? q[3] : 1.0f};
    }
  }
  HIPCHK(hipMemcpyAsync(t->dev, buf.data(), t->bytes, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  tex_written(t);
  return PT_OK;
}

int pt_texture_upload_rgba(uint32_t tex, const float* data, size_t bytes) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(tex);
  if (!t || t->target != PT_TEXTURE_2D) return err(PT_ERR_INVALID_HANDLE, "invalid 2-D texture");
  if (!data || bytes != t->bytes) return err(PT_ERR_ARG, "upload size must equal the stored rows");
  if (t->env && t->env->sb.buf) HIPCHK(t->env->sb.wait_built(g.stream));  // (as pt_texture2d_upload)
  HIPCHK(hipMemcpyAsync(t->dev, data, bytes, hipMemcpyHostToDevice, g.stream));
  HIPCHK(hipStreamSynchronize(g.stream));
  tex_written(t);
  return PT_OK;
}

int pt_texbuffer_create(const void* data, size_t bytes, uint32_t fmt, uint32_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (fmt != PT_RGB32F) return err(PT_ERR_FORMAT, "texture buffers are RGB32F (main.cpp:142,151,168)");
  if ((!data && bytes) || bytes % 12 || !out) return err(PT_ERR_ARG, "texbuffer size must be whole RGB32F texels");
  auto t = std::make_unique<Texture>();
  t->target = PT_TEXTURE_BUFFER;
  t->bytes = bytes;
  t->W = (int)(bytes / 12);
  t->H = 1;
  t->rows = 1;
  if (bytes) {
    t->host.assign((const uint8_t*)data, (const uint8_t*)data + bytes);
    HIPCHK(hipMalloc(&t->dev, bytes));
    HIPCHK(hipMemcpy(t->dev, data, bytes, hipMemcpyHostToDevice));
  }
  return new_texture(std::move(t), out);
}

int pt_texture_readback_aux(uint32_t tex, float* host_out, size_t cap, size_t* bytes) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(tex);
  if (!t || t->target != PT_TEXTURE_2D) return err(PT_ERR_INVALID_HANDLE, "invalid 2-D texture");
  if (!bytes) return err(PT_ERR_ARG, "null bytes");
  *bytes = t->aux && t->aux_valid ? (size_t)t->W * t->rows * 4 : 0;
  if (!host_out || !*bytes) return PT_OK;
  if (cap < *bytes) return err(PT_ERR_ARG, "aux buffer too small");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_out, t->aux, *bytes, hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_point_bins_info(uint32_t tri_tex, uint32_t node_tex, int* info8x4, int* dims4, size_t* bytes) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto it = g.scenes.find({tri_tex, node_tex});
  if (it == g.scenes.end() || !it->second.pbins.sb.buf)
    return err(PT_ERR_STATE, "pt_point_bins_info: no point-light bins built for this scene");
  const PointBinsGPU& m = it->second.pbins;
  HIPCHK(hipDeviceSynchronize());
  if (info8x4) {
    memset(info8x4, 0, sizeof(int) * ptk::kPointBins * ptk::kPointBinsInfo);
    HIPCHK(hipMemcpy(info8x4, m.dev.info, sizeof(int) * m.nl * ptk::kPointBinsInfo, hipMemcpyDeviceToHost));
  }
  if (dims4) {
    dims4[0] = m.R;
    dims4[1] = m.nl;
    dims4[2] = m.dev.cap;
    dims4[3] = ptk::kPointBinsEntryBytes;
  }
  if (bytes) *bytes = m.sb.bytes;
  return PT_OK;
}

int pt_debug_point_bins_overlap(const float* px, const float* py, int n, float fw, int R, int cx0, int cy0, int cx1,
                                int cy1, uint8_t* kept, size_t cap, int* degenerate) {
  if (!px || !py || !kept || R < 1 || cx0 < 0 || cy0 < 0 || cx1 >= R || cy1 >= R || cx0 > cx1 || cy0 > cy1)
    return err(PT_ERR_ARG, "pt_debug_point_bins_overlap: bad box");
  const int bw = cx1 - cx0 + 1, bh = cy1 - cy0 + 1;
  if (cap < (size_t)bw * bh) return err(PT_ERR_ARG, "pt_debug_point_bins_overlap: kept is too small");
  ptk::PbEdges e;
  e.n = 0;
  const bool ok = ptk::pb_edges(px, py, n, &e);
  if (degenerate) *degenerate = ok ? 0 : 1;
  if (bw * bh <= 2) e.n = 0;  // (as pb_bin: a box of at most two cells keeps both)
  for (int cy = cy0; cy <= cy1; ++cy)
    for (int cx = cx0; cx <= cx1; ++cx) kept[(cy - cy0) * bw + (cx - cx0)] = ptk::pb_cell_kept(e, fw, cx, cy, R) ? 1 : 0;
  return PT_OK;
}

int pt_texarray_create(int w, int h, int layers, uint32_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (w <= 0 || h <= 0 || layers <= 0 || !out) return err(PT_ERR_ARG, "pt_texarray_create: bad size");
  auto t = std::make_unique<Texture>();
  t->target = PT_TEXTURE_2D_ARRAY;
  t->W = w; t->H = h; t->rows = h; t->layers = layers;
  t->bytes = (size_t)w * h * layers * 4;
  HIPCHK(hipMalloc(&t->dev, t->bytes));
  HIPCHK(hipMemset(t->dev, 0, t->bytes));
  return new_texture(std::move(t), out);
}

int pt_texarray_upload_layer(uint32_t tex, int layer, int w, int h, int ch, const uint8_t* data) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(tex);
  if (!t || t->target != PT_TEXTURE_2D_ARRAY) return err(PT_ERR_INVALID_HANDLE, "invalid texture array");
  if (!data || layer < 0 || layer >= t->layers || w > t->W || h > t->H || (ch != 3 && ch != 4))
    return err(PT_ERR_ARG, "pt_texarray_upload_layer: bad argument");
  // glTexSubImage3D at the origin (help_func.h:12): a w x h sub-rectangle of the layer
  std::vector<uint8_t> row((size_t)w * 4);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) {
      const uint8_t* q = data + ((size_t)y * w + x) * ch;
      row[4 * x] = q[0]; row[4 * x + 1] = q[1]; row[4 * x + 2] = q[2]; row[4 * x + 3] = ch == 4 ? q[3] : 255;
    }
    HIPCHK(hipMemcpy((char*)t->dev + (((size_t)layer * t->H + y) * t->W) * 4, row.data(), row.size(),
                     hipMemcpyHostToDevice));
  }
  t->version++;
  return PT_OK;
}

int pt_texture_readback(uint32_t tex, float* out, size_t bytes) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(tex);
  if (!t || !t->dev) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  if (!out || bytes < t->bytes) return err(PT_ERR_ARG, "readback buffer too small");
  HIPCHK(hipDeviceSynchronize());  // every stream: a frame may be in flight on another renderer's stream
  HIPCHK(hipMemcpy(out, t->dev, t->bytes, hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_texture_device_ptr(uint32_t tex, void** out) {
  Texture* t = tex_of(tex);
  if (!t || !out) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  *out = t->dev;
  return PT_OK;
}

int pt_texture_info(uint32_t tex, int* w, int* h, int* row0) {
  Texture* t = tex_of(tex);
  if (!t) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  if (w) *w = t->W;
  if (h) *h = t->rows;
  if (row0) *row0 = t->row0;
  return PT_OK;
}

int pt_texture_destroy(uint32_t tex) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  auto it = g.textures.find(tex);
  if (it == g.textures.end()) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  (void)hipStreamSynchronize(g.stream);
  free_texture(it->second.get());  // (the scenes that borrowed its trees are dropped below)
  g.textures.erase(it);
  for (auto hm = g.hdr_merged.begin(); hm != g.hdr_merged.end();) {  // merged environments built from it
    if (hm->first.first == tex || hm->first.second == tex) {
      (void)hipDeviceSynchronize();  // its readers may run on any stream
      free_hdr_merged(hm->second);
      hm = g.hdr_merged.erase(hm);
    } else {
      ++hm;
    }
  }
  // the device scenes decoded from this buffer (keyed by (triangles, nodes) handles) go with it
  for (auto sc = g.scenes.begin(); sc != g.scenes.end();) {
    if (sc->first.first == tex || sc->first.second == tex) {
      free_scene(sc->second);
      sc = g.scenes.erase(sc);
    } else {
      ++sc;
    }
  }
  return PT_OK;
}

int pt_pass_create(uint32_t program, int w, int h, uint32_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!g.programs.count(program)) return err(PT_ERR_INVALID_HANDLE, "invalid program");
  if (w <= 0 || h <= 0 || !out) return err(PT_ERR_ARG, "pt_pass_create: bad size");
  auto p = std::make_unique<Pass>();
  p->program = program;
  p->W = w;
  p->H = h;
  uint32_t hnd = g.next++;
  g.passes[hnd] = std::move(p);
  *out = hnd;
  return PT_OK;
}

int pt_pass_add_color_attachment(uint32_t pass, uint32_t tex) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (!tex_of(tex)) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  p->att.push_back(tex);
  return PT_OK;
}

int pt_pass_bind(uint32_t pass, int final_pass) {
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  p->bound = true;
  p->final_pass = final_pass != 0;
  return PT_OK;
}

int pt_raster_pass_share(uint32_t pass, uint32_t src_pass) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Pass *p = pass_of(pass), *s = pass_of(src_pass);
  if (!p || !s) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_RASTER || g.programs[s->program] != PK_RASTER)
    return err(PT_ERR_ARG, "pt_raster_pass_share: both passes must be rasterize passes");
  if (pass == src_pass || s->raster_src) return err(PT_ERR_ARG, "pt_raster_pass_share: share from an own-bound pass");
  p->raster_src = src_pass;
  p->bound = true;
  raster_touch(p);
  p->gcache.valid = false;  // another pass's triangles: the next draw draws
  return PT_OK;
}

int pt_raster_pass_adopt(uint32_t pass, int y_begin, int y_end) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (g.programs[p->program] != PK_RASTER) return err(PT_ERR_ARG, "pt_raster_pass_adopt: not a rasterize pass");
  if (p->att.size() < 4) return err(PT_ERR_STATE, "pt_raster_pass_adopt: the pass has no G-buffer attachments");
  GBufParams k;
  memset(&k, 0, sizeof(k));
  k.W = p->W;
  k.H = p->H;
  if (y_begin < 0 || y_end > p->H || y_begin > y_end) return err(PT_ERR_ARG, "pt_raster_pass_adopt: bad rows");
  raster_touch(p);  // the attachments hold texels no draw of this pass wrote (att_plane below clears their stamps)
  p->gcache.valid = false;
  k.y0 = y_begin;
  k.y1 = y_end;
  for (int i = 0; i < 4; ++i) {  // the attachments now hold new texels (their versions move on, as after a draw)
    Plane* dst[4] = {&k.world, &k.normal_depth, &k.motion, &k.fwidth};
    TRY(att_plane(p, i, dst[i]));
  }
  Texture* fwt = tex_of(p->att[3]);
  for (int i : {1, 3}) {
    const Texture* t = tex_of(p->att[i]);
    if (y_begin < t->row0 || y_end > t->row0 + t->rows)
      return err(PT_ERR_ARG, "pt_raster_pass_adopt: rows outside the attachments' stored rows");
  }
  if (!fwt->aux) {  // rows no draw has reached read 0 (pt_texture_readback_aux returns the whole plane)
    const size_t n = (size_t)fwt->W * fwt->rows;
    HIPCHK(hipMalloc((void**)&fwt->aux, n * 4));
    HIPCHK(hipMemsetAsync(fwt->aux, 0, n * 4, g.stream));
  }
  k.fwidth_aux = fwt->aux;
  TRY(gbuf_flags(p, fwt, k));
  const int rc = ptk::launch_gbuffer_adopt(k, g.stream);
  if (rc) return hip_err((hipError_t)rc, "pt_raster_pass_adopt");
  fwt->aux_valid = true;
  return PT_OK;
}

int pt_tiles_count(int frame_w, int tile_y0, int stride, int offset, int y_begin, int y_end, int64_t* out_pixels) {
  if (!out_pixels || frame_w <= 0 || frame_w % 16 || stride < 1 || offset < 0 || offset >= stride || y_begin > y_end ||
      y_begin < tile_y0)
    return err(PT_ERR_ARG, "pt_tiles_count: width a multiple of 16, 0 <= offset < stride, tile_y0 <= y_begin <= y_end");
  *out_pixels = ptk::shard_pixels(frame_w, tile_y0, stride, offset, y_begin, y_end);
  return PT_OK;
}

int pt_tiles_copy(const uint32_t* tex, int ntex, int tile_y0, int stride, const PtTileSeg* segs, int nseg, int unpack) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!tex || ntex < 1 || ntex > 4 || (nseg > 0 && !segs) || nseg < 0 || stride < 1)
    return err(PT_ERR_ARG, "pt_tiles_copy: 1..4 textures, segments, stride >= 1");
  ptk::ShardCopy c;
  memset(&c, 0, sizeof(c));
  c.tile_y0 = tile_y0;
  c.stride = stride;
  c.nplanes = ntex;
  c.unpack = unpack ? 1 : 0;
  Texture* ts[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int j = 0; j < ntex; ++j) {
    Texture* t = tex_of(tex[j]);
    if (!t || t->target != PT_TEXTURE_2D || !t->dev) return err(PT_ERR_INVALID_HANDLE, "pt_tiles_copy: invalid texture");
    if (j > 0 && t->W != ts[0]->W) return err(PT_ERR_ARG, "pt_tiles_copy: textures of different widths");
    if (t->W % 16) return err(PT_ERR_ARG, "pt_tiles_copy: the frame width must be a multiple of 16");
    ts[j] = t;
    c.plane[j] = (float4*)t->dev;
    c.row0[j] = t->row0;
  }
  c.W = ts[0]->W;
  for (int s = 0; s < nseg; ++s) {
    const PtTileSeg& q = segs[s];
    if (q.offset < 0 || q.offset >= stride || q.y_begin < tile_y0 || q.y_begin > q.y_end || (!q.packed && q.y_end > q.y_begin))
      return err(PT_ERR_ARG, "pt_tiles_copy: bad segment");
    for (int j = 0; j < ntex; ++j)
      if (q.y_end > q.y_begin && (q.y_begin < ts[j]->row0 || q.y_end > ts[j]->row0 + ts[j]->rows))
        return err(PT_ERR_ARG, "pt_tiles_copy: segment rows outside a texture's stored rows");
  }
  for (int s0 = 0; s0 < nseg; s0 += ptk::kShardSegs) {  // one launch per kShardSegs segments
    c.nseg = std::min(ptk::kShardSegs, nseg - s0);
    for (int s = 0; s < c.nseg; ++s) {
      const PtTileSeg& q = segs[s0 + s];
      c.seg[s] = ptk::ShardSeg{q.y_begin, q.y_end, q.offset, (float4*)q.packed};
    }
    const int rc = ptk::launch_shard_copy(c, g.stream);
    if (rc) return hip_err((hipError_t)rc, "pt_tiles_copy");
  }
  if (unpack)
    for (int j = 0; j < ntex; ++j) {  // new texels, as after a draw
      ts[j]->version++;
      ts[j]->raster_stamp = 0;
      ts[j]->bg = ptk::bg_fresh(&g.bg_serial);
      ts[j]->bg_prim = ts[j]->bg_gbuf = 0;
      ts[j]->bg_pass = nullptr;
      ts[j]->bg_off = 0;
    }
  return PT_OK;
}

int pt_pass_reset_texture_slot(uint32_t pass) {
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  p->slot = 0;
  return PT_OK;
}

int pt_pass_set_texture(uint32_t pass, uint32_t target, uint32_t tex, const char* name) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  Texture* t = tex_of(tex);
  if (!t) return err(PT_ERR_INVALID_HANDLE, "invalid texture");
  if (!name) return err(PT_ERR_ARG, "null sampler name");
  if (target != t->target) return err(PT_ERR_FORMAT, "texture bound to the wrong target");
  if (p->slot == 0) g.unit0 = tex;  // glActiveTexture(GL_TEXTURE0 + slot) is global state
  p->slot++;
  p->tex[name] = tex;
  return PT_OK;
}

int pt_pass_set_uniform_mat4(uint32_t pass, const char* name, const float* m) {
  int rc;
  Uniform* u = set_u(pass, name, 6, &rc);
  if (!u) return rc;
  if (!m) return err(PT_ERR_ARG, "null matrix");
  memcpy(u->f, m, 64);
  return PT_OK;
}
int pt_pass_set_uniform_float(uint32_t pass, const char* name, float v) {
  int rc;
  Uniform* u = set_u(pass, name, 1, &rc);
  if (!u) return rc;
  u->f[0] = v;
  return PT_OK;
}
int pt_pass_set_uniform_int(uint32_t pass, const char* name, int v) {
  int rc;
  Uniform* u = set_u(pass, name, 2, &rc);
  if (!u) return rc;
  u->i = v;
  return PT_OK;
}
int pt_pass_set_uniform_uint(uint32_t pass, const char* name, uint32_t v) {
  int rc;
  Uniform* u = set_u(pass, name, 3, &rc);
  if (!u) return rc;
  u->u = v;
  return PT_OK;
}
int pt_pass_set_uniform_bool(uint32_t pass, const char* name, int v) {
  int rc;
  Uniform* u = set_u(pass, name, 4, &rc);
  if (!u) return rc;
  u->i = v != 0;
  return PT_OK;
}
int pt_pass_set_uniform_vec3(uint32_t pass, const char* name, const float* v) {
  int rc;
  Uniform* u = set_u(pass, name, 5, &rc);
  if (!u) return rc;
  if (!v) return err(PT_ERR_ARG, "null vector");
  memcpy(u->f, v, 12);
  return PT_OK;
}

int pt_pass_set_rows(uint32_t pass, int y0, int y1) {
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (y0 < 0 && y1 < 0) { p->y_begin = p->y_end = -1; return PT_OK; }
  if (y0 < 0 || y1 > p->H || y0 > y1) return err(PT_ERR_ARG, "pt_pass_set_rows: bad range");
  p->y_begin = y0;
  p->y_end = y1;
  return PT_OK;
}

int pt_pass_set_row_cost(uint32_t pass, void* device_counts) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  p->row_cost = (uint32_t*)device_counts;
  return PT_OK;
}

int pt_pass_set_sample_counts(uint32_t pass, void* device_u8) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (device_u8 && g.programs[p->program] != PK_PATHTRACE) return err(PT_ERR_ARG, "sample counts need a path-tracing pass");
  p->sample_counts = (uint8_t*)device_u8;
  return PT_OK;
}

int pt_pass_set_sample_stats(uint32_t pass, void* device_f32x2) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (device_f32x2 && g.programs[p->program] != PK_PATHTRACE)
    return err(PT_ERR_ARG, "sample statistics need a path-tracing pass");
  p->sample_stats = (float2*)device_f32x2;
  return PT_OK;
}

int pt_pass_set_sample_moments(uint32_t pass, void* device_f32x4) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (device_f32x4 && g.programs[p->program] != PK_PATHTRACE)
    return err(PT_ERR_ARG, "sample moments need a path-tracing pass");
  p->sample_moments = (float4*)device_f32x4;
  return PT_OK;
}

int pt_sample_counts_derive(const void* stats, uint32_t motion_tex, uint32_t nd_tex, float lag, float tolerance,
                            int nmax, void* out_u8) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!stats || !out_u8) return err(PT_ERR_ARG, "pt_sample_counts_derive: null plane");
  if (!(tolerance > 0.0f)) return err(PT_ERR_ARG, "pt_sample_counts_derive: the tolerance must be > 0");
  if (nmax < 2 || nmax > kMaxBatch) return err(PT_ERR_ARG, "pt_sample_counts_derive: nmax must lie in 2 .. 8");
  Texture *mt, *nt;
  TRY(sample_count_planes("pt_sample_counts_derive", motion_tex, nd_tex, &mt, &nt));
  ptk::SppCountsParams c{};
  c.stats = (const float2*)stats;
  c.motion = (const float4*)mt->dev;
  c.nd = (const float4*)nt->dev;
  c.out = (uint8_t*)out_u8;
  c.W = mt->W;
  c.H = mt->H;
  c.nmax = nmax;
  c.lag = lag;
  c.tol = tolerance;
  const int rc = launch_spp_counts(c, g.stream);
  return rc ? hip_err((hipError_t)rc, "sample counts launch") : PT_OK;
}

int pt_sample_counts_pool(const void* stats, const void* counts_prev, int nmax_prev, const void* pool_in,
                          uint32_t motion_tex, uint32_t nd_tex, float lag, float wmax, float zeta, int rule,
                          float tolerance, int nmax, void* pool_out, void* out_u8) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!pool_out || !out_u8) return err(PT_ERR_ARG, "pt_sample_counts_pool: null output plane");
  if (pool_out == pool_in) return err(PT_ERR_ARG, "pt_sample_counts_pool: pool_out must not be pool_in");
  if (out_u8 == counts_prev) return err(PT_ERR_ARG, "pt_sample_counts_pool: out_u8 must not be counts_prev");
  if (!(tolerance > 0.0f)) return err(PT_ERR_ARG, "pt_sample_counts_pool: the tolerance must be > 0");
  if (!(zeta > 0.0f)) return err(PT_ERR_ARG, "pt_sample_counts_pool: zeta must be > 0");
  if (!(wmax >= 2.0f)) return err(PT_ERR_ARG, "pt_sample_counts_pool: wmax must be >= 2");
  if (rule != 0 && rule != 1) return err(PT_ERR_ARG, "pt_sample_counts_pool: rule must be 0 (relative) or 1 (absolute)");
  if (nmax < 2 || nmax > kMaxBatch || nmax_prev < 2 || nmax_prev > kMaxBatch)
    return err(PT_ERR_ARG, "pt_sample_counts_pool: nmax and nmax_prev must lie in 2 .. 8");
  Texture *mt, *nt;
  TRY(sample_count_planes("pt_sample_counts_pool", motion_tex, nd_tex, &mt, &nt));
  ptk::SppPoolParams c{};
  c.stats = (const float2*)stats;
  c.counts_prev = (const uint8_t*)counts_prev;
  c.pool_in = (const float4*)pool_in;
  c.motion = (const float4*)mt->dev;
  c.nd = (const float4*)nt->dev;
  c.pool_out = (float4*)pool_out;
  c.out = (uint8_t*)out_u8;
  c.W = mt->W;
  c.H = mt->H;
  c.nmax = nmax;
  c.nmax_prev = nmax_prev;
  c.rule = rule;
  c.lag = lag;
  c.tol = tolerance;
  c.wmax = wmax;
  c.zeta = zeta;
  const int rc = launch_spp_pool(c, g.stream);
  return rc ? hip_err((hipError_t)rc, "sample counts pool launch") : PT_OK;
}

int pt_pass_set_trace_stats_n(uint32_t pass, void* device_u64, int count) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (device_u64 && g.programs[p->program] != PK_PATHTRACE) return err(PT_ERR_ARG, "trace stats need a path-tracing pass");
  if (device_u64 && count <= 0) return err(PT_ERR_ARG, "trace stats buffer of no counters");
  p->stats = (unsigned long long*)device_u64;
  p->stats_n = device_u64 ? std::min(count, (int)kStatCount) : 0;
  return PT_OK;
}

// the entry point as first published took a buffer of 12 counters: it still writes those 12 only
int pt_pass_set_trace_stats(uint32_t pass, void* device_u64) {
  return pt_pass_set_trace_stats_n(pass, device_u64, PT_TRACE_STATS_V1);
}

int pt_trace_stats_count(void) { return ptk::kStatCountV2; }
int pt_trace_stats_total(void) { return kStatCount; }

int pt_pass_set_motion_bound(uint32_t pass, void* device_u32) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (device_u32 && g.programs[p->program] != PK_RASTER) return err(PT_ERR_ARG, "motion bound needs a rasterize pass");
  p->motion_max = (uint32_t*)device_u32;
  return PT_OK;
}

int pt_pass_draw(uint32_t pass) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (!p->bound) return err(PT_ERR_STATE, "pass drawn before bindData");
  const int kind = g.programs[p->program];
  return timed_draw(p, [&] {
    return kind == PK_PATHTRACE ? draw_pathtrace(p) : kind == PK_RASTER ? draw_raster(p) : draw_svgf(p, kind);
  });
}

int pt_pass_draw_batch(const uint32_t* passes, int count) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!passes || count < 1 || count > kMaxBatch) return err(PT_ERR_ARG, "a batch holds 1 to 8 path-tracing passes");
  Pass* ps[kMaxBatch];
  for (int b = 0; b < count; ++b) {
    ps[b] = pass_of(passes[b]);
    if (!ps[b]) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
    if (!ps[b]->bound) return err(PT_ERR_STATE, "pass drawn before bindData");
    if (g.programs[ps[b]->program] != PK_PATHTRACE) return err(PT_ERR_ARG, "a batch holds path-tracing passes only");
    for (int c = 0; c < b; ++c)
      if (ps[c] == ps[b]) return err(PT_ERR_ARG, "a pass appears twice in a batch");
  }
  return timed_draw(ps[0], [&] { return draw_pathtrace_batch(ps, count); });  // timed as the first pass's draw
}

int pt_pass_last_ms(uint32_t pass, float* ms) {
  Pass* p = pass_of(pass);
  if (!p || !ms) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  if (!p->timed) return err(PT_ERR_STATE, "pass has no timed draw (pt_set_profiling(1))");
  HIPCHK(hipEventSynchronize(p->ev1));
  HIPCHK(hipEventElapsedTime(ms, p->ev0, p->ev1));
  return PT_OK;
}

int pt_pass_destroy(uint32_t pass) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  auto it = g.passes.find(pass);
  if (it == g.passes.end()) return err(PT_ERR_INVALID_HANDLE, "invalid pass");
  (void)hipStreamSynchronize(g.stream);
  free_pass(it->second.get());
  g.passes.erase(it);
  return PT_OK;
}

}  // extern "C"

// capi_rays.hip — ray queries (include/ptsvgf.h "ray queries", DESIGN.md "Ray queries"): pt_rays_closest,
// pt_rays_occluded, pt_rays_primary and the diagnostics of include/ptsvgf_debug_rays.h. The definition is
// tests/ray_query_ref.py's; the kernels are kernels_rays.hip's. The scene is the draws' (scene_of: decoded on first
// use, current after a rebuild, refit, pose or skin); a query touches no pass.
#include "../../include/ptsvgf_debug_rays.h"
#include "capi_state.h"
#include "rays_device.h"

using namespace ptapi;

namespace ptapi {

namespace {

constexpr long long kRaysMax = 1LL << 28;

// Spill columns of the queries over deep trees: grown before a launch that needs more, kept, freed by pt_shutdown.
struct RayState {
  int* spill = nullptr;
  size_t ints = 0;
  uint64_t allocs = 0;  // allocations of spill so far
  int variant = -1;     // pt_debug_rays_variant: -1 the default
  int last_kind = -1;   // the last launched query's stack: 0 small, 1 full, 2 deep
  int last_variant = -1;
} g_rays;

// lane refill: on incoherent rays it measured about twice one ray per lane, far beyond the spread of three
// alternating repetitions, and faster on primary rays too (tools/ray_query_prof.py, DESIGN.md "Ray queries")
constexpr int kRaysDefaultVariant = ptk::kRaysRefill;

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int check_list(const char* fn, const void* in, int64_t n, const void* out, bool out16) {
  if (n < 0 || n > kRaysMax) return err(PT_ERR_ARG, std::string(fn) + ": n must lie in [0, 2^28]");
  if (n > 0 && (!in || !out)) return err(PT_ERR_ARG, std::string(fn) + ": null pointer with n > 0");
  if (!aligned16(in) || (out16 && !aligned16(out)))
    return err(PT_ERR_ARG, std::string(fn) + ": ray and hit records must be 16-byte aligned");
  return PT_OK;
}

// The query over the scene of (tri_tex, node_tex) with every check done and the spill scratch in place; reads: the
// version of the shading records the launch reads, to be noted after it (none: the decode's own buffer).
int query_for(const char* fn, uint32_t tri_tex, uint32_t node_tex, const void* rays, int64_t n, ptk::RayQuery* q,
              DrawReads* reads) {
  Texture* tt = tex_of(tri_tex);
  Texture* nt = tex_of(node_tex);
  if (!tt || tt->target != PT_TEXTURE_BUFFER || !nt || nt->target != PT_TEXTURE_BUFFER)
    return err(PT_ERR_INVALID_HANDLE, std::string(fn) + ": tri_tex and node_tex must be texture buffers");
  *reads = DrawReads{};
  memset(q, 0, sizeof(*q));
  if (n == 0) return PT_OK;
  SceneGPU* sg = nullptr;
  TRY(scene_of(tt, tri_tex, nt, node_tex, &sg));
  q->rays = (const float4*)rays;
  q->n = n;
  ptk::SceneDev& sc = q->scene;
  sc.tri_geom = sg->geom;
  sc.tri_shade = (const float4*)sg->shade.sb.buf;
  // the records' build event: a device decode a draw queued on another stream (a query may run on the library's own),
  // or the pt_materials_update that wrote this version on its stream; such a version is read until noted
  if (sg->shade.edited()) TRY(read_shared(*reads, sg->shade.sb));
  else if (sg->shade.sb.built) HIPCHK(sg->shade.sb.wait_built(g.stream));
  sc.bvh = sg->bvh;
  sc.root_ref = sg->root_ref;
  sc.ntris = sg->ntris;
  q->stack_need = sg->stack_need;
  q->fine_limit = sg->fine_eye_limit;
  if (sg->bvh_any) {  // the trees closest_tree and shadow_tree select by default
    sc.bvh_any = sg->bvh_any;
    sc.root_any = sg->root_any;
    q->sah = 1;
    q->stack_need = std::max(q->stack_need, sg->need_any);
    if (sg->has4 && !sg->nan4 && sg->bvh4) {
      sc.bvh4 = sg->bvh4;
      sc.root4 = sg->root4;
      sc.root4c = sg->root4c;
      q->wide = 1;
    }
  }
  const int levels = q->stack_need - ptk::kSpillKS + 1;
  if (levels > 0) {
    const size_t cols = (size_t)ptk::ray_query_blocks(n) * 128, need = cols * (size_t)levels;
    if (g_rays.ints < need) {
      if (g_rays.spill) (void)hipFree(g_rays.spill);  // (waits for the queries in flight)
      g_rays.spill = nullptr;
      g_rays.ints = 0;
      HIPCHK(hipMalloc((void**)&g_rays.spill, need * sizeof(int)));
      g_rays.ints = need;
      g_rays.allocs++;
    }
    q->spill = g_rays.spill;
    q->spill_stride = cols;
  }
  return PT_OK;
}

int after_launch(const char* what, int rc, const ptk::RayQuery& q, const DrawReads& reads, int variant) {
  if (rc) return hip_err((hipError_t)rc, what);
  TRY(note_reads(reads));
  g_rays.last_kind = q.spill ? 2 : (q.stack_need <= ptk::kStackSmall ? 0 : 1);
  g_rays.last_variant = variant;
  return PT_OK;
}

int variant_now() { return g_rays.variant < 0 ? kRaysDefaultVariant : g_rays.variant; }

}  // namespace

void free_rays() {
  if (g_rays.spill) (void)hipFree(g_rays.spill);
  g_rays = RayState{};
}

}  // namespace ptapi

extern "C" {

int pt_rays_closest(uint32_t tri_tex, uint32_t node_tex, const void* device_rays, int64_t n, void* device_hits) {
  TRY(check_list("pt_rays_closest", device_rays, n, device_hits, true));
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  ptk::RayQuery q;
  DrawReads reads;
  TRY(query_for("pt_rays_closest", tri_tex, node_tex, device_rays, n, &q, &reads));
  if (n == 0) return PT_OK;
  const int v = variant_now();
  return after_launch("pt_rays_closest", ptk::launch_rays_closest(q, device_hits, v, g.stream), q, reads, v);
}

int pt_rays_occluded(uint32_t tri_tex, uint32_t node_tex, const void* device_rays, int64_t n, void* device_u8) {
  TRY(check_list("pt_rays_occluded", device_rays, n, device_u8, false));
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  ptk::RayQuery q;
  DrawReads reads;
  TRY(query_for("pt_rays_occluded", tri_tex, node_tex, device_rays, n, &q, &reads));
  if (n == 0) return PT_OK;
  const int v = variant_now();
  // (the verdict reads no shading record: nothing to note)
  return after_launch("pt_rays_occluded", ptk::launch_rays_occluded(q, device_u8, v, g.stream), q, DrawReads{}, v);
}

int pt_rays_primary(const float* eye3, const float* cameraRotate16, int width, int height, int aspect_corrected,
                    const int32_t* device_xy, int64_t n, void* device_rays_out) {
  if (!eye3 || !cameraRotate16) return err(PT_ERR_ARG, "pt_rays_primary: null eye3 or cameraRotate16");
  if (width < 1 || height < 1) return err(PT_ERR_ARG, "pt_rays_primary: width and height must be >= 1");
  if (n < 0 || n > kRaysMax) return err(PT_ERR_ARG, "pt_rays_primary: n must lie in [0, 2^28]");
  if (n > 0 && !device_rays_out) return err(PT_ERR_ARG, "pt_rays_primary: null device_rays_out with n > 0");
  if (!aligned16(device_rays_out) || ((uintptr_t)device_xy & 7u))
    return err(PT_ERR_ARG, "pt_rays_primary: ray records must be 16-byte aligned, pixel pairs 8-byte aligned");
  if (!device_xy && n != (int64_t)width * height)
    return err(PT_ERR_ARG, "pt_rays_primary: without device_xy n must be width * height");
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (n == 0) return PT_OK;
  ptk::PTParams p;
  memset(&p, 0, sizeof(p));
  p.W = width;
  p.H = height;
  p.aspect_corrected = aspect_corrected ? 1 : 0;
  memcpy(p.eye, eye3, sizeof(p.eye));
  memcpy(p.camRot, cameraRotate16, sizeof(p.camRot));
  const int rc = ptk::launch_rays_primary(p, device_xy, n, device_rays_out, g.stream);
  return rc ? hip_err((hipError_t)rc, "pt_rays_primary") : PT_OK;
}

// ------------------------------------------------------------ diagnostics (ptsvgf_debug_rays.h) ---
int pt_debug_rays_variant(int variant) {
  if (variant < -1 || variant > 1) return err(PT_ERR_ARG, "pt_debug_rays_variant: -1 (default), 0 or 1");
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  g_rays.variant = variant;
  return PT_OK;
}

int pt_debug_rays_state(int* stack_kind, int* variant, uint64_t* scratch_allocs, size_t* scratch_bytes) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (stack_kind) *stack_kind = g_rays.last_kind;
  if (variant) *variant = g_rays.last_variant;
  if (scratch_allocs) *scratch_allocs = g_rays.allocs;
  if (scratch_bytes) *scratch_bytes = g_rays.ints * sizeof(int);
  return PT_OK;
}

}  // extern "C"

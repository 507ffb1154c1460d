// capi.hip — implementation of include/ptsvgf.h: the GL-plumbing-shaped C ABI
// (Utils/render_pass.h:82-182, Utils/shader.h:21-67, Utils/help_func.h:22-32)
// over HIP device memory and the gfx950 kernels. The entry points of geometry that moves (builds, refits, raster binds,
// poses) are in capi_geometry.hip, those of lights that move in capi_lights.hip, and the static view's bookkeeping
// (keys, caches, quiet-tile sets; the draws here call into it) in capi_static.hip; capi_state.h holds what they share.
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
#include "../../include/ptsvgf_debug_background.h"
#include "../../include/ptsvgf_scene.h"
#include "capi_state.h"
#include "glsl_builtins.h"
#include "host_trees.h"
#include "pb_overlap.h"
#include "spp_params.h"

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

}  // namespace ptapi

using namespace ptapi;

namespace {

using namespace ptk;

std::string basename_of(const char* p) {
  std::string s(p ? p : "");
  size_t k = s.find_last_of("/\\");
  return k == std::string::npos ? s : s.substr(k + 1);
}

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
  WFState s0{};
  float4** f4p[10] = {&s0.ray_o, &s0.ray_d, &s0.light, &s0.red, &s0.pend0,
                      &s0.pend1, &s0.pend2, &s0.pend3, &s0.sh_h, &s0.sh_p};
  for (auto q : f4p) { *q = (float4*)c; c += up(f4); }
  s0.hit = (int2*)c; c += up(m * 8);
  s0.hit0 = (int2*)c; c += up(m * 8);
  s0.pcache = (uint16_t*)c; c += up(m * 2);
  s0.seed = (uint32_t*)c; c += up(m * 4);
  s0.occ_h = (uint8_t*)c; c += up(m);
  s0.occ_p = (uint8_t*)c; c += up(m);
  s0.straggler = (int*)c; c += up(m * 8);  // both shadow kinds of one bounce (a batch's: frame 0's pointer)
  s0.strag_c = (int*)c; c += up(m * 4);    // bounce rays of one bounce
  int* counters = (int*)c; c += up((size_t)nb * kWfCounters * 4);  // contiguous: one memset per draw
  for (int f = 0; f < nb; ++f) {
    WFState st = s0;
    const size_t o = (size_t)f * n;
    st.ray_o = s0.ray_o + o;
    st.ray_d = s0.ray_d + o;
    st.light = s0.light + o;
    st.red = s0.red + o;
    st.pend0 = s0.pend0 + o;
    st.pend1 = s0.pend1 + o;
    st.pend2 = s0.pend2 + o;
    st.pend3 = s0.pend3 + o;
    st.sh_h = s0.sh_h + o;
    st.sh_p = s0.sh_p + o;
    st.hit = s0.hit + o;
    st.hit0 = s0.hit0 + o;
    st.pcache = s0.pcache + o;
    st.seed = s0.seed + o;
    st.occ_h = s0.occ_h + o;
    st.occ_p = s0.occ_p + o;
    st.straggler = s0.straggler + 2 * o;
    st.strag_c = s0.strag_c + o;
    st.counters = counters + (size_t)f * kWfCounters;
    st.list0 = (int*)c; c += up(nl * 4 * kLiveBins);
    st.list1 = (int*)c; c += up(nl * 4 * kLiveBins);
    st.shadow_list = (int*)c; c += up(nl * 4 * (1 + kPointBins));
    b.stb[f] = st;
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
// drops a scene's point-light bins (the caller has synchronised the streams that read them)
void free_point_bins(PointBinsGPU& m) {
  m.sb.free();
  m = PointBinsGPU{};
}

// drops a merged environment: its buffers (the caller has synchronised the streams that read them) and events
void free_hdr_merged(HdrMerged& m) {
  m.sb.free();
  m = HdrMerged{};
}

constexpr int kLbvhWideDefault = 1;  // pass uniform lbvh_wide (pt_params)
// pass uniform primary_raster (pt_wf_setup): 2 = triangles binned to tiles (wf_primary_tri), 1 = reference leaves
constexpr int kPrimaryRasterDefault = 2;

// the trees a GPU-built scene borrowed from its node texture are that texture's to free (free_trees)
void drop_borrowed(SceneGPU& sg) {
  if (!sg.lbvh) return;
  sg.bvh = sg.bvh4 = sg.bvh_any = sg.leaves = nullptr;
  sg.lbvh = false;
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
  HIPCHK(hipMalloc(&sg.shade.buf, shade_bytes));
  sg.shade.bytes = shade_bytes;
  TRY(materials_order(g.stream));  // the texels as every pt_materials_update so far left them
  HIPCHK((hipError_t)ptk::decode_tris((const float*)tris->dev, (int)ntris, sg.geom, (float4*)sg.shade.buf, g.stream));
  HIPCHK(sg.shade.mark_built(g.stream));  // for a pt_materials_update that follows: draws do not wait for it
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
    sg.shade.buf = sh;
    sg.shade.bytes = shade.size() * sizeof(float4);
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

int plane_of(Texture* t, Pass* p, Plane* out, const char* what) {
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
int att_plane(Pass* p, int k, Plane* out) {
  if ((int)p->att.size() <= k) return err(PT_ERR_ARG, "pass has too few color attachments");
  Texture* t = tex_of(p->att[k]);
  int rc = plane_of(t, p, out, "color attachment");
  if (rc != PT_OK) return rc;
  tex_written(t);  // (a draw into it by any pass)
  return PT_OK;
}

// sobol (path_tracing.frag:480-495): a per-frame uniform value
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
  HIPCHK(m.sb.wait_built(g.stream));
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
  reads.pbins = &m.sb;
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
  k.scene.tri_shade = (const float4*)sg->shade.buf;
  if (sg->shade_first) {  // pt_materials_update wrote it, on another stream; this version is read until noted
    HIPCHK(sg->shade.wait_built(g.stream));
    reads.shade = &sg->shade;
  }
  k.scene.bvh = sg->bvh;
  k.scene.root_ref = sg->root_ref;
  k.stack_need = sg->stack_need;
  const Uniform* e = U(p, "eye", 5);
  if (e) memcpy(k.eye, e->f, 12);
  // the any-hit / closest-hit SAH trees hold fine boxes padded for eyes within sg->fine_eye_limit (refine_leaves): an
  // eye further out walks the reference tree, whose boxes are the reference's own
  const bool eye_near = fabsf(k.eye[0]) <= sg->fine_eye_limit && fabsf(k.eye[1]) <= sg->fine_eye_limit &&
                        fabsf(k.eye[2]) <= sg->fine_eye_limit;
  // lbvh_wide (default kLbvhWideDefault): a scene pt_bvh_build wrote is walked through the 4-wide tree its device stage
  // derived (same bits; DESIGN.md "Dynamic scenes"); 0 = its binary tree alone, as before that stage existed. Its
  // any-hit tree is that same binary tree, so it is bound only for the 4-wide walk.
  const bool wide_on = sg->has4 && !(PT_WIDE_SIGNED && sg->nan4) && ui(p, "wide_bvh", 1) &&
                       (!sg->lbvh || ui(p, "lbvh_wide", kLbvhWideDefault));
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
      HIPCHK(lt->lights->sb.wait_built(g.stream));
      reads.lights = &lt->lights->sb;
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
  // A/B switch hdr_merge (default 1): the NEE's radiance and pdf fetches at one direction from one merged texture
  if (ui(p, "hdr_merge", 1) && hm != hc && hm->W == hc->W && hm->H == hc->H && hm->target == PT_TEXTURE_2D &&
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
    HIPCHK(m.sb.wait_built(g.stream));
    reads.hdr = &m.sb;
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
    k.wf.shadow_budget = (uint32_t)ui(p, "shadow_budget", 0);
    // > 0: bounce rays past this many visits finish in the wave-cooperative closest-hit walk (refill kernel only)
    k.wf.closest_budget = (uint32_t)ui(p, "closest_budget", 0);
    // percent of the bounce / shadow lists traced by lane-refill waves: 75 pays with frames in flight (the renderer
    // sets it then), 0 (default) keeps the shortest single-frame latency
    k.refill = std::min(100, std::max(0, ui(p, "trace_refill", 0)));
    k.refill_waves = std::max(0, ui(p, "refill_waves", 0));
    k.refill_grid = std::max(0, ui(p, "refill_grid", 0));
    k.list_grid = std::max(0, ui(p, "list_grid", 0));
    // 1: paths end in place (no wf_finalize, no wf_finish between two shades); 0 keeps those launches (A/B, tests)
    k.shade_fold = ui(p, "shade_fold", 1) != 0;
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
  if (!ui(p, "trace_fork", 0)) return nullptr;
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

// after a path-tracing draw's launch: its stream's use events on the shared buffers it read (SharedBuf::note_read)
int note_reads(const DrawReads& r) {
  if (r.pbins) HIPCHK(r.pbins->note_read(g.stream));
  if (r.hdr) HIPCHK(r.hdr->note_read(g.stream));
  if (r.lights) HIPCHK(r.lights->note_read(g.stream));
  if (r.shade) HIPCHK(r.shade->note_read(g.stream));
  return PT_OK;
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
    // compared at its effective value (the default pt_params / pt_wf_setup apply when a pass never set it)
    struct Same { const char* name; int dflt; };
    const Same same[] = {{"trace_refill", 0}, {"shadow_budget", 0}, {"closest_budget", 0}, {"wide_bvh", 1}, {"lbvh_wide", kLbvhWideDefault},
                         {"refill_waves", 0}, {"trace_fork", 0}, {"refill_grid", 0}, {"list_grid", 0},
                         {"shade_fold", 1}};
    bool agree = true;
    for (const Same& u : same) agree = agree && ui(ps[b], u.name, u.dflt) == ui(ps[0], u.name, u.dflt);
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

// The tile flags of a draw of p over rows [k.y0, k.y1): the rows the a-trous passes draw ("atrous_rows_begin" /
// "_end", e.g. a band's ghost-zone margin), default the G-buffer's own rows; they must lie inside them (a tile's flag is
// marked by the G-buffer pixels it holds). Allocates and zeroes them on the fwidth texture; k.tflags null when off.
static int gbuf_flags(Pass* p, Texture* fwt, GBufParams& k) {
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
  if (!fwt->aux) {  // rows no draw has reached read 0 (pt_texture_readback_aux returns the whole plane)
    const size_t n = (size_t)fwt->W * fwt->rows;
    HIPCHK(hipMalloc((void**)&fwt->aux, n * 4));
    HIPCHK(hipMemsetAsync(fwt->aux, 0, n * 4, g.stream));
  }
  k.fwidth_aux = fwt->aux;
  // the a-trous per-tile surface flags of this G-buffer, marked by the G-buffer kernels as they write the pixels
  TRY(gbuf_flags(p, fwt, k));
  // vec3 uniform bound_eye (the origin of this frame's primary rays): the draw also writes the primary rasterisers'
  // pruning bound of every pixel into the world attachment's compact plane, 4 bytes instead of their 32 of texels
  Texture* wt = tex_of(p->att[0]);
  const Uniform* be = U(p, "bound_eye", 5);
  if (be) {
    if (!wt->aux) {  // rows no draw has reached hold "no bound"
      const size_t n = (size_t)wt->W * wt->rows;
      HIPCHK(hipMalloc((void**)&wt->aux, n * 4));
      HIPCHK(hipMemsetD32Async((hipDeviceptr_t)wt->aux, 0x7f800000, n, g.stream));
    }
    k.bound_aux = wt->aux;
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

int draw_svgf(Pass* p, int kind) {
  int y0, y1;
  rows_of(p, &y0, &y1);
  int rc = 0;
  BgDraw bg;
  if (kind == PK_REPROJECT || kind == PK_VARIANCE || kind == PK_ATROUS) bg.reason = bg_bypass(p, y0, y1);
  if (kind == PK_REPROJECT) {
    ReprojParams k;
    memset(&k, 0, sizeof(k));
    k.W = p->W; k.H = p->H; k.y0 = y0; k.y1 = y1;
    TRY(plane_of(sampler(p, "gMotion"), p, &k.motion, "gMotion"));
    TRY(plane_of(sampler(p, "gColor"), p, &k.color, "gColor"));
    TRY(plane_of(sampler(p, "gAlbedo"), p, &k.albedo, "gAlbedo"));
    TRY(plane_of(sampler(p, "gEmission"), p, &k.emission, "gEmission"));
    TRY(plane_of(sampler(p, "gPrevIllum"), p, &k.prev_illum, "gPrevIllum"));
    TRY(plane_of(sampler(p, "gPrevMoments_HistoryLength"), p, &k.prev_moments, "gPrevMoments_HistoryLength"));
    TRY(plane_of(sampler(p, "gNormalAndLinearZ"), p, &k.nd, "gNormalAndLinearZ"));
    TRY(plane_of(sampler(p, "gPrevNormalAndLinearZ"), p, &k.prev_nd, "gPrevNormalAndLinearZ"));
    TRY(plane_of(sampler(p, "gNormalDepthFwidth"), p, &k.fwidth, "gNormalDepthFwidth"));
    if (p->att.size() >= 2) {  // (the stamps as the draw finds them: att_plane makes the outputs' fresh)
      bg.pair(sampler(p, "gColor"), tex_of(p->att[0]), false);
      bg.pair(sampler(p, "gPrevMoments_HistoryLength"), tex_of(p->att[1]), false);
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
    {
      const Texture *ct = sampler(p, "gColor"), *ft = sampler(p, "gNormalDepthFwidth");
      bg.need(!k.sm.p, PT_BG_R_SAMPLE_MOMENTS);
      bg.need(bg_whole(ct, p->H) && bg_whole(ft, p->H) && bg_whole(bg.out[0], p->H) && bg_whole(bg.out[1], p->H) &&
                  bg_whole(sampler(p, "gPrevMoments_HistoryLength"), p->H),
              PT_BG_R_ROWS);
      bg.need(bg_one_gbuffer(sampler(p, "gNormalAndLinearZ"), ft), PT_BG_R_NO_PLANE);
      bg.need(ct->bg_prim && ft->bg_gbuf, PT_BG_R_NO_CONTENT);
      bool build = false;
      // (a pass with the switch off takes no part: it leaves the choice to the passes that have it on)
      if (bg.reason != PT_BG_R_UNIFORM && bg.reason != PT_BG_R_ENV)
        bg.set = ptk::quiet_set_for(g.bg_choice, bg.reason ? 0 : ct->bg_prim, bg.reason ? 0 : ft->bg_gbuf,
                                    &g.bg_serial, &build);
      if (build) {
        bool built = false;
        TRY(bg_build_set(bg.set, ct, ft, k.W, k.H, &built));
        if (!built) {  // (no primary plane to read: PT_BG_R_NO_PLANE, and the next draw tries again)
          g.bg_choice.set = bg.set = 0;
          bg.reason = PT_BG_R_NO_PLANE;
        }
      }
      bg.in_off = 0;  // (the head of the chain: what bypassed the last frame's draws does not bind this one)
      bg.decide();
      if (bg.skip) k.busy16 = bg.qs->flags + bg.qs->off16;
    }
    rc = launch_reproject(k, g.stream);
    bg.finish(p, 5, rc == 0);
  } else if (kind == PK_VARIANCE) {
    VarianceParams k;
    memset(&k, 0, sizeof(k));
    k.W = p->W; k.H = p->H; k.y0 = y0; k.y1 = y1;
    TRY(plane_of(sampler(p, "gIllumination"), p, &k.illum, "gIllumination"));
    TRY(plane_of(sampler(p, "gMoments_HistoryLength"), p, &k.moments, "gMoments_HistoryLength"));
    TRY(plane_of(sampler(p, "gNormalAndLinearZ"), p, &k.nd, "gNormalAndLinearZ"));
    TRY(plane_of(sampler(p, "gNormalDepthFwidth"), p, &k.fwidth, "gNormalDepthFwidth"));
    if (!p->att.empty()) bg.pair(sampler(p, "gIllumination"), tex_of(p->att[0]), false);
    TRY(att_plane(p, 0, &k.out));
    k.phi_color = uf(p, "gPhiColor", 0.0f);
    k.phi_normal = uf(p, "gPhiNormal", 0.0f);
    if (Texture* sm = bound_sampler(p, "gSampleMoments")) TRY(plane_of(sm, p, &k.sm, "gSampleMoments"));
    {
      const Texture *it = sampler(p, "gIllumination"), *ft = sampler(p, "gNormalDepthFwidth");
      bg.need(!k.sm.p, PT_BG_R_SAMPLE_MOMENTS);
      bg.need(bg_whole(it, p->H) && bg_whole(ft, p->H) && bg_whole(bg.out[0], p->H), PT_BG_R_ROWS);
      bg.need(bg_one_gbuffer(sampler(p, "gNormalAndLinearZ"), ft), PT_BG_R_NO_PLANE);
      if (!bg.reason) bg.set = bg_set_from_input(it, ft, k.W, k.H);
      bg.decide();
      if (bg.skip) k.busy16 = bg.qs->flags + bg.qs->off16;
    }
    rc = launch_variance(k, g.stream);
    bg.finish(p, 5, rc == 0);
  } else if (kind == PK_ATROUS) {
    AtrousParams k;
    memset(&k, 0, sizeof(k));
    k.W = p->W; k.H = p->H; k.y0 = y0; k.y1 = y1;
    TRY(plane_of(sampler(p, "gIllumination"), p, &k.illum, "gIllumination"));
    TRY(plane_of(sampler(p, "gNormalAndLinearZ"), p, &k.nd, "gNormalAndLinearZ"));
    TRY(plane_of(sampler(p, "gNormalDepthFwidth"), p, &k.fwidth, "gNormalDepthFwidth"));
    if (!p->att.empty()) bg.pair(sampler(p, "gIllumination"), tex_of(p->att[0]), false);
    if (ui(p, "fuse_modulate", 0) && p->att.size() >= 2) bg.pair(sampler(p, "gIllumination"), tex_of(p->att[1]), true);
    TRY(att_plane(p, 0, &k.out));
    if (k.out.p == k.illum.p) return err(PT_ERR_ARG, "a-trous output aliases its input (GL feedback loop)");
    k.step = ui(p, "gStepSize", 1);
    k.phi_color = uf(p, "gPhiColor", 0.0f);
    k.phi_normal = uf(p, "gPhiNormal", 0.0f);
    // production tiled kernel: per-tile surface flags, derived once per G-buffer from its depth-fwidth plane
    const int si = k.step == 1 ? 0 : k.step == 2 ? 1 : k.step == 4 ? 2 : k.step == 8 ? 3 : k.step == 16 ? 4 : -1;
    const int av = ui(p, "atrous_variant", 0);
    if (!ui(p, "exact", 0) && av == 0 && ui(p, "atrous_tile_flags", 1) && k.fwidth.aux &&
        si >= 0 && y1 > y0) {
      Texture* ft = sampler(p, "gNormalDepthFwidth");
      const size_t nb = ptk::atrous_flag_bytes(k.W, y0, y1);
      if (ft->tflags_cap < nb) {
        if (ft->tflags) (void)hipFree(ft->tflags);
        ft->tflags = nullptr;
        ft->tflags_cap = 0;
        HIPCHK(hipMalloc((void**)&ft->tflags, nb));
        ft->tflags_cap = nb;
        ft->tflags_ver = 0;
      }
      if (ft->tflags_ver != ft->version || ft->tflags_y0 != y0 || ft->tflags_y1 != y1) {
        const int frc = ptk::atrous_tile_flags(k.fwidth, k.W, y0, y1, ft->tflags, g.stream);
        if (frc) return hip_err((hipError_t)frc, "a-trous tile flags");
        ft->tflags_ver = ft->version;
        ft->tflags_y0 = y0;
        ft->tflags_y1 = y1;
      }
      k.tile_any = ft->tflags + ptk::atrous_flag_offset(si, k.W, y0, y1);
    }
    // fused modulate (fast driver, last iteration): "fuse_modulate" = 1, colour attachment 1 = the modulate target,
    // gAlbedo / gEmission bound; the production kernel writes it from its epilogue, the others launch modulate after
    if (ui(p, "fuse_modulate", 0)) {
      TRY(plane_of(sampler(p, "gAlbedo"), p, &k.albedo, "gAlbedo"));
      TRY(plane_of(sampler(p, "gEmission"), p, &k.emission, "gEmission"));
      TRY(att_plane(p, 1, &k.mod));
      const Plane* mp[3] = {&k.albedo, &k.emission, &k.mod};
      for (const Plane* q : mp)
        if (y0 < std::max(0, q->row0) || y1 > std::min(p->H, q->row0 + q->rows))
          return err(PT_ERR_ARG, "fused modulate: a plane does not store the draw's rows");
      if (k.mod.p == k.illum.p || k.mod.p == k.out.p) return err(PT_ERR_ARG, "fused modulate target aliases the a-trous planes");
    }
    {
      // static background: only the tiled kernel with this draw's own tile flags skips (k.tile_any set: the
      // production variant, a step of 1 .. 16, the compact plane), and only over whole-frame planes, which is also what
      // makes launch_atrous_fast choose it (same_geometry)
      const Texture *it = sampler(p, "gIllumination"), *ft = sampler(p, "gNormalDepthFwidth");
      bg.need(bg_whole(it, p->H) && bg_whole(ft, p->H) && bg_whole(bg.out[0], p->H) &&
                  (bg.npairs < 2 || bg_whole(bg.out[1], p->H)) && bg_whole(sampler(p, "gNormalAndLinearZ"), p->H),
              PT_BG_R_ROWS);
      bg.need(k.fwidth.aux, PT_BG_R_NO_PLANE);
      bg.need(k.tile_any, PT_BG_R_KERNEL);
      bg.need(bg_one_gbuffer(sampler(p, "gNormalAndLinearZ"), ft), PT_BG_R_NO_PLANE);
      if (!bg.reason) bg.set = bg_set_from_input(it, ft, k.W, k.H);
      bg.decide();
      if (bg.skip) k.busy = bg.qs->flags + ptk::atrous_flag_offset(si, k.W, 0, k.H);
    }
    if (ui(p, "exact", 0)) rc = launch_atrous_exact(k, g.stream);          // bit-exact form (tests)
    else if (ui(p, "atrous_variant", 0) == 1) rc = launch_atrous_simple(k, g.stream);  // A/B: generic
    else if (ui(p, "atrous_variant", 0) == 2) rc = launch_atrous_step(k, g.stream);    // A/B: step kernel
    else rc = launch_atrous_fast(k, g.stream);                             // LDS-tiled (production)
    if (rc == PT_OK && k.mod.p && (ui(p, "exact", 0) || ui(p, "atrous_variant", 0) != 0))
      rc = launch_modulate_after(k, g.stream);
    bg.finish(p, si < 0 ? 0 : si, rc == 0);
  } else if (kind == PK_MODULATE) {
    ModulateParams k;
    memset(&k, 0, sizeof(k));
    k.W = p->W; k.H = p->H; k.y0 = y0; k.y1 = y1;
    TRY(plane_of(sampler(p, "gAlbedo"), p, &k.albedo, "gAlbedo"));
    TRY(plane_of(sampler(p, "gEmission"), p, &k.emission, "gEmission"));
    TRY(plane_of(sampler(p, "gIllumination"), p, &k.illum, "gIllumination"));
    TRY(plane_of(sampler(p, "gNormalAndLinearZ"), p, &k.nd, "gNormalAndLinearZ"));
    TRY(att_plane(p, 0, &k.out));
    rc = launch_modulate(k, g.stream);
  } else if (kind == PK_OUTPUT) {
    OutputParams k;
    memset(&k, 0, sizeof(k));
    k.W = p->W; k.H = p->H; k.y0 = y0; k.y1 = y1;
    TRY(plane_of(sampler(p, "texPass0"), p, &k.in, "texPass0"));
    if (p->att.empty()) return PT_OK;  // default framebuffer: nothing to keep
    TRY(att_plane(p, 0, &k.out));
    rc = launch_output(k, g.stream);
  } else if (kind == PK_TAA) {
    TAAParams k;
    memset(&k, 0, sizeof(k));
    k.W = p->W; k.H = p->H; k.y0 = y0; k.y1 = y1;
    TRY(plane_of(sampler(p, "currentColor"), p, &k.cur, "currentColor"));
    TRY(plane_of(sampler(p, "previousColor"), p, &k.prev, "previousColor"));
    TRY(plane_of(sampler(p, "velocityTexture"), p, &k.vel, "velocityTexture"));
    TRY(plane_of(sampler(p, "normal_depth"), p, &k.nd, "normal_depth"));
    TRY(att_plane(p, 0, &k.out));
    k.frameCounter = uu(p, "frameCounter", 0);
    rc = launch_taa(k, g.stream);
  } else if (kind == PK_BLIT) {
    if (p->att.empty()) return err(PT_ERR_ARG, "bilt pass without attachment");
    TRY(copy_plane(tex_of(p->att[0]), sampler(p, "in_texture"), p, y0, y1));
  } else if (kind == PK_SAVE) {
    const char* names[5] = {"texPass0", "texPass1", "texPass2", "accColor", "taaOutput"};
    for (int i = 0; i < 5 && i < (int)p->att.size(); ++i)
      TRY(copy_plane(tex_of(p->att[i]), sampler(p, names[i]), p, y0, y1));
  }
  return rc ? hip_err((hipError_t)rc, "kernel launch") : PT_OK;
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
  for (auto& kv : g.textures) {
    Texture* t = kv.second.get();
    free_lights(t);
    if (t->owned && t->dev) (void)hipFree(t->dev);
    if (t->aux) (void)hipFree(t->aux);
    if (t->tflags) (void)hipFree(t->tflags);
    free_trees(t);
    free_refit(t);
  }
  for (auto& kv : g.passes) free_pass(kv.second.get());
  for (auto& kv : g.poses) free_pose(*kv.second);
  for (auto& kv : g.scenes) free_scene(kv.second);
  free_materials();
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
  // the stream's last reads of the merged environments and of the scenes' point-light bins: done before the entry goes
  for (auto& kv : g.hdr_merged) kv.second.sb.forget(st);
  for (auto& kv : g.scenes) {
    kv.second.pbins.sb.forget(st);
    kv.second.shade.forget(st);
  }
  for (auto& kv : g.textures)
    if (kv.second->lights) kv.second->lights->sb.forget(st);
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
  t->W = w;
  t->H = h;
  if (g.band_h > 0 && w == g.band_w && h == g.band_h) {
    t->row0 = g.band_row0;
    t->rows = g.band_rows;
  } else {
    t->row0 = 0;
    t->rows = h;
  }
  t->bytes = (size_t)w * t->rows * 16;
  HIPCHK(hipMalloc(&t->dev, t->bytes));
  HIPCHK(hipMemsetAsync(t->dev, 0, t->bytes, g.stream));  // GL leaves it undefined; the build zeroes
  return new_texture(std::move(t), out);
}

int pt_texture2d_wrap(void* ptr, int w, int h, uint32_t* out) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!ptr || w <= 0 || h <= 0 || !out) return err(PT_ERR_ARG, "pt_texture2d_wrap: bad argument");
  auto t = std::make_unique<Texture>();
  t->W = w;
  t->H = h;
  if (g.band_h > 0 && w == g.band_w && h == g.band_h) {
    t->row0 = g.band_row0;
    t->rows = g.band_rows;
  } else {
    t->rows = h;
  }
  t->bytes = (size_t)w * t->rows * 16;
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
  if (w != t->W || h != t->H) {  // glTexImage2D respecifies the image
    if (t->owned && t->dev) HIPCHK(hipFree(t->dev));
    if (!t->owned) return err(PT_ERR_ARG, "cannot resize a wrapped texture");
    if (t->aux) (void)hipFree(t->aux);  // sized for the old image
    t->aux = nullptr;
    t->W = w; t->H = h; t->row0 = 0; t->rows = h;
    if (g.band_h > 0 && w == g.band_w && h == g.band_h) { t->row0 = g.band_row0; t->rows = g.band_rows; }
    t->bytes = (size_t)w * t->rows * 16;
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
  free_lights(it->second.get());  // every version of an updated lights buffer (dev is one of them)
  if (it->second->owned && it->second->dev) (void)hipFree(it->second->dev);
  if (it->second->aux) (void)hipFree(it->second->aux);
  if (it->second->tflags) (void)hipFree(it->second->tflags);
  free_trees(it->second.get());  // the scenes that borrowed them are dropped below
  free_refit(it->second.get());
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
  Texture* mt = tex_of(motion_tex);
  Texture* nt = tex_of(nd_tex);
  if (!mt || !nt || mt->target != PT_TEXTURE_2D || nt->target != PT_TEXTURE_2D || !mt->dev || !nt->dev)
    return err(PT_ERR_MISSING_TEXTURE, "pt_sample_counts_derive needs the 2-D textures gMotion and gNormalAndLinearZ");
  if (mt->W != nt->W || mt->H != nt->H) return err(PT_ERR_ARG, "pt_sample_counts_derive: textures of different sizes");
  if (band_partition(mt->W, mt->H) || mt->row0 != 0 || nt->row0 != 0 || mt->rows != mt->H || nt->rows != nt->H)
    return err(PT_ERR_STATE, "pt_sample_counts_derive: not under a pt_set_band partition");
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
  Texture* mt = tex_of(motion_tex);
  Texture* nt = tex_of(nd_tex);
  if (!mt || !nt || mt->target != PT_TEXTURE_2D || nt->target != PT_TEXTURE_2D || !mt->dev || !nt->dev)
    return err(PT_ERR_MISSING_TEXTURE, "pt_sample_counts_pool needs the 2-D textures gMotion and gNormalAndLinearZ");
  if (mt->W != nt->W || mt->H != nt->H) return err(PT_ERR_ARG, "pt_sample_counts_pool: textures of different sizes");
  if (band_partition(mt->W, mt->H) || mt->row0 != 0 || nt->row0 != 0 || mt->rows != mt->H || nt->rows != nt->H)
    return err(PT_ERR_STATE, "pt_sample_counts_pool: not under a pt_set_band partition");
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
  int kind = g.programs[p->program];
  if (g.profiling) {
    if (!p->ev0) { HIPCHK(hipEventCreate(&p->ev0)); HIPCHK(hipEventCreate(&p->ev1)); }
    HIPCHK(hipEventRecord(p->ev0, g.stream));
  }
  int rc;
  if (kind == PK_PATHTRACE) rc = draw_pathtrace(p);
  else if (kind == PK_RASTER) rc = draw_raster(p);
  else rc = draw_svgf(p, kind);
  if (rc != PT_OK) return rc;
  if (g.profiling) {
    HIPCHK(hipEventRecord(p->ev1, g.stream));
    p->timed = true;
  }
  return PT_OK;
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
  Pass* h = ps[0];
  if (g.profiling) {  // the batch is timed as the first pass's draw
    if (!h->ev0) { HIPCHK(hipEventCreate(&h->ev0)); HIPCHK(hipEventCreate(&h->ev1)); }
    HIPCHK(hipEventRecord(h->ev0, g.stream));
  }
  TRY(draw_pathtrace_batch(ps, count));
  if (g.profiling) {
    HIPCHK(hipEventRecord(h->ev1, g.stream));
    h->timed = true;
  }
  return PT_OK;
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

// capi_geometry.hip — the entry points of include/ptsvgf.h for geometry that moves (DESIGN.md "Dynamic scenes"): the
// device BVH build and its refit, the rasterize pass's binds and refit, posed objects, and their debug readbacks, over
// the library state of capi_state.h. What a build, a refit and a pose have in common is one function each here.
#include <algorithm>
#include <cstring>

#include "../../include/ptsvgf_debug.h"
#include "../../include/ptsvgf_debug_pose.h"
#include "../../include/ptsvgf_debug_refit.h"
#include "capi_state.h"
#include "glsl_builtins.h"
#include "host_trees.h"

using namespace ptapi;

namespace {

using namespace ptk;

constexpr int kPoseMaxObjects = 4096;

// a heap-held refit state or set of walk trees with what it holds on the device (null: nothing)
void delete_refit(LbvhRefit* r) {
  if (r) lbvh_refit_free(*r);
  delete r;
}
void delete_trees(LbvhTrees* t) {
  if (t) lbvh_trees_free(*t);
  delete t;
}
// owners that release on scope exit
using RefitPtr = std::unique_ptr<LbvhRefit, void (*)(LbvhRefit*)>;
using TreesPtr = std::unique_ptr<LbvhTrees, void (*)(LbvhTrees*)>;
struct TreesGuard {  // trees that never leave the call
  LbvhTrees t;
  ~TreesGuard() { lbvh_trees_free(t); }
};
struct DevFree {
  void operator()(void* p) const { (void)hipFree(p); }
};

// the skin's device copies (pt_pose_set_skin)
void free_skin(Pose& p) {
  void* dev[] = {p.sk_tri_bones, p.sk_tri_weights, p.sk_r_bones, p.sk_r_weights};
  for (void* d : dev)
    if (d) (void)hipFree(d);
  p.sk_tri_bones = p.sk_r_bones = nullptr;
  p.sk_tri_weights = p.sk_r_weights = nullptr;
  p.skinned = false;
  p.skin_max = 0;
}

}  // namespace

namespace ptapi {

void free_trees(Texture* t) {
  delete_trees(t->trees);
  t->trees = nullptr;
}

void free_refit(Texture* t) {
  delete_refit(t->refit);
  t->refit = nullptr;
}

void free_raster_refit(RasterScene& r) {
  if (r.enc_nodes) (void)hipFree(r.enc_nodes);
  r.enc_nodes = nullptr;
  delete_refit(r.refit);
  r.refit = nullptr;
}

void free_pose(Pose& p) {
  float* dev[] = {p.tri_rest, p.tri_posed, p.r_rest, p.r_list[0], p.r_list[1], p.mats_dev};
  for (float* d : dev)
    if (d) (void)hipFree(d);
  if (p.r_obj) (void)hipFree(p.r_obj);
  if (p.disp_spare) (void)hipFree(p.disp_spare);
  if (p.mats_host) (void)hipHostFree(p.mats_host);
  free_skin(p);
  p = Pose{};
}

}  // namespace ptapi

namespace {

// Device time of what a call issues on one stream between start and stop, for its out_ms (null: nothing is recorded).
// The call reads it after its own synchronisation of that stream, so no wait is added for the events.
struct EventTimer {
  float* out;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit EventTimer(float* out_ms) : out(out_ms) {}
  ~EventTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  void start(hipStream_t s) {
    if (!out) return;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, s);
  }
  void stop(hipStream_t s) { if (out) (void)hipEventRecord(e1, s); }
  void read() {
    if (out && hipEventElapsedTime(out, e0, e1) != hipSuccess) *out = 0.0f;
  }
};

// the one wait of a build, a refit or a pose, also after a failure: the stages' counters are copied into their trees
int sync_after(const char* who, int rc, hipStream_t s) {
  const hipError_t e = hipStreamSynchronize(s);
  return e != hipSuccess && rc == PT_OK ? hip_err(e, who) : rc;
}

// the displacement records of a rasterize pass (pt_raster_pass_set_prev_vertices), freed once no draw reads them
void drop_disp(Pass* p) {
  if (!p->raster.disp) return;
  raster_touch(p);
  (void)hipDeviceSynchronize();
  (void)hipFree(p->raster.disp);
  p->raster.disp = nullptr;
}

// Replace a texbuffer's contents with `bytes` of device data (device + host copy), as a fresh upload would.
int texbuffer_take(Texture* t, const void* dev_src, size_t bytes) {
  if (t->bytes != bytes || !t->dev) {
    if (t->owned && t->dev) (void)hipFree(t->dev);
    t->dev = nullptr;
    if (bytes) HIPCHK(hipMalloc(&t->dev, bytes));
    t->owned = true;
  }
  t->bytes = bytes;
  t->W = (int)(bytes / 12);
  t->host.resize(bytes);
  if (bytes) {
    HIPCHK(hipMemcpyAsync(t->dev, dev_src, bytes, hipMemcpyDeviceToDevice, g.stream));
    HIPCHK(hipMemcpyAsync(t->host.data(), dev_src, bytes, hipMemcpyDeviceToHost, g.stream));
  }
  t->version++;
  t->lbvh = true;
  t->host_stale = false;
  return PT_OK;
}

// tri_out and node_out (with a refit's tri_in, when given) as handles, then as the pair one pt_bvh_build wrote and
// nothing has written since. Texts carry the entry point's name `who`.
int refit_pair(const char* who, uint32_t tri_out, uint32_t node_out, Texture** to_out, Texture** no_out,
               const uint32_t* tri_in = nullptr) {
  const std::string w = std::string(who) + ": ", names = tri_in ? "tri_in, tri_out and node_out" : "tri_out and node_out";
  auto buffer = [](uint32_t h) { return tex_of(h) && tex_of(h)->target == PT_TEXTURE_BUFFER; };
  if (!buffer(tri_out) || !buffer(node_out) || (tri_in && !buffer(*tri_in)))
    return err(PT_ERR_ARG, w + names + " must be texture buffers");
  Texture *to = tex_of(tri_out), *no = tex_of(node_out);
  if (tri_out == node_out || (tri_in && (*tri_in == tri_out || *tri_in == node_out)))
    return err(PT_ERR_ARG, w + names + " must be " + (tri_in ? "three" : "two") + " different buffers");
  const LbvhRefit* rf = no->refit;
  if (!to->lbvh || !no->lbvh || !rf || !rf->base || rf->nnodes < 2 || !no->trees || no->refit_tri != tri_out ||
      no->refit_tri_ver != to->version || no->refit_node_ver != no->version || no->trees->version != no->version ||
      !to->dev || !no->dev || to->bytes != (size_t)rf->n * 45 * sizeof(float) ||
      no->bytes != (size_t)rf->nnodes * 12 * sizeof(float))
    return err(PT_ERR_STATE, w + "tri_out and node_out are not the untouched pair of one pt_bvh_build");
  *to_out = to;
  *no_out = no;
  return PT_OK;
}

// After the call's synchronisation: the counters of the walk trees launched for a node buffer (trc: the launch's code)
int trees_finish(const char* who, LbvhTrees& trees, int trc, int rc) {
  if (rc == PT_OK && trc == 0) trc = lbvh_trees_finish(trees);
  if (rc == PT_OK && trc != 0) rc = err(PT_ERR_HIP, std::string(who) + ": deriving the walk trees failed");
  return rc;
}

// The new trees become the node buffer's, of the versions the pair has now; after a failure the pair can no longer be
// refitted (the trees go with their owner)
void trees_install(Texture* to, Texture* no, TreesPtr& trees, int rc) {
  if (rc != PT_OK) return free_refit(no);
  trees->version = no->version;
  no->trees = trees.release();
  no->refit_tri_ver = to->version;
  no->refit_node_ver = no->version;
}

// The end of a refit that wrote the pair where it lies: the contents changed whatever came of it, so the old trees go
// and every consumer re-reads
int refit_pair_commit(const char* who, Texture* to, Texture* no, TreesPtr& trees, int trc, int rc) {
  rc = trees_finish(who, *trees, trc, rc);
  to->version++;
  no->version++;
  to->host_stale = no->host_stale = true;
  free_trees(no);
  trees_install(to, no, trees, rc);
  return rc;
}

// prefix: of the texts, for an entry point that names itself in them
int raster_pass_of(uint32_t pass, Pass** out, const char* prefix = "") {
  Pass* p = pass_of(pass);
  if (!p) return err(PT_ERR_INVALID_HANDLE, std::string(prefix) + "invalid pass");
  if (g.programs[p->program] != PK_RASTER) return err(PT_ERR_ARG, std::string(prefix) + "not a rasterize pass");
  *out = p;
  return PT_OK;
}

// A rasterize pass that holds what a refit needs: its own triangles, bound by pt_raster_pass_bind_device. (Such a
// bind sets refit and bvh_records >= 1 together, and nothing sets refit elsewhere.)
int refit_pass(const char* who, Pass* p) {
  const std::string w = std::string(who) + ": ";
  if (p->raster_src) return err(PT_ERR_ARG, w + "the pass shares another pass's triangles");
  const RasterScene& rs = p->raster;
  if (!p->bound || !rs.refit || !rs.refit->base || !rs.enc_nodes || !rs.geom || !rs.nrm || !rs.bvh ||
      rs.refit->n != rs.ntris)
    return err(PT_ERR_STATE, w + "the pass was not bound by pt_raster_pass_bind_device (or took its host fallback): "
                                 "bind again");
  return PT_OK;
}

// The raster refit for the vertex list dverts, issued on s: the records in the kept leaf order (the original index in
// geom[4k].w stays), the boxes of the kept nodes, then the packed tree from the device stage as in the bind.
int raster_refit_issue(RasterScene& rs, const float* dverts, LbvhTrees& trees, hipStream_t s) {
  LbvhRefit& rf = *rs.refit;
  int rc = decode_raster(dverts, rf.order, rs.ntris, rs.geom, rs.nrm, s);
  if (rc == 0) rc = lbvh_refit_nodes(rf, rs.enc_nodes, dverts, kRasterVerts, s);
  if (rc == 0) rc = lbvh_trees_launch(g_lbvh, rs.enc_nodes, rf.nnodes, trees, s, rf.err);
  return rc;
}

// The packed tree into the pass's own copy, issued before the counters are back: trees.bin has the bind's room (it
// follows from the node count), which held the bind's records; raster_refit_finish checks the counters afterwards.
int raster_refit_copy(RasterScene& rs, const LbvhTrees& trees, hipStream_t s) {
  return (int)hipMemcpyAsync(rs.bvh, trees.bin, (size_t)rs.bvh_records * 4 * sizeof(float4), hipMemcpyDeviceToDevice, s);
}

// After the synchronisation (rc: what came of the calls above). On a failure the records may be half written: the
// pass loses its refit state and the caller binds again.
int raster_refit_finish(RasterScene& rs, LbvhTrees& trees, int rc) {
  if (rc == 0) rc = lbvh_trees_finish(trees);
  if (rc == 0 && (trees.dev_info[1] != rs.stack_need || std::max(1, trees.nbin()) != rs.bvh_records))
    rc = (int)hipErrorInvalidValue;  // the topology is the bind's: the same depth and as many records
  if (rc == 0) rs.root_ref = trees.dev_info[0];
  else free_raster_refit(rs);
  return rc;
}

// What pt_pose_apply and pt_pose_apply_skin do once their own arguments are checked: the checks they share, then a
// pt_bvh_refit with the placed list standing for tri_in and a pt_raster_pass_refit_device with the placed raster list.
// fill() writes the call's table into ps.mats_host and returns its floats; place(r_out, s) issues the kernels that
// write ps.tri_posed and (with a raster list) r_out from the rest lists and ps.mats_dev. Texts carry `who`.
template <class Fill, class Place>
int pose_apply_with(const char* who, Pose& ps, uint32_t tri_out, uint32_t node_out, uint32_t raster_pass, int motion,
                    float* out_ms, Fill fill, Place place) {
  const std::string w = std::string(who) + ": ";
  Texture *to = nullptr, *no = nullptr;
  TRY(refit_pair(who, tri_out, node_out, &to, &no));
  LbvhRefit* rf = no->refit;
  if (rf->n != ps.ntris) return err(PT_ERR_ARG, w + "the pose holds another triangle count than the build");
  Pass* p = nullptr;
  if (raster_pass) {
    if (!ps.rtris) return err(PT_ERR_ARG, w + "the pose was created without a raster list");
    TRY(raster_pass_of(raster_pass, &p, w.c_str()));
    TRY(refit_pass(who, p));
    if (p->raster.ntris != ps.rtris) return err(PT_ERR_ARG, w + "the pose holds another raster triangle count");
  }
  TRY(materials_order(g.stream));  // the rest list and tri_out as every pt_materials_update so far left them
  // displacement records: the pass's own are rewritten where they lie, else the pair a pose without motion set aside
  float4* disp = nullptr;
  if (p && motion) {
    disp = p->raster.disp ? p->raster.disp : ps.disp_spare;
    if (!disp && hipMalloc((void**)&disp, (size_t)ps.rtris * 3 * sizeof(float4)) != hipSuccess)
      return err(PT_ERR_HIP, w + "out of device memory");
    if (disp == ps.disp_spare) ps.disp_spare = nullptr;
  }
  const size_t table_floats = fill();
  hipStream_t s = g.stream;
  int rc = (int)hipMemcpyAsync(ps.mats_dev, ps.mats_host, table_floats * sizeof(float), hipMemcpyHostToDevice, s);
  if (rc != 0) {
    if (disp && disp != p->raster.disp) ps.disp_spare = disp;
    return hip_err((hipError_t)rc, who);
  }
  if (p) {
    raster_touch(p);  // the records, the tree and the displacement records are rewritten below
    if (motion) {
      p->raster.disp = disp;
    } else if (p->raster.disp) {  // left without records, as a refit leaves it; no draw reads them (see the header)
      if (ps.disp_spare) (void)hipFree(ps.disp_spare);
      ps.disp_spare = p->raster.disp;
      p->raster.disp = nullptr;
    }
  }
  EventTimer timer(out_ms);
  timer.start(s);
  const int nxt = ps.cur ^ 1;
  rc = place(ps.r_list[nxt], s);
  if (rc == 0) rc = lbvh_refit_reorder(*rf, ps.tri_posed, (float*)to->dev, s);
  if (rc == 0) rc = lbvh_refit_nodes(*rf, (float*)no->dev, ps.tri_posed, kTriEncoded, s);
  TreesPtr trees(new LbvhTrees, delete_trees);
  const bool launched = rc == 0;
  const int trc = launched ? lbvh_trees_launch(g_lbvh, (const float*)no->dev, rf->nnodes, *trees, s, rf->err) : 0;
  // the pass's refit with the new list; out_ms ends with its derivation, before the copies that follow it
  TreesGuard rtrees;
  const bool raster_launched = p && launched && trc == 0;
  int rrc = raster_launched ? raster_refit_issue(p->raster, ps.r_list[nxt], rtrees.t, s) : 0;
  timer.stop(s);
  if (raster_launched && rrc == 0) {
    rrc = raster_refit_copy(p->raster, rtrees.t, s);
    if (rrc == 0 && motion)
      rrc = raster_disp(p->raster.geom, ps.r_list[ps.cur], ps.r_list[nxt], ps.rtris, p->raster.disp, s);
  }
  rc = sync_after(who, rc == 0 ? PT_OK : hip_err((hipError_t)rc, who), s);  // the one wait
  timer.read();
  rc = refit_pair_commit(who, to, no, trees, trc, rc);
  if (ps.rtris && launched) ps.cur = nxt;
  if (p) {
    rrc = raster_refit_finish(p->raster, rtrees.t, rc == PT_OK ? rrc : (int)hipErrorUnknown);
    if (rrc != 0) {
      drop_disp(p);
      if (rc == PT_OK) rc = hip_err((hipError_t)rrc, (w + "refitting the rasterize pass").c_str());
    }
  }
  return rc;
}

}  // namespace

extern "C" {

int pt_bvh_build(uint32_t tri_in, int leaf_n, int ploc_radius, uint32_t tri_out, uint32_t node_out, int* out_nodes,
                 float* out_ms) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture *ti = tex_of(tri_in), *to = tex_of(tri_out), *no = tex_of(node_out);
  if (!ti || !to || !no || ti->target != PT_TEXTURE_BUFFER || to->target != PT_TEXTURE_BUFFER ||
      no->target != PT_TEXTURE_BUFFER)
    return err(PT_ERR_ARG, "pt_bvh_build: tri_in, tri_out and node_out must be texture buffers");
  if (tri_in == tri_out || tri_in == node_out || tri_out == node_out)
    return err(PT_ERR_ARG, "pt_bvh_build: tri_in, tri_out and node_out must be three different buffers");
  if (leaf_n < 1 || leaf_n > 15) return err(PT_ERR_ARG, "pt_bvh_build: leaf_n must be in [1, 15]");
  if (ploc_radius < 0 || ploc_radius > 256) return err(PT_ERR_ARG, "pt_bvh_build: ploc_radius must be in [0, 256]");
  if (ti->bytes == 0 || ti->bytes % (45 * sizeof(float)) || !ti->dev)
    return err(PT_ERR_FORMAT, "pt_bvh_build: tri_in must hold whole Triangle_encoded records (45 floats)");
  const size_t nt = ti->bytes / (45 * sizeof(float));
  if (nt > (1u << 24)) return err(PT_ERR_ARG, "pt_bvh_build: more than 2^24 triangles (float-encoded indices)");
  const int n = (int)nt;
  TRY(materials_order(g.stream));  // tri_in is read and tri_out replaced after every pt_materials_update so far
  float *tbuf = nullptr, *nbuf = nullptr;
  HIPCHK(hipMalloc(&tbuf, nt * 45 * sizeof(float)));
  if (hipMalloc(&nbuf, (size_t)2 * n * 12 * sizeof(float)) != hipSuccess) {
    (void)hipFree(tbuf);
    return err(PT_ERR_HIP, "pt_bvh_build: out of device memory");
  }
  EventTimer timer(out_ms);
  timer.start(g.stream);
  int nodes = 0;
  // what a later pt_bvh_refit needs is kept with the node texture: the leaf order the build writes and the parent
  // links of its output nodes (the allocation of the previous build is reused while the triangle count holds)
  if (!no->refit) no->refit = new LbvhRefit;
  int rc = lbvh_refit_alloc(*no->refit, n);
  if (rc == 0)
    rc = lbvh_build(g_lbvh, (const float*)ti->dev, kTriEncoded, n, leaf_n, ploc_radius, tbuf, nbuf, no->refit->order,
                    &nodes, g.stream);
  if (rc == 0) rc = lbvh_refit_link(*no->refit, nbuf, nodes, g.stream);
  // the walk trees of the new nodes, derived where they lie; their counters arrive with the synchronisation below
  TreesPtr trees(new LbvhTrees, delete_trees);
  const int trc = rc == 0 ? lbvh_trees_launch(g_lbvh, nbuf, nodes, *trees, g.stream) : 0;
  timer.stop(g.stream);
  if (rc == 0) rc = texbuffer_take(to, tbuf, nt * 45 * sizeof(float));
  else rc = hip_err((hipError_t)rc, "lbvh_build");
  if (rc == PT_OK) rc = texbuffer_take(no, nbuf, (size_t)nodes * 12 * sizeof(float));
  rc = sync_after("pt_bvh_build", rc, g.stream);
  timer.read();
  rc = trees_finish("pt_bvh_build", *trees, trc, rc);
  if (no->trees && no->trees->version != no->version) free_trees(no);  // the replaced contents' trees
  trees_install(to, no, trees, rc);  // (the versions moved in texbuffer_take)
  if (rc == PT_OK) no->refit_tri = tri_out;
  (void)hipFree(tbuf);
  (void)hipFree(nbuf);
  if (rc == PT_OK && out_nodes) *out_nodes = nodes;
  return rc;
}

int pt_bvh_refit(uint32_t tri_in, uint32_t tri_out, uint32_t node_out, float* out_ms) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture *to = nullptr, *no = nullptr;
  TRY(refit_pair("pt_bvh_refit", tri_out, node_out, &to, &no, &tri_in));
  const Texture* ti = tex_of(tri_in);
  if (ti->bytes == 0 || ti->bytes % (45 * sizeof(float)) || !ti->dev)
    return err(PT_ERR_ARG, "pt_bvh_refit: tri_in must hold whole Triangle_encoded records (45 floats)");
  if (ti->bytes != to->bytes) return err(PT_ERR_ARG, "pt_bvh_refit: tri_in holds another triangle count than the build");
  LbvhRefit* rf = no->refit;
  TRY(materials_order(g.stream));  // tri_in is read and tri_out overwritten after every pt_materials_update so far
  EventTimer timer(out_ms);
  timer.start(g.stream);
  // both buffers are written where they lie: no staging, no copy (the host mirrors turn lazy, refresh_host)
  int rc = lbvh_refit_reorder(*rf, (const float*)ti->dev, (float*)to->dev, g.stream);
  if (rc == 0) rc = lbvh_refit_nodes(*rf, (float*)no->dev, (const float*)ti->dev, kTriEncoded, g.stream);
  TreesPtr trees(new LbvhTrees, delete_trees);
  const int trc = rc == 0 ? lbvh_trees_launch(g_lbvh, (const float*)no->dev, rf->nnodes, *trees, g.stream, rf->err) : 0;
  timer.stop(g.stream);
  rc = sync_after("pt_bvh_refit", rc == 0 ? PT_OK : hip_err((hipError_t)rc, "pt_bvh_refit"), g.stream);
  timer.read();
  return refit_pair_commit("pt_bvh_refit", to, no, trees, trc, rc);
}

int pt_debug_lbvh_order(uint32_t node_tex, int* host_out, size_t cap, size_t* n) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(node_tex);
  if (!t || t->target != PT_TEXTURE_BUFFER) return err(PT_ERR_INVALID_HANDLE, "pt_debug_lbvh_order: not a texture buffer");
  if (!t->lbvh || !t->refit || !t->refit->base || t->refit_node_ver != t->version)
    return err(PT_ERR_STATE, "pt_debug_lbvh_order: not a node buffer pt_bvh_build wrote");
  if (n) *n = (size_t)t->refit->n;
  if (!host_out) return PT_OK;
  if (cap < (size_t)t->refit->n) return err(PT_ERR_ARG, "pt_debug_lbvh_order: host_out is too small");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_out, t->refit->order, sizeof(int) * (size_t)t->refit->n, hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_debug_lbvh_trees(uint32_t node_tex, int source, int which, void* host_out, size_t cap, size_t* bytes,
                        int* info8) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Texture* t = tex_of(node_tex);
  if (!t || t->target != PT_TEXTURE_BUFFER) return err(PT_ERR_INVALID_HANDLE, "pt_debug_lbvh_trees: not a texture buffer");
  if (!t->lbvh || !t->trees || t->trees->version != t->version)
    return err(PT_ERR_STATE, "pt_debug_lbvh_trees: not a node buffer pt_bvh_build wrote");
  if (source < 0 || source > 1 || which < 0 || which > 2) return err(PT_ERR_ARG, "pt_debug_lbvh_trees: source 0-1, which 0-2");
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<Float4> host;
  const void* src = nullptr;
  size_t n = 0;
  if (source == 0) {
    const LbvhTrees& tr = *t->trees;
    for (int i = 0; i < 7; ++i) info[i] = tr.dev_info[i];
    info[7] = (int)lrintf(tr.stage_ms * 1000.0f);
    src = which == 0 ? tr.bin : which == 1 ? tr.leaves : tr.wide;
    n = which == 0 ? (size_t)tr.nbin() * 4 : which == 1 ? (size_t)tr.nleaves() * 2 : (size_t)tr.nwide() * kWideStride;
  } else {
    // the host functions over the host mirror of the texels: what the device stage has to equal
    TRY(refresh_host(t));
    const float* ne = (const float*)t->host.data();
    const int nnodes = (int)(t->host.size() / (12 * sizeof(float)));
    std::vector<Float4> bin, leaves, wide;
    std::string msg;
    if (const int rc = pack_bvh(ne, nnodes, bin, &info[0], (1 << 24) + 15, &info[1], &msg)) return err(rc, msg);
    collect_leaves(ne, (size_t)nnodes, leaves);
    info[2] = (int)(leaves.size() / 2);
    TRY(pack_wide_encoded(ne, nnodes, wide, &info[3], &info[4]));
    info[5] = (int)(wide.size() / kWideStride);
    info[6] = wide_has_nan(wide);
    host.swap(which == 0 ? bin : which == 1 ? leaves : wide);
    n = host.size();
  }
  if (bytes) *bytes = n * sizeof(float4);
  if (info8) memcpy(info8, info, sizeof(info));
  if (host_out && n) {
    if (cap < n * sizeof(float4)) return err(PT_ERR_ARG, "pt_debug_lbvh_trees: host_out is too small");
    if (source == 0) HIPCHK(hipMemcpy(host_out, src, n * sizeof(float4), hipMemcpyDeviceToHost));
    else memcpy(host_out, host.data(), n * sizeof(float4));
  }
  return PT_OK;
}

int pt_raster_pass_bind(uint32_t pass, const float* verts, size_t n_floats) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Pass* p = nullptr;
  TRY(raster_pass_of(pass, &p));
  if (n_floats % 18) return err(PT_ERR_ARG, "vertex list must be whole triangles of pos3+nrm3");
  int ntris = (int)(n_floats / 18);
  raster_touch(p);  // new triangles and tree: the next G-buffer draw of this pass and of its sharers draws
  drop_disp(p);  // the triangle order changes
  free_raster_refit(p->raster);  // a host-built tree is not refitted
  p->raster.ntris = ntris;
  p->raster_src = 0;
  p->bound = true;
  if (ntris == 0) return PT_OK;
  // SAH tree over the raster triangles (build_raster_tree: the walk's answer does not depend on the tree);
  // geom in leaf order, objIndex = original index (the depth-test tie rule)
  std::vector<int> order;
  std::vector<Float4> bvh;
  int root = 0;
  std::string msg;
  if (const int rc = build_raster_tree(verts, ntris, order, bvh, &root, &p->raster.stack_need, &msg))
    return err(rc, msg);
  using namespace glsl;
  std::vector<float4> geom((size_t)ntris * 4), nrm((size_t)ntris * 3);
  for (int k = 0; k < ntris; ++k) {
    const int oi = order[k];
    const float* f = verts + (size_t)oi * 18;
    v3 p1 = mk(f[0], f[1], f[2]), p2 = mk(f[6], f[7], f[8]), p3 = mk(f[12], f[13], f[14]);
    v3 e1 = sub(p2, p1), e2 = sub(p3, p1), ng = cross(e1, e2);
    float oif;
    memcpy(&oif, &oi, 4);
    float4* q = &geom[(size_t)k * 4];
    q[0] = float4{p1.x, p1.y, p1.z, oif};
    q[1] = float4{e1.x, e1.y, e1.z, 0};
    q[2] = float4{e2.x, e2.y, e2.z, 0};
    q[3] = float4{ng.x, ng.y, ng.z, 0};
    float4* n = &nrm[(size_t)k * 3];
    n[0] = float4{f[3], f[4], f[5], 0};
    n[1] = float4{f[9], f[10], f[11], 0};
    n[2] = float4{f[15], f[16], f[17], 0};
  }
  if (bvh.empty()) bvh.push_back(Float4{0, 0, 0, 0});
  TRY(upload_vec(geom, &p->raster.geom));
  TRY(upload_vec(nrm, &p->raster.nrm));
  TRY(upload_vec(bvh, &p->raster.bvh));
  p->raster.root_ref = root;
  return PT_OK;
}

int pt_raster_pass_bind_device(uint32_t pass, const void* dverts, size_t n_floats, int ploc_radius) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Pass* p = nullptr;
  TRY(raster_pass_of(pass, &p));
  if (n_floats % 18) return err(PT_ERR_ARG, "vertex list must be whole triangles of pos3+nrm3");
  if (ploc_radius < 0 || ploc_radius > 256) return err(PT_ERR_ARG, "ploc_radius must be in [0, 256]");
  if (n_floats / 18 > (1u << 24)) return err(PT_ERR_ARG, "more than 2^24 raster triangles");
  const int ntris = (int)(n_floats / 18);
  if (ntris > 0 && !dverts) return err(PT_ERR_ARG, "null device vertex list");
  raster_touch(p);
  drop_disp(p);  // the triangle order changes
  RasterScene& rs = p->raster;
  rs.ntris = ntris;
  p->raster_src = 0;
  p->bound = true;
  free_raster_refit(rs);  // of the bind this one replaces
  if (ntris == 0) return PT_OK;
  // the encoded nodes, the leaf order and the parent links stay with the pass after a device bind
  // (pt_raster_pass_refit_device); until then, and on every other way out, they are released here
  RefitPtr rf(new LbvhRefit, delete_refit);
  float* nraw = nullptr;
  HIPCHK(hipMalloc(&nraw, (size_t)2 * ntris * 12 * sizeof(float)));
  std::unique_ptr<float, DevFree> nbuf(nraw);
  if (lbvh_refit_alloc(*rf, ntris) != 0) return err(PT_ERR_HIP, "pt_raster_pass_bind_device: out of device memory");
  int nodes = 0;
  int rc = lbvh_build(g_lbvh, (const float*)dverts, kRasterVerts, ntris, 8, ploc_radius, nullptr, nbuf.get(), rf->order,
                      &nodes, g.stream);
  if (rc == 0) rc = lbvh_refit_link(*rf, nbuf.get(), nodes, g.stream);
  if (rc) return hip_err((hipError_t)rc, "raster lbvh_build");
  // the packed binary tree (pack_bvh's records) and its depth come from the device stage: no node readback
  TreesGuard tg;
  LbvhTrees& trees = tg.t;
  rc = lbvh_trees_launch(g_lbvh, nbuf.get(), nodes, trees, g.stream);
  if (hipStreamSynchronize(g.stream) != hipSuccess && rc == 0) rc = (int)hipErrorUnknown;
  if (rc == 0) rc = lbvh_trees_finish(trees);
  const int root = trees.dev_info[0], need = trees.dev_info[1];
  if (rc != 0 || need >= kStack) {
    // the G-buffer walk's stack holds kStack entries: a deeper device tree (coincident centroids) takes the host
    // bind, whose SAH builder caps the depth; the G-buffer does not depend on the tree
    lbvh_trees_free(trees);
    std::vector<float> hv(n_floats);
    const bool ok = hipMemcpy(hv.data(), dverts, n_floats * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
    nbuf.reset();  // (before the host bind allocates)
    rf.reset();
    if (!ok) return err(PT_ERR_HIP, "pt_raster_pass_bind_device: vertex readback");
    return pt_raster_pass_bind(pass, hv.data(), n_floats);
  }
  if (rs.geom) (void)hipFree(rs.geom);
  if (rs.nrm) (void)hipFree(rs.nrm);
  rs.geom = rs.nrm = nullptr;
  if (hipMalloc((void**)&rs.geom, (size_t)ntris * 4 * sizeof(float4)) != hipSuccess ||
      hipMalloc((void**)&rs.nrm, (size_t)ntris * 3 * sizeof(float4)) != hipSuccess)
    return err(PT_ERR_HIP, "pt_raster_pass_bind_device: out of device memory");
  rc = decode_raster((const float*)dverts, rf->order, ntris, rs.geom, rs.nrm, g.stream);
  if (rc) return hip_err((hipError_t)rc, "decode_raster");
  // the pass owns a copy sized to the tree (an empty tree: one zero record, as the host bind uploads)
  const int records = std::max(1, trees.nbin());
  const size_t bvh_bytes = (size_t)records * 4 * sizeof(float4);
  if (rs.bvh) { (void)hipFree(rs.bvh); rs.bvh = nullptr; }
  if (hipMalloc((void**)&rs.bvh, bvh_bytes) != hipSuccess ||
      hipMemcpyAsync(rs.bvh, trees.bin, bvh_bytes, hipMemcpyDeviceToDevice, g.stream) != hipSuccess)
    return err(PT_ERR_HIP, "pt_raster_pass_bind_device: out of device memory");
  rs.root_ref = root;
  rs.stack_need = need;
  // draws of other frames may run on other streams: the records are complete when this returns
  if (const hipError_t e = hipStreamSynchronize(g.stream)) return hip_err(e, "pt_raster_pass_bind_device");
  rs.enc_nodes = nbuf.release();
  rs.refit = rf.release();
  rs.bvh_records = records;
  return PT_OK;
}

int pt_raster_pass_refit_device(uint32_t pass, const void* dverts, size_t n_floats) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Pass* p = nullptr;
  TRY(raster_pass_of(pass, &p));
  TRY(refit_pass("pt_raster_pass_refit_device", p));
  RasterScene& rs = p->raster;
  if (n_floats != (size_t)rs.ntris * 18)
    return err(PT_ERR_ARG, "pt_raster_pass_refit_device: not the bound triangle count");
  if (!dverts) return err(PT_ERR_ARG, "null device vertex list");
  raster_touch(p);
  drop_disp(p);  // their values are stale
  TreesGuard trees;
  int rc = raster_refit_issue(rs, (const float*)dverts, trees.t, g.stream);
  if (rc == 0) rc = raster_refit_copy(rs, trees.t, g.stream);
  // draws of other frames may run on other streams: the records are complete when this returns
  if (hipStreamSynchronize(g.stream) != hipSuccess && rc == 0) rc = (int)hipErrorUnknown;
  rc = raster_refit_finish(rs, trees.t, rc);
  return rc ? hip_err((hipError_t)rc, "pt_raster_pass_refit_device") : PT_OK;
}

int pt_raster_pass_set_prev_vertices(uint32_t pass, const void* dprev, const void* dcur, size_t n_floats) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  Pass* p = nullptr;
  TRY(raster_pass_of(pass, &p));
  if (p->raster_src) return err(PT_ERR_ARG, "pt_raster_pass_set_prev_vertices: the pass shares another pass's triangles");
  if (!p->bound) return err(PT_ERR_ARG, "pt_raster_pass_set_prev_vertices: raster pass not bound");
  raster_touch(p);  // the records come, go or change
  if (!dprev) {
    drop_disp(p);
    return PT_OK;
  }
  if (n_floats != (size_t)p->raster.ntris * 18)
    return err(PT_ERR_ARG, "pt_raster_pass_set_prev_vertices: not the bound triangle count");
  if (!dcur) return err(PT_ERR_ARG, "null device vertex list");
  drop_disp(p);
  const int ntris = p->raster.ntris;
  if (ntris == 0) return PT_OK;
  if (!p->raster.geom) return err(PT_ERR_ARG, "pt_raster_pass_set_prev_vertices: raster pass not bound");
  float4* disp = nullptr;
  HIPCHK(hipMalloc((void**)&disp, (size_t)ntris * 3 * sizeof(float4)));
  const int rc = raster_disp(p->raster.geom, (const float*)dprev, (const float*)dcur, ntris, disp, g.stream);
  // draws of other frames may run on other streams: the records are complete when this returns
  const hipError_t e = rc ? (hipError_t)rc : hipStreamSynchronize(g.stream);
  if (e != hipSuccess) {
    (void)hipFree(disp);
    return hip_err(e, "pt_raster_pass_set_prev_vertices");
  }
  p->raster.disp = disp;
  return PT_OK;
}

int pt_pose_create(uint32_t tri_rest, const float* raster_rest, size_t n_floats, const int* raster_obj,
                   uint32_t* out_pose) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  if (!out_pose) return err(PT_ERR_ARG, "pt_pose_create: null out_pose");
  Texture* t = tex_of(tri_rest);
  if (!t || t->target != PT_TEXTURE_BUFFER) return err(PT_ERR_ARG, "pt_pose_create: tri_rest must be a texture buffer");
  if (t->bytes == 0 || t->bytes % (45 * sizeof(float)) || !t->dev)
    return err(PT_ERR_ARG, "pt_pose_create: tri_rest must hold whole Triangle_encoded records (45 floats)");
  const size_t nt = t->bytes / (45 * sizeof(float));
  if (nt > (1u << 24)) return err(PT_ERR_ARG, "pt_pose_create: more than 2^24 triangles");
  if (n_floats % 18) return err(PT_ERR_ARG, "pt_pose_create: the raster list must be whole triangles of pos3+nrm3");
  if (n_floats / 18 > (1u << 24)) return err(PT_ERR_ARG, "pt_pose_create: more than 2^24 raster triangles");
  if (n_floats && (!raster_rest || !raster_obj))
    return err(PT_ERR_ARG, "pt_pose_create: a raster list needs its vertices and one object per triangle");
  std::unique_ptr<Pose> ps(new Pose);
  ps->ntris = (int)nt;
  ps->rtris = (int)(n_floats / 18);
  const size_t rbytes = n_floats * sizeof(float), mbytes = (size_t)kPoseMaxObjects * kPoseMatFloats * sizeof(float);
  hipError_t e = hipMalloc((void**)&ps->tri_rest, t->bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&ps->tri_posed, t->bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&ps->mats_dev, mbytes);
  if (e == hipSuccess) e = hipHostMalloc((void**)&ps->mats_host, mbytes, hipHostMallocDefault);
  if (e == hipSuccess && ps->rtris) {
    e = hipMalloc((void**)&ps->r_rest, rbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&ps->r_list[0], rbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&ps->r_list[1], rbytes);
    if (e == hipSuccess) e = hipMalloc((void**)&ps->r_obj, (size_t)ps->rtris * sizeof(int));
  }
  // on the library stream: tri_rest may have been written there (or, by pt_materials_update, on that call's stream)
  if (e == hipSuccess && materials_order(g.stream) != PT_OK) e = hipErrorUnknown;
  if (e == hipSuccess) e = hipMemcpyAsync(ps->tri_rest, t->dev, t->bytes, hipMemcpyDeviceToDevice, g.stream);
  if (e == hipSuccess && ps->rtris) {
    e = hipMemcpyAsync(ps->r_rest, raster_rest, rbytes, hipMemcpyHostToDevice, g.stream);
    if (e == hipSuccess)
      e = hipMemcpyAsync(ps->r_obj, raster_obj, (size_t)ps->rtris * sizeof(int), hipMemcpyHostToDevice, g.stream);
    for (int k = 0; k < 2 && e == hipSuccess; ++k)
      e = hipMemcpyAsync(ps->r_list[k], ps->r_rest, rbytes, hipMemcpyDeviceToDevice, g.stream);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
  if (e != hipSuccess) {
    free_pose(*ps);
    return hip_err(e, "pt_pose_create");
  }
  const uint32_t h = g.next++;
  g.poses[h] = std::move(ps);
  *out_pose = h;
  return PT_OK;
}

int pt_pose_destroy(uint32_t pose) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto it = g.poses.find(pose);
  if (it == g.poses.end()) return err(PT_ERR_INVALID_HANDLE, "pt_pose_destroy: unknown pose");
  (void)hipDeviceSynchronize();  // a pt_pose_apply has completed; nothing else reads the lists
  free_pose(*it->second);
  g.poses.erase(it);
  return PT_OK;
}

int pt_pose_apply(uint32_t pose, const float* mats16, int n_obj, uint32_t tri_out, uint32_t node_out,
                  uint32_t raster_pass, int motion, float* out_ms) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto pit = g.poses.find(pose);
  if (pit == g.poses.end()) return err(PT_ERR_INVALID_HANDLE, "pt_pose_apply: unknown pose");
  Pose& ps = *pit->second;
  if (!mats16) return err(PT_ERR_ARG, "pt_pose_apply: null mats16");
  if (n_obj < 1 || n_obj > kPoseMaxObjects) return err(PT_ERR_ARG, "pt_pose_apply: n_obj must be in [1, 4096]");
  // the table: each matrix with the cofactor columns of its upper 3x3 (cross products of its columns), once per object
  auto fill = [&] {
    for (int k = 0; k < n_obj; ++k) {
      const float* m = mats16 + (size_t)k * 16;
      float* o = ps.mats_host + (size_t)k * kPoseMatFloats;
      memcpy(o, m, 16 * sizeof(float));
      const glsl::v3 c0 = glsl::mk(m[0], m[1], m[2]), c1 = glsl::mk(m[4], m[5], m[6]), c2 = glsl::mk(m[8], m[9], m[10]);
      const glsl::v3 a[3] = {glsl::cross(c1, c2), glsl::cross(c2, c0), glsl::cross(c0, c1)};
      for (int j = 0; j < 3; ++j) {
        o[16 + 3 * j] = a[j].x;
        o[17 + 3 * j] = a[j].y;
        o[18 + 3 * j] = a[j].z;
      }
    }
    return (size_t)n_obj * kPoseMatFloats;
  };
  auto place = [&](float* r_out, hipStream_t s) {
    int rc = pose_tris_launch(ps.tri_rest, ps.ntris, ps.mats_dev, n_obj, ps.tri_posed, s);
    if (rc == 0 && ps.rtris) rc = pose_raster_launch(ps.r_rest, ps.r_obj, ps.rtris, ps.mats_dev, n_obj, r_out, s);
    return rc;
  };
  return pose_apply_with("pt_pose_apply", ps, tri_out, node_out, raster_pass, motion, out_ms, fill, place);
}

int pt_pose_set_skin(uint32_t pose, const uint16_t* tri_bones, const float* tri_weights, const uint16_t* raster_bones,
                     const float* raster_weights) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto pit = g.poses.find(pose);
  if (pit == g.poses.end()) return err(PT_ERR_INVALID_HANDLE, "pt_pose_set_skin: unknown pose");
  Pose& ps = *pit->second;
  if (!tri_bones || !tri_weights) return err(PT_ERR_ARG, "pt_pose_set_skin: null tri_bones or tri_weights");
  if (ps.rtris ? !raster_bones || !raster_weights : raster_bones || raster_weights)
    return err(PT_ERR_ARG, ps.rtris ? "pt_pose_set_skin: the pose has a raster list and needs its influences"
                                    : "pt_pose_set_skin: raster influences for a pose without a raster list");
  // the new skin whole, then the old one released: a failed call leaves the pose as it was
  const size_t nt = (size_t)ps.ntris * 12, nr = (size_t)ps.rtris * 12;
  std::unique_ptr<void, DevFree> tb, tw, rb, rw;
  auto up = [](std::unique_ptr<void, DevFree>& d, const void* src, size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    d.reset(p);
    if (e == hipSuccess) e = hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, g.stream);
    return e;
  };
  hipError_t e = up(tb, tri_bones, nt * sizeof(uint16_t));
  if (e == hipSuccess) e = up(tw, tri_weights, nt * sizeof(float));
  if (e == hipSuccess && nr) e = up(rb, raster_bones, nr * sizeof(uint16_t));
  if (e == hipSuccess && nr) e = up(rw, raster_weights, nr * sizeof(float));
  const hipError_t es = hipStreamSynchronize(g.stream);  // the caller's arrays are free again, also after a failure
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return hip_err(e, "pt_pose_set_skin");
  int mx = 0;
  for (size_t i = 0; i < nt; ++i) mx = std::max(mx, (int)tri_bones[i]);
  for (size_t i = 0; i < nr; ++i) mx = std::max(mx, (int)raster_bones[i]);
  free_skin(ps);  // an apply has completed: nothing reads the old influences
  ps.sk_tri_bones = (uint16_t*)tb.release();
  ps.sk_tri_weights = (float*)tw.release();
  ps.sk_r_bones = (uint16_t*)rb.release();
  ps.sk_r_weights = (float*)rw.release();
  ps.skin_max = mx;
  ps.skinned = true;
  return PT_OK;
}

int pt_pose_apply_skin(uint32_t pose, const float* bones16, int n_bones, uint32_t tri_out, uint32_t node_out,
                       uint32_t raster_pass, int motion, float* out_ms) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto pit = g.poses.find(pose);
  if (pit == g.poses.end()) return err(PT_ERR_INVALID_HANDLE, "pt_pose_apply_skin: unknown pose");
  Pose& ps = *pit->second;
  if (!ps.skinned) return err(PT_ERR_STATE, "pt_pose_apply_skin: the pose has no skin (pt_pose_set_skin)");
  if (!bones16) return err(PT_ERR_ARG, "pt_pose_apply_skin: null bones16");
  if (n_bones < 1 || n_bones > kPoseMaxObjects)
    return err(PT_ERR_ARG, "pt_pose_apply_skin: n_bones must be in [1, 4096]");
  if (n_bones <= ps.skin_max)
    return err(PT_ERR_ARG, "pt_pose_apply_skin: the skin names bone " + std::to_string(ps.skin_max) + ", n_bones is " +
                               std::to_string(n_bones));
  // the table: the 12 affine floats of each bone as three rows of four, permuted only (the bits are the caller's)
  static_assert(kSkinBoneFloats <= kPoseMatFloats, "the bone table lies in the pose's matrix table");
  auto fill = [&] {
    for (int k = 0; k < n_bones; ++k) {
      const float* m = bones16 + (size_t)k * 16;
      float* o = ps.mats_host + (size_t)k * kSkinBoneFloats;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) o[4 * r + c] = m[4 * c + r];
    }
    return (size_t)n_bones * kSkinBoneFloats;
  };
  auto place = [&](float* r_out, hipStream_t s) {
    int rc = skin_tris_launch(ps.tri_rest, ps.ntris, ps.sk_tri_bones, ps.sk_tri_weights, ps.mats_dev, n_bones,
                              ps.tri_posed, s);
    if (rc == 0 && ps.rtris)
      rc = skin_raster_launch(ps.r_rest, ps.rtris, ps.sk_r_bones, ps.sk_r_weights, ps.mats_dev, n_bones, r_out, s);
    return rc;
  };
  return pose_apply_with("pt_pose_apply_skin", ps, tri_out, node_out, raster_pass, motion, out_ms, fill, place);
}

int pt_debug_pose_raster(uint32_t pose, int which, float* host_out, size_t cap, size_t* n) {
  std::lock_guard<std::recursive_mutex> lk(g_mu);
  TRY(ensure_init());
  auto it = g.poses.find(pose);
  if (it == g.poses.end()) return err(PT_ERR_INVALID_HANDLE, "pt_debug_pose_raster: unknown pose");
  if (which < 0 || which > 1) return err(PT_ERR_ARG, "pt_debug_pose_raster: which 0 (current) or 1 (previous)");
  const Pose& ps = *it->second;
  const size_t floats = (size_t)ps.rtris * 18;
  if (n) *n = floats;
  if (!host_out || !floats) return PT_OK;
  if (cap < floats) return err(PT_ERR_ARG, "pt_debug_pose_raster: host_out is too small");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_out, ps.r_list[ps.cur ^ which], floats * sizeof(float), hipMemcpyDeviceToHost));
  return PT_OK;
}

}  // extern "C"

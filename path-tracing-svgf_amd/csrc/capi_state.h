// capi_state.h — the library state behind include/ptsvgf.h, shared by the translation units that implement it:
// capi.hip (init, textures, passes, uniforms, streams; it defines the state and the helpers declared here),
// capi_draw_pt.hip (the path tracer's draws, the scene cache, the point-light bins), capi_draw_svgf.hip (the G-buffer
// draw and the SVGF chain's, one function per pass kind), capi_geometry.hip (geometry that moves: builds, refits,
// raster binds, poses), capi_lights.hip (point lights that move), capi_environment.hip (the environment edited in place),
// capi_materials.hip (materials edited in place),
// capi_rays.hip (ray queries) and capi_static.hip (the static view: keys, caches, quiet-tile sets). The three kinds of
// edit in place share one type for the device versions they write (Versions) and, with the draws and the ray queries,
// one way to read a buffer another stream wrote (read_shared, note_reads). Internal: nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ptsvgf.h"
#include "pt_device.h"
#include "static_key.h"
#include "lights_key.h"

namespace ptapi {

struct LightVersions;
struct EnvVersions;

enum ProgKind { PK_PATHTRACE = 1, PK_REPROJECT, PK_VARIANCE, PK_ATROUS, PK_MODULATE, PK_BLIT, PK_SAVE, PK_OUTPUT, PK_TAA,
                PK_RASTER };

struct Texture {
  uint32_t target = PT_TEXTURE_2D;
  int W = 0, H = 0;      // logical (global) size
  int row0 = 0, rows = 0;  // stored rows (band)
  int layers = 0;
  bool owned = true;
  void* dev = nullptr;
  size_t bytes = 0;
  std::vector<uint8_t> host;  // buffers: host copy for decoding
  uint64_t version = 1;
  // the serial of the draw_raster that wrote this attachment last (Lib::raster_serial); 0 once anything else in the
  // library wrote the texture (tex_written): part of the G-buffer draw's key (static_key.h)
  uint64_t raster_stamp = 0;
  // the background stamp (static_key.h, DESIGN.md "Static view, part 3"): what this texture holds on background
  // tiles. With it, on a colour plane a one-sample wavefront draw wrote: the draw's primary content id and the pass
  // whose hit0 holds its primary hits (with the allocation's generation); on a depth-fwidth attachment draw_raster
  // wrote: the draw's G-buffer content id. tex_written clears the three and makes the stamp fresh.
  ptk::BgStamp bg;
  // the reason (ptsvgf_debug_background.h) of the bypassed SVGF draw that wrote this texture last, 0: none. The draws
  // further down the chain that read it are bypassed for the same reason, and say so.
  int bg_off = 0;
  uint64_t bg_prim = 0, bg_gbuf = 0;
  const void* bg_pass = nullptr;
  uint64_t bg_pass_gen = 0;
  // the first-hit record (static_key.h, DESIGN.md "Static view, part 4"): on an emission or albedo attachment a
  // qualifying one-sample wavefront draw wrote, the content id of that draw's FirstHitKey; 0: nothing is known.
  // tex_written clears it.
  uint64_t first_hit = 0;
  // compact one-float side plane of the stored rows: a depth-fwidth attachment's fwidth.y with the background flag, a
  // world-position attachment's primary-ray bound for rays from aux_eye (draw_raster)
  float* aux = nullptr;
  bool aux_valid = false;
  float aux_eye[3] = {0.0f, 0.0f, 0.0f};
  unsigned char* tflags = nullptr;  // a-trous per-tile surface flags derived from aux (atrous_tile_flags)
  size_t tflags_cap = 0;
  uint64_t tflags_ver = 0;          // texture version / rows they were derived for
  int tflags_y0 = 0, tflags_y1 = -1;
  bool lbvh = false;     // written by pt_bvh_build (the device copy is authoritative: get_scene decodes it there)
  // a node buffer pt_bvh_build wrote: the walk trees the device derived from it (owned; trees->version == version)
  ptk::LbvhTrees* trees = nullptr;
  // a node buffer pt_bvh_build wrote: what pt_bvh_refit needs (owned, held as trees is) and the pair it belongs to,
  // the triangle buffer's handle and both versions as the build (or the last refit) left them
  ptk::LbvhRefit* refit = nullptr;
  uint32_t refit_tri = 0;
  uint64_t refit_tri_ver = 0, refit_node_ver = 0;
  // pt_bvh_refit wrote dev in place; host is brought up to date by its readers (refresh_host)
  bool host_stale = false;
  // a lights buffer pt_lights_update has written (capi_lights.hip; owned): dev is then lights->sb.buf
  LightVersions* lights = nullptr;
  // an hdrMap or hdrCache texture pt_environment_update has written (capi_environment.hip): the pair's versions, held
  // by both textures and owned by the hdrMap; dev is then a plane of env->sb.buf
  EnvVersions* env = nullptr;
};

struct Uniform {
  int type = 0;  // 1 float 2 int 3 uint 4 bool 5 vec3 6 mat4
  float f[16] = {0};
  int i = 0;
  uint32_t u = 0;
};

struct RasterScene {
  float4* geom = nullptr;
  float4* nrm = nullptr;
  float4* disp = nullptr;  // pt_raster_pass_set_prev_vertices: displacement records beside nrm, or null
  float4* bvh = nullptr;
  int root_ref = 0;
  int stack_need = 0;
  int ntris = 0;
  // pt_raster_pass_bind_device: the encoded nodes of the bind and what refits them (pt_raster_pass_refit_device);
  // null after a host bind
  float* enc_nodes = nullptr;
  ptk::LbvhRefit* refit = nullptr;
  int bvh_records = 0;  // packed records bvh has room for (that bind's; >= 1 while refit is set)
  // moved on (raster_touch, from Lib::raster_ver: no two states of any pass share a value) by every entry point that
  // changes geom, nrm, disp, bvh or ntris: part of the G-buffer draw's key (static_key.h)
  uint64_t version = 0;
};

// Scratch of the tile-binned G-buffer (launch_gbuffer_raster), per rasterize pass, sized by its triangles and band.
struct RasterBins {
  void* base = nullptr;
  int ntris = 0, ntiles = 0, pair_cap = 0, big_cap = 0;
  int4* tri_box = nullptr;
  float* tri_tmin = nullptr;
  int *tile_count = nullptr, *tile_off = nullptr, *pairs = nullptr, *big = nullptr, *ctr = nullptr;
};

struct WFBuffers {
  void* base = nullptr;  // one allocation carved into the WFState arrays
  size_t n = 0;          // pixels per frame
  int nb = 1;            // frames (pt_pass_draw_batch): per-pixel arrays for nb * n pixels, lists and counters per frame
  ptk::WFState stb[ptk::kMaxBatch]{};  // frame b's state: per-pixel arrays at pid offset b * n; stb[0] == st
  ptk::WFState st{};
  float4* spp = nullptr;  // the sample planes of an spp draw: nsp planes of n texels (SppResolve::samples)
  int nsp = 0;
  uint64_t gen = 0;      // counts the allocations of base: part of the primary-hit cache's key (static_key.h)
  int* spill = nullptr;  // deep reference trees: stack entries past the LDS stack (WFState::spill)
  int spill_levels = 0;
  size_t spill_cols = 0;
};

// Cost-ordered tile dispatch state of one traversal pass (TileSched, pt_device.h).
struct TileOrder {
  uint32_t* cost = nullptr;  // per-tile cost recorded by the current launch
  int* perm = nullptr;       // dispatch order computed from the previous launch
  int n = 0;
  bool ordered = false;      // perm holds a valid order for n tiles
};

struct Pass {
  uint32_t program = 0;
  WFBuffers wf;
  TileOrder order;
  ptk::PrimaryCache pcache;  // path-tracing pass: the primary-hit cache (static_key.h, DESIGN.md "Static view")
  ptk::GbufCache gcache;     // rasterize pass: its last completed draw's key (reuse_static)
  ptk::PointCache lcache;    // path-tracing pass: the bounce-0 point-light verdict cache (DESIGN.md "Static view, part 2")
  int lcache_last_mode = 0;  // the PointCacheMode of the pass's last draw (pt_debug_point_cache_mode)
  uint32_t lcache_last_forgot = 0;  // the lights that draw's cache forgot first (pt_debug_point_cache_forgotten)
  // path-tracing pass: the bounce-0 shade's keep mode (DESIGN.md "Static view, part 4"). The busy-tile list of the
  // primary stage that ran last (ptk::launch_busy_tiles; busy_valid: built since that stage, busy_n: the tiles it was
  // sized and built for), and of the pass's last draw its FirstHitMode / FirstHitReason; the draws that kept.
  int* busy = nullptr;
  int busy_n = 0;
  bool busy_valid = false;
  int fh_mode = 0, fh_reason = 0;
  uint64_t fh_kept = 0;
  int W = 0, H = 0;
  std::vector<uint32_t> att;
  bool bound = false, final_pass = false;
  int slot = 0;
  std::unordered_map<std::string, uint32_t> tex;
  std::unordered_map<std::string, Uniform> uni;
  int y_begin = -1, y_end = -1;
  RasterScene raster;
  uint32_t raster_src = 0;  // pt_raster_pass_share: draw this rasterize pass's triangles and tree instead
  RasterBins bins;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  uint32_t* row_cost = nullptr;  // pt_pass_set_row_cost (not owned)
  uint8_t* sample_counts = nullptr;  // pt_pass_set_sample_counts (not owned)
  float2* sample_stats = nullptr;    // pt_pass_set_sample_stats (not owned)
  float4* sample_moments = nullptr;  // pt_pass_set_sample_moments (not owned)
  uint32_t* motion_max = nullptr;  // pt_pass_set_motion_bound (not owned)
  // an SVGF pass's last draw (ptsvgf_debug_background.h): BgMode, BgReason, the quiet-tile set it worked with and the
  // tile shape it skips by (0 .. 4: the a-trous steps, 5: 16 x 16 blocks)
  int bg_mode = 0, bg_reason = 0, bg_shape = 0;
  uint64_t bg_set = 0;
  unsigned long long* stats = nullptr;  // pt_pass_set_trace_stats (not owned)
  int stats_n = 0;                      // counters that buffer holds (pt_pass_set_trace_stats_n)
};

// A device buffer built on one draw's stream and read by the draws of every frame in flight on other streams (the
// merged environment, the point-light bins). A rebuild writes a buffer no draw still reads: the current one is retired
// with the event of the build that wrote it and its readers' events, and a retired buffer is taken again only once all
// of those have completed, else a new one is allocated. Every reader's stream waits for the build's event. No host
// wait anywhere, so a rebuild never blocks on the device (e.g. on RCCL receives in flight for peers); retired buffers
// are kept, never freed mid-run. Rebuilds are rare.
struct SharedBuf {
  void* buf = nullptr;
  size_t bytes = 0;
  hipEvent_t built = nullptr;              // recorded after the work that wrote buf, on the stream that ran it
  std::map<hipStream_t, hipEvent_t> uses;  // per draw stream: recorded after its latest draw that read buf
  struct Retired {
    void* buf;
    size_t bytes;
    hipEvent_t built;  // the build that wrote it (null: none was recorded)
    std::vector<hipEvent_t> readers;
  };
  std::vector<Retired> spare;

  // a buffer of at least `need` bytes that nothing in flight reads or writes, in place of the current one
  hipError_t renew(size_t need) {
    if (buf) {
      Retired r{buf, bytes, built, {}};
      for (auto& u : uses) r.readers.push_back(u.second);
      uses.clear();
      spare.push_back(std::move(r));
      buf = nullptr;
      bytes = 0;
      built = nullptr;
    }
    for (size_t i = 0; i < spare.size(); ++i) {
      Retired& r = spare[i];
      bool idle = r.bytes >= need && (!r.built || hipEventQuery(r.built) == hipSuccess);
      for (size_t j = 0; idle && j < r.readers.size(); ++j) idle = hipEventQuery(r.readers[j]) == hipSuccess;
      if (!idle) continue;
      buf = r.buf;
      bytes = r.bytes;
      built = r.built;  // completed: recorded again by mark_built
      for (hipEvent_t e : r.readers) (void)hipEventDestroy(e);
      spare.erase(spare.begin() + i);
      return hipSuccess;
    }
    const hipError_t e = hipMalloc(&buf, need);
    if (e != hipSuccess) buf = nullptr;
    else bytes = need;
    return e;
  }
  // after the work that wrote buf was issued on s
  hipError_t mark_built(hipStream_t s) {
    if (!built)
      if (const hipError_t e = hipEventCreateWithFlags(&built, hipEventDisableTiming)) return e;
    return hipEventRecord(built, s);
  }
  // before work on s reads buf (a no-op wait once the build has run)
  hipError_t wait_built(hipStream_t s) { return hipStreamWaitEvent(s, built, 0); }
  // after a draw on s that read buf was issued: a later renew knows when that draw no longer reads it
  hipError_t note_read(hipStream_t s) {
    if (!buf) return hipSuccess;
    hipEvent_t& e = uses[s];
    if (!e)
      if (const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming)) return rc;
    return hipEventRecord(e, s);
  }
  // s is released (pt_stream_release): its last read is waited for, so its event need not outlive the stream
  void forget(hipStream_t s) {
    auto u = uses.find(s);
    if (u == uses.end()) return;
    (void)hipEventSynchronize(u->second);
    (void)hipEventDestroy(u->second);
    uses.erase(u);
  }
  bool any() const { return buf || !spare.empty(); }
  // drops every buffer and event (the caller has synchronised the streams that read them)
  void free() {
    if (buf) (void)hipFree(buf);
    if (built) (void)hipEventDestroy(built);
    for (auto& u : uses) (void)hipEventDestroy(u.second);
    for (Retired& r : spare) {
      (void)hipFree(r.buf);
      if (r.built) (void)hipEventDestroy(r.built);
      for (hipEvent_t e : r.readers) (void)hipEventDestroy(e);
    }
    *this = SharedBuf{};
  }
};

// The versions of a device buffer that an update call edits while draws are in flight on other streams (DESIGN.md
// "Moving point lights" describes the protocol once): a lights buffer (pt_lights_update), a scene's tri_shade records
// (pt_materials_update), an (hdrMap, hdrCache) pair (pt_environment_update). An update never writes memory a queued
// draw may read: it takes a version that nothing in flight reads (next), fills it on a stream of the owner's own
// (stream; host data through the version's pinned buffer, stage), records sb.mark_built there and makes the version
// what the owner points at. Every launch that reads it waits for that event and notes its read (read_shared,
// note_reads). The buffer the owner held before the first update is read by draws that noted nothing, so that update
// sets it aside for good (`first`): it is freed with the versions. No host wait anywhere.
struct Versions {
  SharedBuf sb;
  void* first = nullptr;
  hipStream_t upload = nullptr;    // the updates' stream (non-blocking), where the owner keeps one of its own
  std::map<void*, void*> staging;  // per device version: its pinned host buffer (free again when the version is)

  bool edited() const { return first != nullptr; }  // an update has written a version: readers wait and note
  // a version of at least `need` bytes that nothing in flight reads, in sb.buf; `cur`: the buffer the owner holds now.
  // A failure of the first call changes nothing; a later one has retired the current version (sb.buf is null), which
  // stays valid to read until a later call hands it out.
  hipError_t next(void* cur, size_t need) {
    if (first) return sb.renew(need);
    void* nb = nullptr;
    if (const hipError_t e = hipMalloc(&nb, need)) return e;
    first = cur;
    sb.buf = nb;
    sb.bytes = need;
    return hipSuccess;
  }
  // the pinned host buffer of the current version, `bytes` long (the same for every call); null: out of memory
  void* stage(size_t bytes) {
    void*& s = staging[sb.buf];
    if (!s && hipHostMalloc(&s, bytes, hipHostMallocDefault) != hipSuccess) s = nullptr;
    return s;
  }
  hipStream_t stream() {  // null: it could not be created
    if (!upload && hipStreamCreateWithFlags(&upload, hipStreamNonBlocking) != hipSuccess) upload = nullptr;
    return upload;
  }
  int count() const { return (int)sb.spare.size() + (sb.buf ? 1 : 0) + (first ? 1 : 0); }  // device buffers held
  // the set-aside buffer, given back to its owner (free_environment), which frees it
  void* take_first() { return std::exchange(first, nullptr); }
  // drops every buffer, the events and the stream (the caller has synchronised the device)
  void free() {
    sb.free();
    if (first) (void)hipFree(first);
    for (auto& s : staging) (void)hipHostFree(s.second);
    if (upload) (void)hipStreamDestroy(upload);
    *this = Versions{};
  }
};

// The versions of a lights texture buffer that pt_lights_update changes: whole copies of the host copy. The current
// one is Texture::dev; `first` is the buffer pt_texbuffer_create made.
struct LightVersions : Versions {
  std::vector<uint64_t> pos_stamp;  // per light: the Texture::version at which its position last changed bitwise
};

// The versions of an (hdrMap, hdrCache) pair that pt_environment_update changes (DESIGN.md "Environment edits"). One
// version is one buffer of three float4 planes of W x H texels: the hdr texels, the cache texels and the merged plane
// (hdr.xyz, cache.z); its first two planes are the textures' dev. The buffers pt_texture2d_create made are set aside
// as `first` (the hdrMap's) and first_cache.
struct EnvVersions : Versions {
  uint32_t hdr_handle = 0, cache_handle = 0;
  int W = 0, H = 0;
  void* first_cache = nullptr;
  hipEvent_t src_done = nullptr;   // a device source: its expansion on the current stream, which the build waits for
  float* scratch = nullptr;        // lum / pdf and the conditional CDFs (W x H each), both marginals (W each), the total
  // the textures' versions as the last update left them: while they stand, the version's merged plane is the pair's
  uint64_t vh = 0, vc = 0;
  size_t plane() const { return (size_t)W * H * sizeof(float4); }
};

// What the draw or ray query being issued reads of the shared buffers (read_shared), noted on its stream after a
// successful launch (note_reads). Local to the call, which holds g_mu throughout.
struct DrawReads {
  // at most: the shade records, the lights, two environment pairs, the merged environment, the point-light bins
  SharedBuf* bufs[6] = {};
  int n = 0;
  const uint64_t* light_stamps = nullptr;  // the bound lights' per-light position stamps (null: never updated, all 0)
  int light_count = 0;
  // the pointLights texture the draw bound (0: none): part of the verdict cache's key (static_key.h)
  uint32_t light_handle = 0;
  uint64_t light_ver = 0;
  // the hdrMap and hdrCache textures the draw bound: part of the miss-colour key (static_key.h)
  uint32_t hdr_handle = 0, cache_handle = 0;
  uint64_t hdr_ver = 0, cache_ver = 0;
};

// The point-light triangle bins of a scene (ptk::PointBinsDev, kernels_pointbins.hip) for the lights texture a
// path-tracing draw bound: built on the device by the first such draw, rebuilt when the scene's triangles or tree, the
// lights texture (handle, device memory, version), pointLightSize, R or the binning (point_bins_tight) change. Read
// by the path tracers of every frame in flight on other streams: a SharedBuf.
struct PointBinsGPU {
  SharedBuf sb;
  ptk::PointBinsDev dev{};
  uint64_t tri_ver = 0, node_ver = 0, light_ver = 0;
  uint32_t light_handle = 0;
  const void* light_dev = nullptr;
  int nl = 0, R = 0, ntris = 0, tight = 0;
  // per light: the position stamp its lists were built for, and how long a moved light has stood (lights_key.h)
  ptk::LightBinsState per_light[ptk::kPointBins];
};

struct SceneGPU {
  PointBinsGPU pbins;
  float4* geom = nullptr;
  // the tri_shade records, in shade.sb.buf: the decode's buffer, then the versions pt_materials_update writes
  // (capi_materials.hip, DESIGN.md "Material edits"; freed with the scene or at the next decode). Draws wait for and
  // note them once edited(). shade.sb.built after a device decode: that decode's event, which the first update's
  // kernel waits for.
  Versions shade;
  // bumped per update, never reset: with tri_ver in the first-hit key (a retired version taken again has the same
  // pointer and other contents)
  uint64_t shade_ver = 0;
  float4* bvh = nullptr;
  float4* bvh4 = nullptr;
  float4* bvh_any = nullptr;  // any-hit tree over the reference leaves (build_anyhit_tree)
  float4* leaves = nullptr;   // the reference leaves: (box lo, leaf ref bits), (box hi, 0) (wf_primary_raster)
  int nleaves = 0;
  int* tri_leaf = nullptr;    // per triangle: its reference leaf's index in `leaves` (wf_primary_tri); always owned
  int tri_leaf_cap = 0;       // triangles tri_leaf has room for
  bool tri_shared = false;    // host-built trees: some triangle lies in two leaves (upload_leaves)
  int root_any = 0, need_any = 0;
  bool has4 = false;  // bvh4: the 4-wide form of bvh_any (pack_wide)
  bool nan4 = false;  // a child box of bvh4 has a NaN coordinate (PT_WIDE_SIGNED walks need lo <= hi: not walked)
  // a scene pt_bvh_build wrote: bvh (== bvh_any), bvh4 and leaves belong to the node texture's LbvhTrees, not to this
  bool lbvh = false;
  int root4 = 0, need4 = 0, root4c = 0;  // root4c: the closest-hit walks' root (SceneDev::root4c)
  // refine_leaves' fine boxes are padded for rays whose origin lies within kFineEyeReach x the scene's largest vertex
  // coordinate; an eye further out (pt_params) walks the reference tree instead
  float fine_eye_limit = INFINITY;
  int stack_need = 0;
  int root_ref = 0;
  int ntris = 0;
  uint64_t tri_ver = 0, node_ver = 0;
};

// The environment map with its importance cache's pdf channel beside it (PTParams::hdr_pdf): built on the device
// when a path-tracing draw binds an hdrMap and an hdrCache of one size, rebuilt when either changes (versions), freed
// with either texture. Read by the path tracers of every frame in flight on other streams: a SharedBuf of float4.
struct HdrMerged {
  SharedBuf sb;
  const void *hdr_dev = nullptr, *cache_dev = nullptr;
  uint64_t vh = 0, vc = 0;
  int W = 0, H = 0;
};

// Posed objects (pt_pose_create): the rest-pose lists on the device and what pt_pose_apply writes from them
struct Pose {
  int ntris = 0;               // Triangle_encoded records
  float* tri_rest = nullptr;   // in the order of the build's tri_in
  float* tri_posed = nullptr;  // staging: the posed list, pt_bvh_refit's tri_in
  int rtris = 0;               // raster triangles (0: the pose serves the path tracer only)
  float* r_rest = nullptr;
  int* r_obj = nullptr;        // one object per raster triangle
  float* r_list[2] = {nullptr, nullptr};  // posed raster lists; r_list[cur] is what the pass holds
  int cur = 0;
  float* mats_dev = nullptr;   // kPoseMaxObjects x kPoseMatFloats
  float* mats_host = nullptr;  // pinned staging of the same size
  float4* disp_spare = nullptr;  // displacement records taken off the pass by a pose without motion, for the next
  // the skin (pt_pose_set_skin): four bones and four weights per corner, three corners per record / raster triangle
  bool skinned = false;
  int skin_max = 0;  // the largest bone index the skin names
  uint16_t *sk_tri_bones = nullptr, *sk_r_bones = nullptr;
  float *sk_tri_weights = nullptr, *sk_r_weights = nullptr;
};

// A quiet-tile set (static_key.h): per tile of the five a-trous tile shapes (atrous_flag_offset's layout over the whole
// frame) and per 16 x 16 block, one byte that is 0 iff every pixel of the tile is background in the G-buffer and a miss
// in the primary plane; then six counts of the non-zero bytes per shape. Read-only once built.
struct QuietSet {
  uint64_t id = 0, gbuf = 0;  // the set's id and the G-buffer content it was built for
  int W = 0, H = 0;
  unsigned char* flags = nullptr;
  size_t cap = 0, off16 = 0, off_counts = 0;
  hipStream_t last_stream = nullptr;  // the stream of the draws that read it, mixed: more than one
  bool mixed = false;
};
constexpr int kQuietSets = 4;

// Content ids by key (static_key.h): equal keys, one id. A small table, oldest out: a key that comes back after it
// left gets a new id, which only costs the skips of a frame.
struct ContentIds {
  std::vector<std::pair<std::vector<uint64_t>, uint64_t>> known;
  uint64_t of(const uint64_t* w, int n, uint64_t* serial) {
    for (size_t i = 0; i < known.size(); ++i)
      if ((int)known[i].first.size() == n && memcmp(known[i].first.data(), w, n * sizeof(uint64_t)) == 0) {
        if (i + 1 != known.size()) std::rotate(known.begin() + i, known.begin() + i + 1, known.end());
        return known.back().second;
      }
    if (known.size() >= 8) known.erase(known.begin());
    known.emplace_back(std::vector<uint64_t>(w, w + n), ++*serial);
    return known.back().second;
  }
};

struct Lib {
  bool init = false;
  int device = 0;
  hipStream_t own = nullptr, stream = nullptr;
  uint32_t next = 1;
  std::map<uint32_t, int> programs;
  std::map<uint32_t, std::unique_ptr<Texture>> textures;
  std::map<uint32_t, std::unique_ptr<Pass>> passes;
  std::map<uint32_t, std::unique_ptr<Pose>> poses;
  std::map<std::pair<uint32_t, uint32_t>, SceneGPU> scenes;
  std::map<std::pair<uint32_t, uint32_t>, HdrMerged> hdr_merged;  // keyed by (hdrMap, hdrCache) handles
  std::map<hipStream_t, ptk::WfFork> forks;  // per draw stream: the path tracer's side stream (uniform trace_fork)
  uint32_t unit0 = 0;  // GL texture unit 0 binding (global)
  int band_w = 0, band_h = 0, band_y0 = 0, band_y1 = 0, band_row0 = 0, band_rows = 0;
  bool profiling = false;
  uint64_t raster_serial = 0;  // draw_raster calls that launched (Texture::raster_stamp)
  uint64_t raster_ver = 0;     // RasterScene::version values handed out
  // the static background (DESIGN.md "Static view, part 3"): the counter of content and quiet-set ids, the ids of the
  // keys, the reproject draws' choice of a set, and the sets (the newest kQuietSets)
  uint64_t bg_serial = 0;
  ContentIds bg_miss, bg_prim, bg_gbuf;
  ContentIds bg_first;  // of FirstHitKeys (Texture::first_hit)
  ptk::QuietChoice bg_choice;
  QuietSet bg_sets[kQuietSets];
  int bg_next = 0;
};

// defined in capi.hip
extern Lib g;
// an entry point changes (or may have half changed) the pass's raster triangles, tree or displacement records
inline void raster_touch(Pass* p) { p->raster.version = ++g.raster_ver; }
extern std::recursive_mutex g_mu;
extern ptk::LbvhWork g_lbvh;  // GPU BVH builder scratch (grows, reused across rebuilds)

int err(int code, const std::string& m);  // sets the calling thread's pt_last_error text
int hip_err(hipError_t e, const char* what);
#define HIPCHK(x)                                    \
  do {                                               \
    hipError_t e_ = (x);                             \
    if (e_ != hipSuccess) return hip_err(e_, #x);    \
  } while (0)
#define TRY(x)                    \
  do {                            \
    int rc_ = (x);                \
    if (rc_ != PT_OK) return rc_; \
  } while (0)

// the launch being issued on g.stream reads sb.buf: after the work that wrote it; noted after the launch (note_reads)
inline int read_shared(DrawReads& r, SharedBuf& sb) {
  HIPCHK(sb.wait_built(g.stream));
  r.bufs[r.n++] = &sb;
  return PT_OK;
}
// after the launch: its stream's use events on the shared buffers it read (SharedBuf::note_read)
inline int note_reads(const DrawReads& r) {
  for (int i = 0; i < r.n; ++i) HIPCHK(r.bufs[i]->note_read(g.stream));
  return PT_OK;
}

Texture* tex_of(uint32_t h);
Pass* pass_of(uint32_t h);
// the library wrote (or is about to write) new texels into t: its version moves on, its compact plane and its
// G-buffer stamp no longer describe it
inline void tex_written(Texture* t) {
  t->version++;
  t->aux_valid = false;
  t->raster_stamp = 0;
  t->bg = ptk::bg_fresh(&g.bg_serial);
  t->bg_prim = t->bg_gbuf = 0;
  t->bg_pass = nullptr;
  t->bg_off = 0;
  t->first_hit = 0;
}
int ensure_init();
int refresh_host(Texture* t);
// a pass's bindings: a uniform of `type` (null: not set as one), an int / float / uint uniform or `def`, a sampler by
// name (texture unit 0 when unbound; bound_sampler: null when unbound), the rows its draws cover; whether pt_set_band
// holds a partition of W x H frames
const Uniform* U(Pass* p, const char* name, int type);
int ui(Pass* p, const char* n, int def);
float uf(Pass* p, const char* n, float def);
uint32_t uu(Pass* p, const char* n, uint32_t def);
Texture* sampler(Pass* p, const char* name, uint32_t* handle = nullptr);
Texture* bound_sampler(Pass* p, const char* name);
void rows_of(Pass* p, int* y0, int* y1);
bool band_partition(int W, int H);
// the plane of a 2-D texture of the pass's size (`what` names it in the error text); of the pass's k-th colour
// attachment, which the draw is about to write (tex_written)
int plane_of(Texture* t, Pass* p, ptk::Plane* out, const char* what);
int att_plane(Pass* p, int k, ptk::Plane* out);
// drops a merged environment; forgets the trees a GPU-built scene borrowed from its node texture
void free_hdr_merged(HdrMerged& m);
void drop_borrowed(SceneGPU& sg);

// ---- defined in capi_draw_pt.hip: the path tracer's draws (pt_pass_draw, pt_pass_draw_batch), and the tile
// rasterisers' scratch and the cost-ordered tile dispatch, which the G-buffer draw uses too
int draw_pathtrace(Pass* p);
int draw_pathtrace_batch(Pass** ps, int n);
int bins_for(RasterBins& b, int n, int W, int y0, int y1, int cap, ptk::Bins* out);
int tile_order_begin(Pass* p, int ntiles, ptk::TileSched* out);
int tile_order_finish(Pass* p, const ptk::TileSched& t);

// ---- defined in capi_draw_svgf.hip: the G-buffer draw and the SVGF chain's draws (pt_pass_draw); the a-trous tile
// flags of a G-buffer draw or adoption (pt_raster_pass_adopt)
int draw_raster(Pass* p);
int draw_svgf(Pass* p, int kind);
int gbuf_flags(Pass* p, Texture* fwt, ptk::GBufParams& k);

// ---- defined in capi_static.hip: the static view (DESIGN.md "Static view"), as the draws use it
ptk::PrimaryKey primary_key(const Pass* p, const ptk::PTParams& k, const SceneGPU* sg, int pair_cap);
bool gbuf_key(Pass* p, const Pass* src, ptk::GbufKey* out);
bool reuse_static_on(Pass* p);
void primary_cache_note(Pass* p, const ptk::PrimaryKey& key, bool reused, bool ok);
// One one-sample wavefront draw's use of the primary-hit cache, the verdict cache and the keep mode, in three steps.
struct StaticView {
  ptk::BgStamp colour;  // before(): what the attachments say as the draw finds them
  uint64_t emission = 0, albedo = 0;
  ptk::PrimaryKey key;  // pt_wf_setup: the draw's key, and whether it reads the cached primary hit
  bool reuse = false, forgets = false;
  ptk::LightsKey lkey;  // setup(): the verdict cache's key; `forgets`: its plane first forgets the lights of `forget`
  uint32_t forget = 0;
  uint64_t first = 0;   // setup(): the content id of the draw's FirstHitKey
  void before(Pass* p);  // before pt_params, whose att_plane renews the attachments' stamps
  // after pt_wf_setup: the verdict cache's mode into k.point_cache, the keep mode and with it k.busy
  int setup(Pass* p, ptk::PTParams& k, const SceneGPU* sg, const DrawReads& reads);
  void finish(Pass* p, const ptk::PTParams& k, const DrawReads& reads, int rc);  // after the launch (rc 0: it succeeded)
};
// A path-tracing draw that uses none of it (sampled, batched, the megakernel's): the verdict cache is stale, the keep
// mode off for `reason` (a FirstHitReason), and the primary-hit cache stale too unless the draw serves it
void static_view_off(Pass* p, int reason, bool keep_primary);
// One SVGF draw's decision. Before the draw's att_plane calls pair() reads the stamps as the draw finds them; need()
// states what the draw requires, decide() whether it may skip its tiles; finish() stamps the outputs after the launch.
struct BgDraw {
  int reason = 0;  // PT_BG_R_NONE
  uint64_t set = 0;
  QuietSet* qs = nullptr;
  bool skip = false;
  int npairs = 0;
  Texture* out[2] = {nullptr, nullptr};
  ptk::BgStamp in[2], was[2];
  bool mod[2] = {false, false};
  int in_off = 0;  // an input was written by a bypassed draw of the chain: its reason
  void pair(const Texture* i, Texture* o, bool modulated);
  void need(bool cond, int r) { if (!reason && !cond) reason = r; }  // the first unmet condition is the reason
  void decide();
  void finish(Pass* p, int shape, bool ok);
};
int bg_bypass(Pass* p, int y0, int y1);
bool bg_whole(const Texture* t, int H);
bool bg_one_gbuffer(const Texture* nd, const Texture* ft);
uint64_t bg_set_from_input(const Texture* in, const Texture* ft, int W, int H);
int bg_build_set(uint64_t id, const Texture* ct, const Texture* ft, int W, int H, bool* built);

// defined in capi_geometry.hip: what pt_shutdown and the destroy calls release of a texture, a pass, a pose
void free_trees(Texture* t);
void free_refit(Texture* t);
void free_raster_refit(RasterScene& r);
void free_pose(Pose& p);
// defined in capi_lights.hip: the versions of an updated lights buffer, the current one (t->dev) included
void free_lights(Texture* t);
// defined in capi_environment.hip: the versions of an updated (hdrMap, hdrCache) pair, given either texture. Both
// textures are left with a buffer of their own that holds what they held (nothing in flight reads them afterwards:
// it synchronises)
void free_environment(Texture* t);
// defined in capi_materials.hip (DESIGN.md "Material edits"). free_shade: every version of a scene's tri_shade records
// (the caller holds no draw in flight that reads them, or they are all the decode's: it synchronises when versions
// exist). materials_order: work issued on s after this call runs after every pt_materials_update issued so far, whose
// kernels patch the triangle texels and a pose's rest list in place on a stream of their own; called by whatever reads
// or overwrites those on the device. free_materials: the update stream and its staging (pt_shutdown).
void free_shade(SceneGPU& sg);
int materials_order(hipStream_t s);
void free_materials();
// defined in capi_rays.hip: the ray queries' spill scratch (pt_shutdown)
void free_rays();
// defined in capi_draw_pt.hip: the decoded scene of a (triangles, nodes) pair of texture buffers, as the path-tracing
// draws get it (decoded on first use and again when either buffer's version moved on); the scene errors are the draws'
int scene_of(Texture* tris, uint32_t th, Texture* nodes, uint32_t nh, SceneGPU** out);

// (T: the device type, or the host tree builder's Float4 for float4)
template <class T, class D>
int upload_vec(const std::vector<T>& v, D** dst) {
  static_assert(sizeof(T) == sizeof(D), "upload_vec copies records as they are");
  if (*dst) { (void)hipFree(*dst); *dst = nullptr; }
  if (v.empty()) return PT_OK;
  HIPCHK(hipMalloc((void**)dst, v.size() * sizeof(T)));
  HIPCHK(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return PT_OK;
}

}  // namespace ptapi

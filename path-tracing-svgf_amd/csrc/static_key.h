// static_key.h — the key of everything the path tracer's primary stage reads (DESIGN.md "Static view"). A pass keeps
// the key of the last stage it ran; a draw whose key equals it reads the primary hit plane that stage wrote
// (WFState::hit0) instead of running the stage again. Plain host C++ with no HIP type, so the CPU suite reaches the
// compare through pt_debug_static_key_diff.
//
// A key is one 64-bit word per field: a pointer's address, an integer, or a float's bit pattern (so a NaN equals
// itself, and -0 differs from +0, which costs one stage and is never wrong). The compare walks the words, so a field
// cannot be left out of it (every kind of key below goes through the one loop, key_words_diff); a new input of the
// stage is a new enumerator here and a line in capi_static.hip's primary_key().
#pragma once
#include <stdint.h>
#include <string.h>

#include <initializer_list>

namespace ptk {

enum PrimaryKeyField {
  kPkEye0, kPkEye1, kPkEye2,          // uniform eye
  kPkCamRot0,                         // uniform cameraRotate, 16 floats
  kPkW = kPkCamRot0 + 16, kPkH,       // the pass's frame size
  kPkY0, kPkY1,                       // the rows drawn (pt_pass_set_rows, or the band's)
  kPkBandW, kPkBandH, kPkBandY0, kPkBandY1, kPkBandRow0, kPkBandRows,  // pt_set_band
  kPkTileStride, kPkTileOffset, kPkAspectCorrected,
  kPkPrune, kPkClosestTree, kPkPrimaryRaster,  // as the draw uses them (pt_params, pt_wf_setup), not as set
  kPkScene, kPkTriVer, kPkNodeVer, kPkNtris,   // the SceneGPU and the texture versions it was decoded from
  kPkTriGeom, kPkBvh, kPkRootRef, kPkBvhAny, kPkRootAny, kPkBvh4, kPkRoot4, kPkRoot4c,  // what pt_params bound
  kPkLeaves, kPkNleaves, kPkTriLeaf,
  kPkStackNeed, kPkSpill,             // which instantiation walks (stack size, deep tree)
  kPkPairCap,                         // uniform raster_pair_cap
  kPkPlane, kPkPlaneGen,              // hit0 of this draw and the generation of the allocation it lies in (wf_alloc)
  kPkTileCost, kPkTilePerm,           // the tile order the bounce-0 shade reads: present or not, and where
  kPkWords
};

struct PrimaryKey {
  uint64_t w[kPkWords];
};

inline uint64_t key_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof(u));
  return u;
}
inline uint64_t key_bits(const void* p) { return (uint64_t)(uintptr_t)p; }
inline uint64_t key_bits(int v) { return (uint64_t)(int64_t)v; }

// The compare of every kind of key: the first of the n words in which a and b differ, -1 when they are equal. The
// fields of `skip` are not compared.
inline int key_words_diff(const uint64_t* a, const uint64_t* b, int n, std::initializer_list<int> skip = {}) {
  for (int i = 0; i < n; ++i) {
    bool differs = a[i] != b[i];
    for (int s : skip) differs = differs && s != i;
    if (differs) return i;
  }
  return -1;
}
// the first field in which two keys of one kind differ, -1 when they are equal
template <class K>
inline int key_diff(const K& a, const K& b, std::initializer_list<int> skip = {}) {
  return key_words_diff(a.w, b.w, (int)(sizeof(a.w) / sizeof(a.w[0])), skip);
}
// a key from the words of one (the C ABI's form of a key)
template <class K>
inline K key_from(const uint64_t* w) {
  K k;
  memcpy(k.w, w, sizeof(k.w));
  return k;
}
// a composite key (LightsKey, MissKey, FirstHitKey: their *Primary0 is word 0) with `head` in front, the rest 0
template <class K>
inline K key_headed(const PrimaryKey& head) {
  K k{};
  memcpy(k.w, head.w, sizeof(head.w));
  return k;
}

// The primary-hit cache of a path-tracing pass: the key of the last stage that ran, whether hit0 still holds that
// stage's result, and the counts of draws that ran the stage / reused it (pt_debug_stage_counts).
struct PrimaryCache {
  PrimaryKey key{};
  bool valid = false;
  uint64_t runs = 0, reuses = 0;
};

// May this draw skip the stage? `bypass`: trace statistics or a row-cost buffer are bound (the stage's counters must
// stay what they are), or the uniform primary_cache is 0.
inline bool primary_cache_hit(const PrimaryCache& c, const PrimaryKey& now, bool bypass) {
  return !bypass && c.valid && key_diff(c.key, now) < 0;
}

// ------------------------------------------- the bounce-0 point-light verdicts ---
// The key of the verdict cache (point_cache.h, DESIGN.md "Static view, part 2"): a verdict is a function of the
// pixel's first hit point, which the primary key covers, and of what the bounce-0 shadow ray reads beyond it.
enum LightsKeyField {
  kLkPrimary0,                             // the draw's whole PrimaryKey
  kLkLightHandle = kLkPrimary0 + kPkWords, // the pointLights texture: handle, device pointer, Texture::version
  kLkLightDev, kLkLightVer,
  kLkPointLightSize, kLkNlightsBuf,        // which light a pixel picks, and which indices read a light at all
  kLkPointBins, kLkPointBinsDev,           // who decides the ray (the lights' triangle bins or the walk), and the bins
  kLkPlane,                                // WFState::pcache of this draw (kPkPlaneGen covers the allocation)
  kLkWords
};

struct LightsKey {
  uint64_t w[kLkWords];
};

// The verdict cache of a path-tracing pass: the key of the draw that reset the plane, and whether the plane still
// holds verdicts of that key (false: stale).
struct PointCache {
  LightsKey key{};
  bool valid = false;
};

// The mode of a draw (PointCacheMode: 0 off, 1 reset, 2 use). stage_reused: the draw reads the cached primary hit
// (primary_cache_hit). bypass: point_cache = 0, trace statistics or a row-cost buffer bound, pointLightSize outside
// 1 .. 4, a deep tree, shade_fold = 0 or max_tracing_depth = 0 (no folded shade runs). A draw that runs the primary
// stage, or a bypassed one, is off and leaves the plane stale (point_cache_note); the first draw that reuses the stage with the plane stale, or under another key, resets it;
// a later draw under the reset draw's key uses it. A moving camera therefore never touches the plane.
inline int point_cache_mode(const PointCache& c, const LightsKey& now, bool stage_reused, bool bypass) {
  if (bypass || !stage_reused) return 0;
  return c.valid && key_diff(c.key, now) < 0 ? 2 : 1;
}
// after the draw's launch (ok: it succeeded)
inline void point_cache_note(PointCache& c, const LightsKey& now, int mode, bool ok) {
  if (mode == 0 || !ok) {
    c.valid = false;
  } else if (mode == 1) {
    c.key = now;
    c.valid = true;
  }
}

// ---------------------------------------------------------------- the G-buffer draw ---
// The key of a rasterize pass's draw (draw_raster): everything the draw reads, and the state of everything it writes
// as its last completed draw left it. With the pass's int uniform reuse_static set (the caller's statement that nothing
// outside the library writes the attachments between this pass's draws) a draw whose key equals the last completed
// draw's launches nothing: the attachments, both compact planes and the tile flags already hold its result.
enum GbufKeyField {
  kGkW, kGkH, kGkY0, kGkY1,
  kGkBandW, kGkBandH, kGkBandY0, kGkBandY1, kGkBandRow0, kGkBandRows,
  // per attachment (world, normal/depth, motion, fwidth): handle, device pointer, Texture::version, and the serial of
  // the draw_raster that wrote it last (0 once anything else in the library wrote it)
  kGkAtt0,
  kGkFwAux = kGkAtt0 + 4 * 4, kGkFwAuxValid,  // the fwidth attachment's compact plane
  kGkBoundAux, kGkBoundAuxValid,              // the world attachment's compact plane (the primary rays' bound)
  kGkAuxEye0, kGkAuxEye1, kGkAuxEye2,         // and the eye it was formed for
  kGkBoundEyeSet, kGkBoundEye0, kGkBoundEye1, kGkBoundEye2,  // uniform bound_eye: present, value
  kGkView0,
  kGkProj0 = kGkView0 + 16,
  kGkPreViewProj0 = kGkProj0 + 16,
  kGkDisp = kGkPreViewProj0 + 16,             // the displacement records the draw reads (null: object_motion 0, or none)
  kGkMode, kGkPairCap,                        // gbuffer_mode, raster_pair_cap
  kGkTileFlags, kGkTfRows0, kGkTfRows1,       // atrous_tile_flags, atrous_rows_begin / _end as set
  kGkTflags, kGkTflagsCap, kGkTflagsVer, kGkTflagsY0, kGkTflagsY1,  // the flags' allocation and what they were derived for
  kGkSource, kGkSceneVer,                     // raster_src (0: the pass's own triangles) and RasterScene::version
  kGkWords
};

struct GbufKey {
  uint64_t w[kGkWords];
};

struct GbufCache {
  GbufKey key{};
  bool valid = false;  // key is that of a completed draw
  uint64_t runs = 0, reuses = 0;
};

// May this draw be elided? enabled: reuse_static is set (and PTSVGF_STATIC_REUSE does not force it off) and no motion
// bound is bound (it is cleared and reduced per draw). Every compact plane the draw writes must be present and valid:
// the fwidth attachment's always, the world attachment's bound plane when bound_eye is set (without it a draw leaves
// that plane invalid, and so does an elided one).
inline bool gbuf_cache_hit(const GbufCache& c, const GbufKey& now, bool enabled) {
  const bool planes = now.w[kGkFwAux] && now.w[kGkFwAuxValid] &&
                      (!now.w[kGkBoundEyeSet] || (now.w[kGkBoundAux] && now.w[kGkBoundAuxValid]));
  return enabled && c.valid && planes && key_diff(c.key, now) < 0;
}

// ------------------------------------------------ the static background of the SVGF chain ---
// DESIGN.md "Static view, part 3". On a background pixel every SVGF pass copies a texel, so on a standing view a draw
// stores what its destination already holds. A draw skips a tile only where that is proven, from three facts kept on
// the host: which tiles are all background (a quiet-tile set, built on the device once per view), what the source
// holds there (a content id), and that the destination holds the same content there (its stamp).

// The content of a key, as opposed to where the draw that used it put its results: the fields that name a plane, an
// allocation or scratch are cleared, so the K slots' draws of one view have one content.
inline PrimaryKey primary_content(const PrimaryKey& k) {
  PrimaryKey c = k;
  c.w[kPkSpill] = k.w[kPkSpill] != 0;  // (which instantiation walks, not where its spill columns lie)
  c.w[kPkPlane] = c.w[kPkPlaneGen] = c.w[kPkTileCost] = c.w[kPkTilePerm] = 0;
  return c;
}
// `source`: the identity of the pass whose triangles the draw reads (its own, or the one it shares); kGkSceneVer is
// already that pass's. The attachments, their compact planes and the tile flags are where, not what.
inline GbufKey gbuf_content(const GbufKey& k, uint64_t source) {
  GbufKey c = k;
  for (int i = kGkAtt0; i < kGkFwAux; ++i) c.w[i] = 0;
  c.w[kGkFwAux] = c.w[kGkBoundAux] = c.w[kGkBoundAuxValid] = 0;
  c.w[kGkAuxEye0] = c.w[kGkAuxEye1] = c.w[kGkAuxEye2] = 0;
  c.w[kGkTflags] = c.w[kGkTflagsCap] = c.w[kGkTflagsVer] = c.w[kGkTflagsY0] = c.w[kGkTflagsY1] = 0;
  c.w[kGkSource] = source;
  return c;
}

// The key of a miss pixel's colour texel: everything the path tracer reads on the way from the pixel to the texel when
// the primary ray hits nothing (shade_body's miss branch, terminal_write / wf_finalize; DESIGN.md has the table).
// frameCounter is not in it: a miss draws no random number that reaches the texel, and the only other read of it, the
// accumulation's mix, makes the draw no static-background draw at all (kMkAccumulate must be 0 for a content id).
enum MissKeyField {
  kMkPrimary0,                          // primary_content() of the draw's PrimaryKey: the ray, and which pixels miss
  kMkHdrHandle = kMkPrimary0 + kPkWords,  // hdrMap: handle, device pointer, Texture::version, size
  kMkHdrDev, kMkHdrVer, kMkHdrW, kMkHdrH,
  kMkCacheHandle, kMkCacheDev, kMkCacheVer,  // hdrCache: the merged texture the fetch reads is built from both
  kMkMerged,                            // whether the fetch reads the merged texture (hdr_merge and its conditions)
  kMkClamp,                             // uniform clamp_threshold
  kMkAccumulate,                        // uniform accumulate
  kMkMaxDepth, kMkShadeFold,            // which kernels write the texel (folded shade, or wf_finalize)
  kMkSpp,                               // samples per pixel (a resolve averages them)
  kMkWords
};
struct MissKey {
  uint64_t w[kMkWords];
};

// A texture's background stamp: "on the tiles of `scope` this texture holds content `id`". An id names a content, not
// a texture: the miss colour of a MissKey, or whatever some texture held when something other than an SVGF copy wrote
// it last (a fresh id: it equals nothing but its own copies). Ids and quiet-set ids come from one counter, so 0 is
// never one. Bit 63 tags the modulate's form of a content, (c.xyz, 1).
constexpr uint64_t kBgWhole = 0;             // scope: the whole texture
constexpr uint64_t kBgModulated = 1ull << 63;
struct BgStamp {
  uint64_t id = 0, scope = kBgWhole;  // id 0: nothing is known
};
// rule 1: any writer but an SVGF copy leaves a content of its own
inline BgStamp bg_fresh(uint64_t* serial) { return BgStamp{++*serial, kBgWhole}; }
inline bool bg_covers(const BgStamp& s, uint64_t set) { return s.id != 0 && set != 0 && (s.scope == kBgWhole || s.scope == set); }
inline uint64_t bg_tagged(uint64_t id, bool modulated) { return modulated ? id | kBgModulated : id; }
// rule 2: after an SVGF draw (elided or not) whose quiet-tile set is `set`, an output holds on those tiles what the
// input it copies from held there; without a set, or with an input that says nothing about the set, it is fresh
inline BgStamp bg_copy(const BgStamp& in, uint64_t set, bool modulated, uint64_t* serial) {
  if (!bg_covers(in, set)) return bg_fresh(serial);
  return BgStamp{bg_tagged(in.id, modulated), set};
}
// rule 3: the draw would store on the set's tiles what `out` already holds there
inline bool bg_pair_quiet(const BgStamp& in, const BgStamp& out, uint64_t set, bool modulated) {
  return bg_covers(in, set) && bg_covers(out, set) && out.id == bg_tagged(in.id, modulated);
}

// Which quiet-tile set a reproject draw works with. A set belongs to one (primary content, G-buffer content) pair; it
// is built when a draw meets the pair of the draw before it, so a moving camera builds none and pays the compare.
struct QuietChoice {
  uint64_t prim = 0, gbuf = 0;  // the last draw's pair
  uint64_t set = 0;             // the set built for it, 0: none yet
};
// returns the draw's set (0: none); *build: the caller builds the flags of the returned (new) set now
inline uint64_t quiet_set_for(QuietChoice& c, uint64_t prim, uint64_t gbuf, uint64_t* serial, bool* build) {
  *build = false;
  if (!prim || !gbuf) {
    c = QuietChoice{};
    return 0;
  }
  if (c.prim != prim || c.gbuf != gbuf) {
    c.prim = prim;
    c.gbuf = gbuf;
    c.set = 0;
    return 0;
  }
  if (!c.set) {
    c.set = ++*serial;
    *build = true;
  }
  return c.set;
}

// ------------------------------------------------ the bounce-0 shade's keep mode ---
// DESIGN.md "Static view, part 4". On a standing view the bounce-0 shade stores, on every miss pixel, the colour,
// emission and albedo texels the planes already hold, and on every hit pixel the emission and albedo texels they
// already hold. A draw leaves those stores out (and does not visit all-miss tiles) only where the host has proven it.
//
// The key of a pixel's emission and albedo texels: which pixels hit what and where (the primary content), and what
// decode_hit reads on the way to Material::emissive and ::baseColor beyond tri_geom, which the primary content covers:
// the tri_shade records, and the texture array a negative baseColor is fetched from. use_normal_map, the metallic and
// roughness layers' results and frameCounter reach neither.
enum FirstHitKeyField {
  kFkPrimary0,                              // primary_content() of the draw's PrimaryKey
  kFkTriShade = kFkPrimary0 + kPkWords,     // SceneDev::tri_shade, and the version of the texture it was decoded from
  kFkTriShadeVer,                           // with, in the high half, the scene's count of pt_materials_update calls
  kFkMatHandle, kFkMatDev, kFkMatVer,       // material_array: handle, device pointer, Texture::version
  kFkMatW, kFkMatH, kFkMatLayers,           // and its size
  kFkWords
};
struct FirstHitKey {
  uint64_t w[kFkWords];
};

// FirstHitMode / FirstHitReason: include/ptsvgf_debug_firsthit.h's PT_FH_* values.
enum FirstHitMode { kFhOff = 0, kFhFull = 1, kFhKeep = 2 };
enum FirstHitReason {
  kFhrNone, kFhrUniform, kFhrEnv, kFhrStats, kFhrSpp, kFhrBatch, kFhrMegakernel, kFhrTiles, kFhrRows, kFhrDeep,
  kFhrUnfolded, kFhrDepth0, kFhrAccumulate,  // bypasses: mode off; bit (1 << reason) of `bypass` below
  kFhrStage, kFhrColour, kFhrEmission, kFhrAlbedo,  // full: the stage ran, or an attachment does not hold this content
  kFhrCount
};
// The mode of a draw. bypass: bit r set when bypass reason r holds (the lowest one is reported). stage_reused: the
// draw reads the cached primary hit. colour: the colour attachment's background stamp as the draw finds it, before
// its own att_plane renews it; emission, albedo: the attachments' first-hit records as the draw finds them (0: none).
// miss, first: the content ids of the draw's MissKey and FirstHitKey. A draw that is not bypassed qualifies: kept or
// not, it leaves the three attachments holding its contents and records that after a successful launch.
inline int first_hit_mode(uint32_t bypass, bool stage_reused, const BgStamp& colour, uint64_t emission,
                          uint64_t albedo, uint64_t miss, uint64_t first, int* reason) {
  for (int r = kFhrUniform; r <= kFhrAccumulate; ++r)
    if (bypass & (1u << r)) {
      *reason = r;
      return kFhOff;
    }
  *reason = !stage_reused ? kFhrStage
            : !(miss && colour.id == miss && colour.scope == kBgWhole) ? kFhrColour
            : !(first && emission == first) ? kFhrEmission
            : !(first && albedo == first) ? kFhrAlbedo
                                          : kFhrNone;
  return *reason == kFhrNone ? kFhKeep : kFhFull;
}

}  // namespace ptk

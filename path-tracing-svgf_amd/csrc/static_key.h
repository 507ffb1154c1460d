// static_key.h — the key of everything the path tracer's primary stage reads (DESIGN.md "Static view"). A pass keeps
// the key of the last stage it ran; a draw whose key equals it reads the primary hit plane that stage wrote
// (WFState::hit0) instead of running the stage again. Plain host C++ with no HIP type, so the CPU suite reaches the
// compare through pt_debug_primary_key_diff.
//
// A key is one 64-bit word per field: a pointer's address, an integer, or a float's bit pattern (so a NaN equals
// itself, and -0 differs from +0, which costs one stage and is never wrong). The compare walks the words, so a field
// cannot be left out of it; a new input of the stage is a new enumerator here and a line in capi.hip's primary_key().
#pragma once
#include <stdint.h>
#include <string.h>

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

// the first field in which the keys differ, -1 when they are equal
inline int primary_key_diff(const PrimaryKey& a, const PrimaryKey& b) {
  for (int i = 0; i < kPkWords; ++i)
    if (a.w[i] != b.w[i]) return i;
  return -1;
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
  return !bypass && c.valid && primary_key_diff(c.key, now) < 0;
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

inline int lights_key_diff(const LightsKey& a, const LightsKey& b) {
  for (int i = 0; i < kLkWords; ++i)
    if (a.w[i] != b.w[i]) return i;
  return -1;
}

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
  return c.valid && lights_key_diff(c.key, now) < 0 ? 2 : 1;
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

inline int gbuf_key_diff(const GbufKey& a, const GbufKey& b) {
  for (int i = 0; i < kGkWords; ++i)
    if (a.w[i] != b.w[i]) return i;
  return -1;
}

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
  return enabled && c.valid && planes && gbuf_key_diff(c.key, now) < 0;
}

}  // namespace ptk

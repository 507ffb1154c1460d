// lights_key.h — the staleness rules of point lights that move (pt_lights_update; DESIGN.md "Moving point lights").
// Plain host C++ with no HIP type, beside static_key.h, so the CPU suite reaches the rules through
// pt_debug_lights_* (include/ptsvgf_debug_lights.h).
//
// A lights texture keeps, per light, the Texture::version at which its position last changed bitwise (its position
// stamp; 0: never since the texture was created). Occlusion depends on a light's position alone, so a colour-only
// update moves no stamp. Everything that caches per light (the triangle bins, the verdict cache's words) compares the
// stamps with the version it was made at.
#pragma once
#include <stdint.h>

#include "point_cache.h"
#include "static_key.h"

namespace ptk {

// which of the lights 0 .. nl-1 (the first 32) moved after version `since`: bit l set iff its stamp is newer
inline uint32_t lights_moved_mask(const uint64_t* pos_stamp, int nl, uint64_t since) {
  uint32_t m = 0;
  for (int l = 0; l < nl && l < 32; ++l)
    if (pos_stamp[l] > since) m |= 1u << l;
  return m;
}

// ---------------------------------------------------------------- the bins of one light ---
// What a path-tracing draw does with one light's bins. `built`: the stamp its lists were built for; a light whose
// stamp differs is stale: its rays walk (info[l][0] = 2, "moved, bins pending") until `settle` consecutive draws have
// found the stamp they found before, then its lists are rebuilt. settle = 0 rebuilds at the first draw after the move.
enum LightBinsAction {
  kLbKeep = 0,     // the lists are this position's
  kLbMark = 1,     // stale since this draw: mark it on the device
  kLbWalk = 2,     // stale and already marked
  kLbRebuild = 3,  // settled: rebuild this light's lists now
};
struct LightBinsState {
  uint64_t built = 0, seen = 0;
  int still = 0;        // consecutive draws that found `seen` again
  bool marked = false;  // info[l][0] says 2 on the device
};
inline int light_bins_step(LightBinsState& s, uint64_t stamp, int settle) {
  if (stamp == s.built) {
    s.seen = stamp;
    s.still = 0;
    return kLbKeep;
  }
  if (stamp != s.seen) {
    s.seen = stamp;
    s.still = 0;
  } else if (s.still < 0x7fffffff) {
    s.still++;
  }
  if (s.still >= (settle > 0 ? settle : 0)) {
    s.built = stamp;
    s.still = 0;
    s.marked = false;
    return kLbRebuild;
  }
  if (!s.marked) {
    s.marked = true;
    return kLbMark;
  }
  return kLbWalk;
}

// ---------------------------------------------------------------- the verdict cache ---
// pc_forget lives in point_cache.h (the kernels use it). The mode rule: a draw that reuses the primary stage and whose
// key differs from the cache's only in the lights' version or device pointer and in the bins fields, with the same
// (non-zero) lights handle and a newer version, forgets the moved lights' bits and then uses the cache
// (*forget = true; the caller takes the mask from lights_moved_mask with since = the cache key's version). The verdict
// is the same whoever decides the ray, so the bins fields may change with the lights. Anything else: point_cache_mode.
inline bool lights_key_forgettable(const LightsKey& last, const LightsKey& now) {
  if (!now.w[kLkLightHandle] || now.w[kLkLightVer] <= last.w[kLkLightVer]) return false;
  return key_diff(last, now, {kLkLightDev, kLkLightVer, kLkPointBins, kLkPointBinsDev}) < 0;
}
inline int point_cache_mode_lights(const PointCache& c, const LightsKey& now, bool stage_reused, bool bypass,
                                   bool* forget) {
  *forget = false;
  const int mode = point_cache_mode(c, now, stage_reused, bypass);
  if (mode != kPcReset || !c.valid || !lights_key_forgettable(c.key, now)) return mode;
  *forget = true;
  return kPcUse;
}
// after the draw's launch, in place of point_cache_note: a draw that forgot moves the cache's key on to its own
inline void point_cache_note_lights(PointCache& c, const LightsKey& now, int mode, bool forget, bool ok) {
  point_cache_note(c, now, mode, ok);
  if (ok && mode == kPcUse && forget) c.key = now;
}

}  // namespace ptk

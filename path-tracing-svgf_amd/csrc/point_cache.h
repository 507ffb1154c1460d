// point_cache.h — the word the bounce-0 point-light verdict cache keeps per pixel (DESIGN.md "Static view, part 2").
// The bounce-0 shade picks one of pointLightSize lights per pixel per frame and asks whether it is occluded from the
// pixel's first hit point. That point is a function of the primary hit (WFState::hit0) and the light's position is a
// constant, so from a standing view the verdict per (pixel, light) never changes: WFState::pcache remembers it.
//   bits 0-3   verdict known for light i
//   bits 4-7   light i occluded
//   bits 8-10  the light whose ray this frame queued, as index + 1; 0: none
// Plain constexpr functions with no HIP type (usable on the host and on the device), so the kernels include this
// header and the CPU suite reaches it through pt_debug_point_cache_word.
#pragma once
#include <stdint.h>

namespace ptk {

constexpr int kPcLights = 4;  // lights a word has room for: a draw with pointLightSize outside 1 .. 4 bypasses the cache
// PTParams::point_cache, the draw's mode. Off: no kernel touches the plane. Reset: every pixel of the bounce-0 shade
// stores a fresh word (nothing is read). Use: a pixel that would queue a point-light ray looks its light up first.
enum PointCacheMode { kPcOff = 0, kPcReset = 1, kPcUse = 2 };

constexpr uint32_t kPcPendingMask = 7u << 8;

// the verdict of light li: -1 not known, 0 lit, 1 occluded
constexpr int pc_lookup(uint32_t w, int li) {
  return ((w >> li) & 1u) ? (int)((w >> (4 + li)) & 1u) : -1;
}
// the light whose ray is queued, -1 for none
constexpr int pc_pending(uint32_t w) { return (int)((w & kPcPendingMask) >> 8) - 1; }
// light li's ray is queued this frame (replaces an earlier pending light)
constexpr uint32_t pc_mark_pending(uint32_t w, int li) { return (w & ~kPcPendingMask) | ((uint32_t)(li + 1) << 8); }
// the pending light's ray came back with `occluded`: its two bits are set, pending is cleared. A word with no pending
// light (or an index past the word's lights) only loses its pending field.
constexpr uint32_t pc_resolve(uint32_t w, bool occluded) {
  const int li = pc_pending(w);
  w &= ~kPcPendingMask;
  if (li < 0 || li >= kPcLights) return w;
  w |= 1u << li;
  return occluded ? (w | (1u << (4 + li))) : (w & ~(1u << (4 + li)));
}
// the lights of `mask` (bit i: light i) moved (pt_lights_update): their known and occluded bits are cleared, and the
// pending field too if it names one of them (its ray went to the old position). The other lights' bits stay.
constexpr uint32_t pc_forget(uint32_t w, uint32_t mask) {
  const uint32_t m = mask & ((1u << kPcLights) - 1u);
  const int li = pc_pending(w);
  w &= ~(m | (m << 4));
  if (li >= 0 && li < kPcLights && ((m >> li) & 1u)) w &= ~kPcPendingMask;
  return w;
}

}  // namespace ptk

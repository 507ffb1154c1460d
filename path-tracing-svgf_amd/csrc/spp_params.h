// spp_params.h — host side of a samples-per-pixel draw (uniform spp, DESIGN.md "Samples per pixel"): the Sobol
// point of a frame counter and the parameter block of each sample. Plain host code over pt_device.h's structs, so a
// stand-alone program can exercise it under the host sanitizers (tools/spp_params_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pt_device.h"

namespace ptk {

// sobol(d, i) of path_tracing.frag:455-463 (i: the Gray code of the index)
inline float sobol_host(uint32_t d, uint32_t i) {
  static const uint32_t V[8 * 32] = {
#include "sobol_v.inc"
  };
  uint32_t r = 0u;
  for (uint32_t j = 0u; i > 0u; i >>= 1u, j++)
    if ((i & 1u) == 1u) r ^= V[j + d * 32u];
  return (float)r * (1.0f / (float)0xFFFFFFFFu);
}

// frameCounter and the sobolVec2(frameCounter + 1, b) of the four bounces, uniform across pixels
inline void pt_counter_params(PTParams& k, uint32_t counter) {
  k.frameCounter = counter;
  for (int b = 0; b < 4; ++b) {
    const uint32_t i = counter + 1u;
    const uint32_t gc = i ^ (i >> 1);
    k.sobol_u[b] = sobol_host(2u * b, gc);
    k.sobol_v[b] = sobol_host(2u * b + 1u, gc);
  }
}

// Sample s of n of the draw `pass` (complete: pt_params and pt_wf_setup ran): a copy with the counter F * n + s
// (uint32, wrapping), no accumulation (wf_spp_resolve mixes the mean with lastFrame), the wavefront state `st` (frame
// s of the pass's batch state; the pass's probes and budgets are kept) and sample plane s as its colour output:
// `planes` holds n planes of W * (y1 - y0) texels, plane s addressed as a band plane of the draw's rows.
inline void spp_sample_params(const PTParams& pass, int n, int s, const WFState& st, float4* planes, PTParams* out) {
  PTParams k = pass;
  pt_counter_params(k, pass.frameCounter * (uint32_t)n + (uint32_t)s);
  k.accumulate = 0;
  k.last = Plane{};
  WFState w = st;
  w.row_cost = pass.wf.row_cost;
  w.shadow_budget = pass.wf.shadow_budget;
  w.closest_budget = pass.wf.closest_budget;
  w.stats = pass.wf.stats;
  w.stats_n = pass.wf.stats_n;
  k.wf = w;
  const int rows = pass.y1 > pass.y0 ? pass.y1 - pass.y0 : 0;
  const size_t npix = (size_t)pass.W * (size_t)rows;
  k.color = Plane{planes + (size_t)s * npix, nullptr, pass.W, pass.y0, rows};
  *out = k;
}

}  // namespace ptk

// kernels_spp.hip — samples per pixel (DESIGN.md "Samples per pixel", "Adaptive sample counts", "SVGF from sample
// moments"): the resolve that folds an spp draw's sample planes into the colour attachment (launched at the end of
// kernels_wavefront.hip's schedule), and the kernels that derive the next draw's per-pixel sample counts.
#include <hip/hip_runtime.h>

#include "glsl_builtins.h"
#include "pt_device.h"
#include "pt_shading.h"
#include "wf_common.h"

using namespace glsl;

namespace ptk {

// ------------------------------------------------------ samples per pixel ---
// The mean of an spp draw's samples (tests/spp_ref.py): sum = c_0, then sum + c_s in sample order, one IEEE division
// by float(n), alpha 1; with accumulation the mix with lastFrame at the frame's own counter (terminal_write's
// statement). One thread per pixel of the drawn tile subset, block b the subset's tile b as in the bounce-0 shade
// (raster order: the resolve has no slow tiles to start first), so pixels outside the subset or the band's rows keep
// their contents. Every index comes from the launch geometry; 16 (n + 1) bytes per pixel, each touched once.
__global__ void __launch_bounds__(256) wf_spp_resolve(SppResolve r) {
  const int ntx = (r.W + 15) / 16;
  const int tile = (int)blockIdx.x * r.tile_stride + r.tile_offset;
  const int x = (tile % ntx) * 16 + (threadIdx.x & 15), ly = (tile / ntx) * 16 + (threadIdx.x >> 4);
  if (x >= r.W || ly >= r.y1 - r.y0) return;
  const size_t pid = (size_t)ly * r.W + x;
  v3 sum = xyz(ldnt(&r.samples[pid]));
  for (int s = 1; s < r.n; ++s) sum = add(sum, xyz(ldnt(&r.samples[(size_t)s * r.stride + pid])));
  v3 color = divs(sum, (float)r.n);
  const int y = r.y0 + ly;
  if (r.accumulate && r.last.p) {  // :1116-1119
    float4 lc = pld(r.last, x, y);
    color = mixv(xyz(lc), color, 1.0f / (float)(r.frameCounter + 1u));
  }
  pst(r.color, x, y, f4(color.x, color.y, color.z, 1.0f));
}

// luminance of svgf_reproject.frag (kernels_svgf.hip lum), of a sample's colour
__device__ __forceinline__ float spp_lum(v3 c) { return (0.2125f * c.x + 0.7154f * c.y) + 0.0721f * c.z; }

// wf_spp_resolve with a count plane and / or a statistics plane bound (tests/adaptive_ref.py; DESIGN.md "Adaptive
// sample counts"). COUNTS: the pixel folds its first n = min(max(c, 1), N) samples, in sample order, and divides by
// float(n); the planes of samples that do not exist are not read. STATS: the samples' luminances stay in registers
// (the loops are unrolled over kMaxBatch and predicated on s < n) and one 8-byte store writes (m, v): the mean in
// sample order over float(n) and sum (l_s - m)^2 in sample order over float(n - 1); (l_0, -1) at n < 2. Block and
// thread indices as wf_spp_resolve; no LDS, no atomics; 16 (n + 1) + 1 + 8 bytes per pixel, each touched once.
// MOMENTS (DESIGN.md "SVGF from sample moments"; tests/sample_moments_ref.cpp): the draw's own emission and albedo
// texels (two more 16-byte loads) demodulate every sample as svgf_reproject.frag demodulates the mean, illum_s =
// (c_s - e) / max(a, 0.001) per channel, 0 when a channel is NaN; with l_s = lum(illum_s) in registers, one 16-byte
// store writes (mu, nu, r, float(n)): mu = (l_0 + l_1 + ...) / float(n) and nu = (l_0 l_0 + l_1 l_1 + ...) / float(n)
// in sample order, r = 1 / float(n), times the accumulation's mix weight when the draw accumulates.
__device__ __forceinline__ float spp_demod_lum(v3 c, v3 e, v3 den) {
  v3 il = mk((c.x - e.x) / den.x, (c.y - e.y) / den.y, (c.z - e.z) / den.z);
  if (f_isnan(il.x) || f_isnan(il.y) || f_isnan(il.z)) il = splat(0.0f);
  return spp_lum(il);
}
template <bool COUNTS, bool STATS, bool MOMENTS>
__global__ void __launch_bounds__(256) wf_spp_resolve_adaptive(SppResolve r, SppAdaptive a) {
  const int ntx = (r.W + 15) / 16;
  const int tile = (int)blockIdx.x * r.tile_stride + r.tile_offset;
  const int x = (tile % ntx) * 16 + (threadIdx.x & 15), ly = (tile / ntx) * 16 + (threadIdx.x >> 4);
  if (x >= r.W || ly >= r.y1 - r.y0) return;
  const size_t pid = (size_t)ly * r.W + x;
  const int y = r.y0 + ly;
  const size_t gp = (size_t)y * r.W + x;  // the count and statistics planes hold the frame's rows
  int n = r.n;
  if (COUNTS) n = min(max((int)a.counts[gp], 1), r.n);
  float l[kMaxBatch];
  v3 sum = xyz(ldnt(&r.samples[pid]));
  l[0] = spp_lum(sum);
  v3 e = splat(0.0f), den = splat(1.0f);
  float mu = 0.0f, nu = 0.0f;  // MOMENTS: the running sums of l_s and l_s l_s of the demodulated samples
  if (MOMENTS) {
    e = xyz(pld(a.emission, x, y));
    const v3 al = xyz(pld(a.albedo, x, y));
    den = mk(f_max(al.x, 0.001f), f_max(al.y, 0.001f), f_max(al.z, 0.001f));
    mu = spp_demod_lum(sum, e, den);
    nu = mu * mu;
  }
#pragma unroll
  for (int s = 1; s < kMaxBatch; ++s) {
    l[s] = 0.0f;
    if (s < n) {
      const v3 c = xyz(ldnt(&r.samples[(size_t)s * r.stride + pid]));
      sum = add(sum, c);
      if (STATS) l[s] = spp_lum(c);
      if (MOMENTS) {
        const float d = spp_demod_lum(c, e, den);
        mu = mu + d;
        nu = nu + d * d;
      }
    }
  }
  v3 color = divs(sum, (float)n);
  float rr = 1.0f / (float)n;  // MOMENTS: a per-sample variance to the variance of the colour written below
  if (r.accumulate && r.last.p) {  // :1116-1119
    float4 lc = pld(r.last, x, y);
    color = mixv(xyz(lc), color, 1.0f / (float)(r.frameCounter + 1u));
    rr = rr * (1.0f / (float)(r.frameCounter + 1u));
  }
  pst(r.color, x, y, f4(color.x, color.y, color.z, 1.0f));
  if (MOMENTS) a.moments[gp] = f4(mu / (float)n, nu / (float)n, rr, (float)n);
  if (STATS) {
    float m = l[0], v = -1.0f;
    if (n >= 2) {
#pragma unroll
      for (int s = 1; s < kMaxBatch; ++s)
        if (s < n) m = m + l[s];
      m = m / (float)n;
      float m2 = (l[0] - m) * (l[0] - m);
#pragma unroll
      for (int s = 1; s < kMaxBatch; ++s)
        if (s < n) m2 = m2 + (l[s] - m) * (l[s] - m);
      v = m2 / (float)(n - 1);
    }
    a.stats[gp] = make_float2(m, v);
  }
}

// pt_sample_counts_derive (tests/adaptive_ref.py derive_counts): one thread per frame pixel, one byte stored. A
// background pixel (nd.w == 1) takes 1 sample. A surface pixel looks its statistics up where it was `lag` frames ago,
// q = floor(pixel centre - lag * motion * size), and takes the largest need of the 3 x 3 texels around q inside the
// frame: N where there is no estimate (v < 0, NaN), else ceil(v / (tol * max(m, 1e-4))^2) held to 2 .. N. A
// non-finite position or a q outside the frame gives N. Every read is of a texel the rule has tested to lie in the
// frame; the nine 8-byte reads of neighbouring threads overlap, so all but the first come from L1 / L2.
__global__ void __launch_bounds__(256) spp_counts_kernel(SppCountsParams c) {
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x >= c.W || y >= c.H) return;
  const size_t i = (size_t)y * c.W + x;
  int count;
  if (c.nd[i].w == 1.0f) {
    count = 1;
  } else {
    const float4 mv = c.motion[i];
    const float fx = ((float)x + 0.5f) - (c.lag * mv.x) * (float)c.W;
    const float fy = ((float)y + 0.5f) - (c.lag * mv.y) * (float)c.H;
    count = c.nmax;
    // (NaN fails every comparison; the bounds hold in float before the conversion, so no int overflows)
    if (fx >= 0.0f && fx < (float)c.W && fy >= 0.0f && fy < (float)c.H) {
      const int qx = (int)floorf(fx), qy = (int)floorf(fy);
      count = 0;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int sx = qx + dx, sy = qy + dy;
          if (sx < 0 || sx >= c.W || sy < 0 || sy >= c.H) continue;
          const float2 mvv = c.stats[(size_t)sy * c.W + sx];
          const float m = mvv.x, v = mvv.y;
          int r = c.nmax;
          if (!(v < 0.0f) && !f_isnan(m) && !f_isnan(v)) {
            const float d = c.tol * fmaxf(m, 1e-4f);
            const float k = ceilf(v / (d * d));
            if (k < (float)c.nmax) r = max(2, (int)k);
          }
          count = max(count, r);
        }
    }
  }
  c.out[i] = (uint8_t)count;
}

int launch_spp_counts(const SppCountsParams& c, hipStream_t s) {
  if (c.W <= 0 || c.H <= 0) return 0;
  hipLaunchKernelGGL(spp_counts_kernel, dim3((c.W + 15) / 16, (c.H + 15) / 16), dim3(256), 0, s, c);
  return (int)hipGetLastError();
}

// One texel of pt_sample_counts_pool (tests/adaptive_pool_ref.py T(p) and r(T)) for the frame pixel (x, y), which the
// caller has tested to lie in the frame: the pooled statistics (m, v, w, z) and the samples they ask for (0 on the
// background). The history and the new samples are read at q, tested to lie in the frame, and only where the rule
// still needs them: nothing past a background pixel, an off-frame q or a failed depth test.
__device__ __forceinline__ int spp_pool_texel(const SppPoolParams& c, int x, int y, float4* T) {
  const size_t i = (size_t)y * c.W + x;
  const float4 nd = c.nd[i];
  *T = make_float4(0.0f, 0.0f, 0.0f, nd.z);
  if (nd.w == 1.0f) return 0;
  const float4 mv = c.motion[i];
  const float fx = ((float)x + 0.5f) - (c.lag * mv.x) * (float)c.W;
  const float fy = ((float)y + 0.5f) - (c.lag * mv.y) * (float)c.H;
  // (NaN fails every comparison; the bounds hold in float before the conversion, so no int overflows)
  if (!(fx >= 0.0f && fx < (float)c.W && fy >= 0.0f && fy < (float)c.H)) return c.nmax;
  const size_t q = (size_t)(int)floorf(fy) * c.W + (int)floorf(fx);
  float am = 0.0f, av = 0.0f, aw = 0.0f;  // the history (m, v, w); its z is the float4's fourth component
  bool a_ok = false;
  if (c.pool_in) {
    const float4 a = c.pool_in[q];
    am = a.x, av = a.y, aw = a.z;
    const float az = fabsf(nd.z);  // (a NaN stays a NaN through the floor below and fails the test)
    if (!(fabsf(a.w - nd.z) <= c.zeta * (az < 1e-4f ? 1e-4f : az))) return c.nmax;
    a_ok = aw >= 1.0f && __builtin_isfinite(am) && __builtin_isfinite(av);
  }
  int n = c.nmax_prev;
  if (c.counts_prev) n = min(max((int)c.counts_prev[q], 1), c.nmax_prev);
  const float ns = (float)n;
  float ms = 0.0f, vs = 0.0f;
  bool s_ok = false;
  if (c.stats) {
    const float2 st = c.stats[q];
    ms = st.x;
    s_ok = __builtin_isfinite(ms) && (n < 2 || (__builtin_isfinite(st.y) && st.y >= 0.0f));
    vs = n >= 2 ? st.y : 0.0f;
  }
  float m, v, w;
  if (a_ok && s_ok) {  // Chan's pairwise update, one rounding per operation (-ffp-contract=off)
    w = aw + ns;
    const float d = ms - am;
    m = am + d * (ns / w);
    const float m2 = (av * (aw - 1.0f) + vs * (ns - 1.0f)) + (d * d) * ((aw * ns) / w);
    v = m2 / (w - 1.0f);
    w = fminf(w, c.wmax);  // (w >= 2 here, never a NaN)
  } else if (s_ok) {
    m = ms, v = vs, w = ns;
  } else if (a_ok) {
    m = am, v = av, w = aw;
  } else {
    return c.nmax;
  }
  *T = make_float4(m, v, w, nd.z);
  if (!(w >= 2.0f)) return c.nmax;
  const float d = c.rule ? c.tol : c.tol * (m < 1e-4f ? 1e-4f : m);  // (a NaN m stays: k is a NaN, r = N)
  const float k = ceilf(v / (d * d));
  if (!(k < (float)c.nmax)) return c.nmax;
  return k >= 1.0f ? (int)k : 1;
}

// pt_sample_counts_pool: one fused launch, a block of 256 threads per 16 x 16 pixel tile. Every thread evaluates the
// texel of its own pixel and keeps it in registers; the first 68 threads also evaluate one texel of the apron ring
// (18 + 18 + 16 + 16). Each texel's need r goes to LDS as one byte (324 per block, 0 for a texel off the frame or on
// the background: neither raises a maximum); after one barrier each thread takes the 9-tap maximum around its pixel
// and stores one byte and one float4. No atomics; every global access is of a texel tested to lie in the frame.
__global__ void __launch_bounds__(256) spp_pool_kernel(SppPoolParams c) {
  __shared__ uint8_t need[18 * 18];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  const int x = x0 + tx, y = y0 + ty;
  const bool own = x < c.W && y < c.H;
  float4 T = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  need[(ty + 1) * 18 + tx + 1] = own ? (uint8_t)spp_pool_texel(c, x, y, &T) : (uint8_t)0;
  if (t < 68) {  // the ring: the rows above and below (18 texels each), then the columns left and right (16 each)
    int ax, ay;
    if (t < 36) {
      ax = t % 18, ay = t < 18 ? 0 : 17;
    } else {
      ax = t < 52 ? 0 : 17, ay = 1 + (t - 36) % 16;
    }
    const int px = x0 + ax - 1, py = y0 + ay - 1;
    float4 unused;
    need[ay * 18 + ax] =
        px >= 0 && px < c.W && py >= 0 && py < c.H ? (uint8_t)spp_pool_texel(c, px, py, &unused) : (uint8_t)0;
  }
  __syncthreads();
  if (!own) return;
  const size_t i = (size_t)y * c.W + x;
  int count = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) count = max(count, (int)need[(ty + dy) * 18 + tx + dx]);
  if (need[(ty + 1) * 18 + tx + 1] == 0) count = 1;  // the background: a surface texel's own need is >= 1
  c.pool_out[i] = T;
  c.out[i] = (uint8_t)count;
}

int launch_spp_pool(const SppPoolParams& c, hipStream_t s) {
  if (c.W <= 0 || c.H <= 0) return 0;
  hipLaunchKernelGGL(spp_pool_kernel, dim3((c.W + 15) / 16, (c.H + 15) / 16), dim3(256), 0, s, c);
  return (int)hipGetLastError();
}

// An spp draw's resolve, after every sample's colour is written on `s`: one block per tile of the drawn subset. With
// any of ad's planes bound it is the adaptive kernel instantiated for exactly those planes (the caller passes an `ad`
// with no plane as no `ad`), else the plain one.
void launch_spp_resolve(const SppResolve& rs, const SppAdaptive* ad, int ntiles, hipStream_t s) {
  using Kernel = void (*)(SppResolve, SppAdaptive);
  static constexpr Kernel kAdaptive[8] = {  // [counts << 2 | stats << 1 | moments]
      nullptr,
      wf_spp_resolve_adaptive<false, false, true>,
      wf_spp_resolve_adaptive<false, true, false>,
      wf_spp_resolve_adaptive<false, true, true>,
      wf_spp_resolve_adaptive<true, false, false>,
      wf_spp_resolve_adaptive<true, false, true>,
      wf_spp_resolve_adaptive<true, true, false>,
      wf_spp_resolve_adaptive<true, true, true>};
  const int planes = ad ? (ad->counts ? 4 : 0) | (ad->stats ? 2 : 0) | (ad->moments ? 1 : 0) : 0;
  if (planes) hipLaunchKernelGGL(kAdaptive[planes], dim3(ntiles), dim3(256), 0, s, rs, *ad);
  else hipLaunchKernelGGL(wf_spp_resolve, dim3(ntiles), dim3(256), 0, s, rs);
}

}  // namespace ptk

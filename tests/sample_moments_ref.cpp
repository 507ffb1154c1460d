// sample_moments_ref.cpp — TEST INFRASTRUCTURE ONLY. The definition of "SVGF from sample moments"  in
// plain C++: the plane a multi-sample path-tracing draw's resolve writes, and svgf_reproject.frag / svgf_variance.frag
// with and without the sampler gSampleMoments. Written from the definition and the shader text, one statement at a
// time; float32, one rounding per operation (build with -ffp-contract=off). It shares the GLSL built-in library
// (glsl_builtins.h: pow, exp, the bilinear sampler) with the kernels, as the oracle does, and nothing else.
// tests/sample_moments_ref.py compiles and loads it.
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "glsl_builtins.h"

namespace {

using glsl::v3;

struct Tex {  // an RGBA32F texture of the frame's size
  const float* p;
  int W, H;
  const float* texel(int x, int y) const { return p + 4 * ((size_t)y * W + x); }
  // texture2D(GL_LINEAR, GL_CLAMP_TO_EDGE)
  void sample(float u, float v, float out[4]) const { glsl::tex2d_linear(p, W, H, 4, u, v, out, 4); }
};

// vert.vert hands the fragment pix = the pixel centre in NDC; every shader starts with uv = pix.xy * 0.5 + 0.5
float centre_uv(int i, int n) {
  const float pix = (float)(2 * i + 1) / (float)n - 1.0f;
  return pix * 0.5f + 0.5f;
}

// luminance() of the three shaders
float luminance(const float c[3]) { return (0.2125f * c[0] + 0.7154f * c[1]) + 0.0721f * c[2]; }

// demodulate(c - e, albedo) of svgf_reproject.frag:26-29, :174-178, with its NaN rule
void demodulated(const float c[3], const float e[3], const float a[3], float out[3]) {
  for (int k = 0; k < 3; ++k) out[k] = (c[k] - e[k]) / glsl::f_max(a[k], 0.001f);
  if (glsl::f_isnan(out[0]) || glsl::f_isnan(out[1]) || glsl::f_isnan(out[2])) out[0] = out[1] = out[2] = 0.0f;
}

struct Thresholds {
  float depth, normal;
};

// isReprjValid, svgf_reproject.frag:31-43
bool reprojection_valid(float u, float v, float Z, float Zprev, float fwidthZ, const float n[3], const float np[3],
                        float fwidthNormal, Thresholds t) {
  if (u < 0.0f || u > 1.0f || v < 0.0f || v > 1.0f) return false;
  if (glsl::f_abs(Zprev - Z) / (fwidthZ + 1e-2f) > t.depth) return false;
  const float d = glsl::distance(glsl::mk(n[0], n[1], n[2]), glsl::mk(np[0], np[1], np[2]));
  if (d / (fwidthNormal + 1e-2f) > t.normal) return false;
  return true;
}

// computeWeight, svgf_variance.frag:23-35
float compute_weight(float zC, float zP, float phiDepth, const float nC[3], const float nP[3], float phiNormal,
                     float lC, float lP, float phiIllum) {
  const float cosine = glsl::dot(glsl::mk(nC[0], nC[1], nC[2]), glsl::mk(nP[0], nP[1], nP[2]));
  const float weightNormal = glsl::g_pow(glsl::f_clamp(cosine, 0.0f, 1.0f), phiNormal);
  const float weightZ = phiDepth == 0.0f ? 0.0f : glsl::f_abs(zC - zP) / phiDepth;
  const float weightL = glsl::f_abs(lC - lP) / phiIllum;
  return glsl::g_exp((0.0f - glsl::f_max(weightL, 0.0f)) - glsl::f_max(weightZ, 0.0f)) * weightNormal;
}

}  // namespace

// The resolve's plane. samples: N frames of H x W x 4 (spp_ref's per-sample colours), emission / albedo: the draw's
// own, counts: H x W bytes or null (every pixel takes N), accumulating != 0: the draw mixes with lastFrame at the
// counter F. out: H x W x 4, every pixel written.
extern "C" int smr_resolve_plane(int W, int H, int N, const float* samples, const float* emission, const float* albedo,
                                 const uint8_t* counts, int accumulating, uint32_t F, float* out) {
  if (N < 1 || N > 8) return 1;
  const size_t frame = (size_t)W * H * 4;
  for (size_t i = 0; i < (size_t)W * H; ++i) {
    int n = N;
    if (counts) {
      n = counts[i];
      if (n < 1) n = 1;
      if (n > N) n = N;
    }
    float l[8];
    for (int s = 0; s < n; ++s) {
      float illum[3];
      demodulated(samples + s * frame + 4 * i, emission + 4 * i, albedo + 4 * i, illum);
      l[s] = luminance(illum);
    }
    float first = l[0], second = l[0] * l[0];
    for (int s = 1; s < n; ++s) {
      first = first + l[s];
      second = second + l[s] * l[s];
    }
    float r = 1.0f / (float)n;
    if (accumulating) r = r * (1.0f / (float)(F + 1u));
    out[4 * i + 0] = first / (float)n;
    out[4 * i + 1] = second / (float)n;
    out[4 * i + 2] = r;
    out[4 * i + 3] = (float)n;
  }
  return 0;
}

// svgf_reproject.frag. sm: the sample-moments plane, or null (the shader as it is). motion.z is the object's own share
// of the depth change (0 unless the G-buffer had displacement records): the current depth the validity test compares
// is nd.w + motion.z, as in the build's kernel.
extern "C" int smr_reproject(int W, int H, const float* motion, const float* color, const float* albedo,
                             const float* emission, const float* prev_illum, const float* prev_moments,
                             const float* nd, const float* prev_nd, const float* fwidth, const float* sm, float inv_w,
                             float inv_h, float depth_thr, float normal_thr, float* out_illum, float* out_moments) {
  const Tex gMotion{motion, W, H}, gColor{color, W, H}, gAlbedo{albedo, W, H}, gEmission{emission, W, H};
  const Tex gPrevIllum{prev_illum, W, H}, gPrevMoments{prev_moments, W, H}, gND{nd, W, H}, gPrevND{prev_nd, W, H};
  const Tex gFwidth{fwidth, W, H};
  const Thresholds thr{depth_thr, normal_thr};
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      float* OutIllumination = out_illum + 4 * ((size_t)y * W + x);
      float* OutMoments = out_moments + 4 * ((size_t)y * W + x);
      const float u = centre_uv(x, W), v = centre_uv(y, H);
      const float* cur = gND.texel(x, y);  // a fetch at a texel centre is the texel
      if (cur[3] == 1.0f) {                // :166-171
        memcpy(OutIllumination, gColor.texel(x, y), 16);
        memcpy(OutMoments, gPrevMoments.texel(x, y), 16);
        continue;
      }
      float illumination[3];
      demodulated(gColor.texel(x, y), gEmission.texel(x, y), gAlbedo.texel(x, y), illumination);

      // loadPrevData
      const float* mv = gMotion.texel(x, y);
      const float normal_fwidth = gFwidth.texel(x, y)[0], depth_fwidth = gFwidth.texel(x, y)[1];
      const float pu = u - mv[0], pv = v - mv[1];
      const float cur_depth = cur[3] + mv[2];
      float prevIllum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, prevMoments[2] = {0.0f, 0.0f};
      const float offu[4] = {0.0f, inv_w, 0.0f, inv_w}, offv[4] = {0.0f, 0.0f, inv_h, inv_h};
      bool tap[4], valid = false;
      for (int i = 0; i < 4; ++i) {
        float q[4];
        gPrevND.sample(pu + offu[i], pv + offv[i], q);
        tap[i] = reprojection_valid(pu + offu[i], pv + offv[i], cur_depth, q[3], depth_fwidth, cur, q, normal_fwidth,
                                    thr);
        valid = valid || tap[i];
      }
      if (valid) {
        float sumw = 0.0f;
        const float fx = pu - (float)glsl::f2i(pu / inv_w) * inv_w;
        const float fy = pv - (float)glsl::f2i(pv / inv_h) * inv_h;
        const float w[4] = {(1.0f - fx) * (1.0f - fy), fx * (1.0f - fy), (1.0f - fx) * fy, fx * fy};
        for (int i = 0; i < 4; ++i) {
          if (!tap[i]) continue;
          float qi[4], qm[4];
          gPrevIllum.sample(pu + offu[i], pv + offv[i], qi);
          gPrevMoments.sample(pu + offu[i], pv + offv[i], qm);
          for (int k = 0; k < 4; ++k) prevIllum[k] += w[i] * qi[k];
          for (int k = 0; k < 2; ++k) prevMoments[k] += w[i] * qm[k];
          sumw += w[i];
        }
        valid = sumw >= 0.01f;
        for (int k = 0; k < 4; ++k) prevIllum[k] = valid ? prevIllum[k] / sumw : 0.0f;
        for (int k = 0; k < 2; ++k) prevMoments[k] = valid ? prevMoments[k] / sumw : 0.0f;
      }
      if (!valid) {  // the 3 x 3 rescue, :111-141
        float nValid = 0.0f;
        for (int yy = -1; yy <= 1; ++yy)
          for (int xx = -1; xx <= 1; ++xx) {
            const float lu = pu + (float)xx * inv_w, lv = pv + (float)yy * inv_h;
            float q[4];
            gPrevND.sample(lu, lv, q);
            if (!reprojection_valid(lu, lv, cur_depth, q[3], depth_fwidth, cur, q, normal_fwidth, thr)) continue;
            float qi[4], qm[4];
            gPrevIllum.sample(lu, lv, qi);
            gPrevMoments.sample(lu, lv, qm);
            for (int k = 0; k < 4; ++k) prevIllum[k] += qi[k];
            for (int k = 0; k < 2; ++k) prevMoments[k] += qm[k];
            nValid += 1.0f;
          }
        if (nValid > 0.0f) {
          valid = true;
          for (int k = 0; k < 4; ++k) prevIllum[k] /= nValid;
          for (int k = 0; k < 2; ++k) prevMoments[k] /= nValid;
        }
      }
      float historyLength = 0.0f;
      if (valid) {
        float q[4];
        gPrevMoments.sample(pu, pv, q);
        historyLength = q[2];
      } else {
        for (int k = 0; k < 4; ++k) prevIllum[k] = 0.0f;
        prevMoments[0] = prevMoments[1] = 0.0f;
      }

      // main(), :185-202
      historyLength = glsl::f_min(32.0f, valid ? historyLength + 1.0f : 1.0f);
      const float alpha = valid ? glsl::f_max(0.2f, 1.0f / historyLength) : 1.0f;
      float first, second, scale = 1.0f;
      if (sm) {  // the draw's own sample moments in place of (lum, lum^2) of the mean
        const float* t = sm + 4 * ((size_t)y * W + x);
        first = t[0];
        second = t[1];
        scale = t[2];
      } else {
        first = luminance(illumination);
        second = first * first;
      }
      const float m0 = (1.0f - alpha) * prevMoments[0] + alpha * first;
      const float m1 = (1.0f - alpha) * prevMoments[1] + alpha * second;
      float variance = glsl::f_max(0.0f, m1 - m0 * m0);
      if (sm) variance = variance * scale;
      for (int k = 0; k < 3; ++k) OutIllumination[k] = (1.0f - alpha) * prevIllum[k] + alpha * illumination[k];
      OutIllumination[3] = variance;
      OutMoments[0] = m0;
      OutMoments[1] = m1;
      OutMoments[2] = historyLength;
      OutMoments[3] = 0.0f;  // (the shader leaves it unwritten; the build defines 0)
    }
  return 0;
}

// svgf_variance.frag. sm: the sample-moments plane (read at the centre only), or null.
extern "C" int smr_variance(int W, int H, const float* illum, const float* moments, const float* nd,
                            const float* fwidth, const float* sm, float gPhiColor, float gPhiNormal, float* out) {
  const Tex gIllumination{illum, W, H}, gMoments{moments, W, H}, gND{nd, W, H}, gFwidth{fwidth, W, H};
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      float* o = out + 4 * ((size_t)y * W + x);
      const float* centre = gIllumination.texel(x, y);
      const float h = gMoments.texel(x, y)[2];
      const float* t = sm ? sm + 4 * ((size_t)y * W + x) : nullptr;
      const float have = t ? h * t[3] : h;  // values the temporal estimate rests on: frames, or frames x samples
      const float* ndc = gND.texel(x, y);
      if (!(have < 4.0f) || ndc[3] == 1.0f) {  // enough history, or the environment: pass through
        memcpy(o, centre, 16);
        continue;
      }
      const float lC = luminance(centre);
      const float phiDepth = glsl::f_max(gFwidth.texel(x, y)[1], 1e-8f) * 3.0f;
      float sumW = 0.0f, sumI[3] = {0.0f, 0.0f, 0.0f}, sumM[2] = {0.0f, 0.0f};
      for (int yy = -3; yy <= 3; ++yy)
        for (int xx = -3; xx <= 3; ++xx) {
          const int px = x + xx, py = y + yy;
          if (px < 0 || px >= W || py < 0 || py >= H) continue;  // :75, on texel centres
          const float* ip = gIllumination.texel(px, py);
          const float* mp = gMoments.texel(px, py);
          const float* q = gND.texel(px, py);
          const float len = glsl::f_sqrt((float)(xx * xx) + (float)(yy * yy));
          const float w = compute_weight(ndc[3], q[3], phiDepth * len, ndc, q, gPhiNormal, lC, luminance(ip),
                                         gPhiColor);
          sumW += w;
          for (int k = 0; k < 3; ++k) sumI[k] += ip[k] * w;
          for (int k = 0; k < 2; ++k) sumM[k] += mp[k] * w;
        }
      sumW = glsl::f_max(sumW, 1e-6f);
      for (int k = 0; k < 3; ++k) sumI[k] /= sumW;
      for (int k = 0; k < 2; ++k) sumM[k] /= sumW;
      float variance = sumM[1] - sumM[0] * sumM[0];
      variance *= 4.0f / have;
      if (t) variance *= t[2];
      o[0] = sumI[0];
      o[1] = sumI[1];
      o[2] = sumI[2];
      o[3] = variance;
    }
  return 0;
}

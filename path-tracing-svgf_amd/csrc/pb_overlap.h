// pb_overlap.h — which cube-map cells a projected polygon reaches (kernels_pointbins.hip pb_bin; restated on the host
// through pt_debug_point_bins_overlap). A face's clipped triangle is a convex polygon in cell coordinates; a ray's
// position q in the face lies within fw (in x and in y) of a point of it, so the cell of q must be kept. A cell is
// dropped only when its square, widened by fw, lies wholly beyond one edge's line (DESIGN.md "Point-light shadow rays
// by light-binned triangles", "Cells by the polygon").
#pragma once

#ifndef PB_HD
#ifdef __HIPCC__
#define PB_HD __host__ __device__ inline
#else
#define PB_HD inline
#endif
#endif

namespace ptk {

constexpr int kPbMaxVerts = 8;  // a triangle clipped by four planes has at most 7 vertices

// The edge lines of a polygon that may drop cells: s (a (x - x0) + b (y - y0)) >= -2 m holds at every vertex.
struct PbEdges {
  int n;  // 0: keep every cell of the box
  float a[kPbMaxVerts], b[kPbMaxVerts], x0[kPbMaxVerts], y0[kPbMaxVerts], m[kPbMaxVerts];
};

// Rounding of E(q) = a (qx - x0) + b (qy - y0), a = dy, b = -dx of an edge, all coordinates within 256 in magnitude
// (cell coordinates reach 1.005 R + fw < 130 at R = 128): the two differences of the edge carry (1 + d), |d| <= eps =
// 2^-24, as do (qx - x0), (qy - y0), the two products and the sum: |fl(E) - E| <= ((1 + eps)^4 - 1) (|a| + |b|) 512
// < 1.0025 * 2^-13 (|a| + |b|). A corner c + 1 + fw of the widened square rounds by at most 2 eps 256 = 2^-15,
// which moves E by at most 2^-15 (|a| + |b|). Together under m = 2^-12 (|a| + |b|); m is computed from the rounded a
// and b, within (1 + eps) of that, which the strict factors below absorb.
constexpr float kPbEdgeSlack = 1.0f / 4096.0f;

// Prepares the edges of the polygon (px, py)[0..n). An edge is used only if the computed E of every vertex lies on
// one side of it by -m (then every vertex, and so the polygon, the hull of its vertices, truly lies within 2 m of
// that side: no assumption on the vertex order, on convexity surviving the clip's rounding, or on the direction of a
// very short edge). Returns false, and n = 0, for a degenerate polygon: fewer than three distinct vertices, a signed
// area within its own rounding of zero, or a non-finite term.
PB_HD bool pb_edges(const float* px, const float* py, int n, PbEdges* out) {
  out->n = 0;
  if (n < 3 || n > kPbMaxVerts) return false;
  int distinct = 1;
  for (int k = 1; k < n; ++k) {
    bool seen = false;
    for (int j = 0; j < k; ++j) seen = seen || (px[j] == px[k] && py[j] == py[k]);
    distinct += seen ? 0 : 1;
  }
  if (distinct < 3) return false;
  float area = 0.0f, mag = 0.0f;
  for (int k = 1; k + 1 < n; ++k) {
    const float ax = px[k] - px[0], ay = py[k] - py[0], bx = px[k + 1] - px[0], by = py[k + 1] - py[0];
    area += ax * by - ay * bx;
    mag += fabsf(ax * by) + fabsf(ay * bx);
  }
  // (each fan term rounds by under 4 eps of its magnitudes, the running sum by eps per step: under 2^-20 mag in all)
  if (!(fabsf(area) > mag * (1.0f / 1048576.0f)) || !(mag <= 3.0e38f)) return false;
  int ne = 0;
  for (int k = 0; k < n; ++k) {
    const int k1 = k + 1 < n ? k + 1 : 0;
    const float a = py[k1] - py[k], b = -(px[k1] - px[k]);
    const float m = kPbEdgeSlack * (fabsf(a) + fabsf(b));
    if (!(m > 0.0f) || !(m <= 3.0e38f)) continue;  // two equal vertices: no line (or not finite)
    bool pos = true, negv = true, fin = true;
    for (int j = 0; j < n; ++j) {
      const float e = a * (px[j] - px[k]) + b * (py[j] - py[k]);
      fin = fin && (e == e);
      pos = pos && e >= -m;
      negv = negv && e <= m;
    }
    if (!fin || pos == negv) continue;  // vertices on both sides, or all on the line: this edge drops nothing
    const float s = pos ? 1.0f : -1.0f;
    out->a[ne] = s * a;
    out->b[ne] = s * b;
    out->x0[ne] = px[k];
    out->y0[ne] = py[k];
    out->m[ne] = m;
    ++ne;
  }
  out->n = ne;
  return true;
}

// Whether cell (cx, cy) of an R x R face is kept: false only if the square [cx - fw, cx + 1 + fw] x [cy - fw, cy + 1 +
// fw] lies beyond one prepared edge: the computed E of its corner farthest inside is under -4 m, so E < -3 m at every
// point of the true square, against E >= -2 m on the polygon. The cells at the face's border take the positions that
// are clamped into them too (a ray's cell coordinate can round to just outside [0, R]): their square reaches one cell
// further out.
PB_HD bool pb_cell_kept(const PbEdges& e, float fw, int cx, int cy, int R) {
  const float X0 = (float)(cx == 0 ? -1 : cx) - fw, X1 = (float)(cx == R - 1 ? R + 1 : cx + 1) + fw;
  const float Y0 = (float)(cy == 0 ? -1 : cy) - fw, Y1 = (float)(cy == R - 1 ? R + 1 : cy + 1) + fw;
  for (int k = 0; k < e.n; ++k) {
    const float qx = e.a[k] >= 0.0f ? X1 : X0, qy = e.b[k] >= 0.0f ? Y1 : Y0;
    const float v = e.a[k] * (qx - e.x0[k]) + e.b[k] * (qy - e.y0[k]);
    if (v < -4.0f * e.m[k]) return false;
  }
  return true;
}

// The whole predicate for one cell of the box [cx0, cx1] x [cy0, cy1] the caller found first: every cell of a box of
// at most two cells, and of a degenerate polygon's box, is kept.
PB_HD bool pb_cell_overlaps(const float* px, const float* py, int n, float fw, int cx, int cy, int R, int box_cells) {
  PbEdges e;
  if (box_cells <= 2 || !pb_edges(px, py, n, &e)) return true;
  return pb_cell_kept(e, fw, cx, cy, R);
}

}  // namespace ptk

// kernels_pointbins.hip — the build of the point-light triangle bins (PointBinsDev, pt_device.h): for every point
// light a cube map of direction cells around it, each cell listing the triangles a shadow ray arriving at the light
// from that cell's directions can hit. wf_shadow_point_bins (kernels_wf_trace.hip) then decides a point-light shadow
// ray by testing its cell's list instead of walking a tree. Built once per scene and light set, on the device.
//
// What a cell must hold (DESIGN.md "Point-light shadow rays by light-binned triangles"). A ray (S, d) toward light L, d = normalize(L - S) rounded, can
// be found to hit triangle T only at a point P = S + d t within e of a point Q of T, e = 3.2e-5 Mtot + 2 dev
// (pr_tri_setup's bound of hitTriangle's slack with the magnitudes of every ray origin and the light: Mtot; the extra
// 0.2e-5 Mtot covers the ray passing the light within a few eps |L - S|). Seen from L, Q lies within the angle
// e / |Q - L| of -d. Each face's triangle is clipped to the face's frustum widened to |x|, |y| <= 1.01 w, projected,
// and binned to the cells its projection covers widened by that angle in cells; |Q - L| >= w >= wmin, the clipped
// polygon's least depth. A triangle with wmin < r0 = 0.01 Mtot or e >= 0.002 wmin on some face (then the angle, under
// 0.002, moves the projection by under 0.007 < 0.01: a point just across a face edge is still inside the widened
// frustum), with a non-finite vertex, or whose N is not perpendicular to its edges goes to the light's catch-all list.
#include <hip/hip_runtime.h>

#include "glsl_builtins.h"
#include "pb_overlap.h"
#include "pt_device.h"
#include "pt_shading.h"

using namespace glsl;

namespace ptk {

namespace {

constexpr int kScanThreads = 1024;

struct PbLayout {
  size_t info, hdr, cnt, tmp, ent, lrg, total;
  int cap, lrg_cap;
};
// entries a light's lists have room for. Measured on the bench scene (30 633 triangles, lights 0.3 .. 1 from the
// geometry), the largest light's entries per triangle at R = 32 / 64 / 128: 4.6 / 8.9 / 20.0 by the polygon (the test
// scenes: at most 13.3 at R = 64), 8.5 / 25 / 84 by the box; the per-cell term leaves room for the few large
// triangles that cover whole faces. A light whose entries do not fit gets no bins (its rays walk).
inline PbLayout pb_layout(int ntris, int nl, int R, int tight) {
  const size_t ncell1 = (size_t)6 * R * R + 1, al = 256;
  auto up = [&](size_t v) { return (v + al - 1) / al * al; };
  PbLayout l{};
  const size_t per_tri = tight ? (R > 64 ? 48 : 24) : (R > 64 ? 96 : 32);
  const size_t cap = per_tri * (size_t)std::max(ntris, 1) + 8 * ncell1;
  l.cap = (int)std::min<size_t>(cap, (size_t)1 << 28);
  l.info = 0;
  l.cnt = up((size_t)(kPointBins + 1) * kPointBinsInfo * sizeof(int));  // (+1: the scene's magnitude)
  l.hdr = l.cnt + up((size_t)nl * ncell1 * sizeof(int));
  l.tmp = l.hdr + up((size_t)nl * ncell1 * sizeof(int2));
  l.ent = l.tmp + up((size_t)l.cap * sizeof(uint4));
  // the large boxes' work list (pb_bin_large): a record per (triangle, face), so it cannot overflow
  l.lrg_cap = (int)std::min<size_t>((size_t)6 * (size_t)std::max(ntris, 1), (size_t)1 << 30);
  l.lrg = l.ent + up((size_t)nl * l.cap * sizeof(uint2));
  l.total = l.lrg + up((size_t)nl * l.lrg_cap * sizeof(uint32_t));
  return l;
}

struct PbBuild {
  SceneDev sc;
  int* info;     // kPointBins x kPointBinsInfo, then [0] of the next record: float bits of the scene's magnitude
  int* cnt;      // nl x (ncell + 1): cell counts, then the scatter's fill counts
  int2* hdr;     // nl x (ncell + 1)
  uint4* tmp;    // cap: one light's entries in scatter order (the lights are scattered and sorted one after another)
  uint2* ent;    // nl x cap: entries (PointBinsDev), each cell ascending by near
  int R, nl, cap;
  int tight;     // cells by the projected polygon (pb_overlap.h), 0: every cell of its box
  int l0;        // the first light of the grid (the scatter's and the sort's grids have one light; so does every
                 // kernel of a one-light rebuild, launch_point_bins_rebuild_light)
  int ln;        // lights pb_lights sets up, from l0
  uint32_t* lrg; // nl x lrg_cap: per light the (triangle << 3 | face) records of the boxes pb_bin left to pb_bin_large;
                 // their count is info[l][7]
  int lrg_cap;
  int large_min; // a box of more cells than this is left to pb_bin_large (kPbLargeCells; INT_MAX: none is)
};

// a (triangle, face) box of more cells than one wave's worth is binned by a wave, not by one thread
constexpr int kPbLargeCells = 64;

// largest finite coordinate magnitude of the triangles' vertices (a positive float's bits order as an int's)
__global__ void __launch_bounds__(256) pb_extent(PbBuild b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  float m = 0.0f;
  if (i < b.sc.ntris) {
    const TriGeom tg = tri_load(b.sc.tri_geom, i);
    const float c[9] = {tg.a.x, tg.a.y, tg.a.z, tg.b.x, tg.b.y, tg.b.z, tg.c.x, tg.c.y, tg.c.z};
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (fabsf(c[k]) <= 3.0e38f) m = fmaxf(m, fabsf(c[k]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(b.info + kPointBins * kPointBinsInfo, __float_as_int(m));
}

__global__ void __launch_bounds__(64) pb_lights(PbBuild b) {
  if ((int)threadIdx.x >= b.ln) return;
  const int l = b.l0 + threadIdx.x;
  if (l >= b.nl) return;
  int* f = b.info + l * kPointBinsInfo;
  const float* lp = b.sc.lights + 6 * l;
  const float ms = __int_as_float(b.info[kPointBins * kPointBinsInfo]);
  const float ml = fmaxf(fabsf(lp[0]), fmaxf(fabsf(lp[1]), fabsf(lp[2])));
  const bool ok = fabsf(lp[0]) <= 3.0e38f && fabsf(lp[1]) <= 3.0e38f && fabsf(lp[2]) <= 3.0e38f;
  f[0] = ok ? 0 : 1;
  f[1] = 0;
  f[2] = __float_as_int(lp[0]);
  f[3] = __float_as_int(lp[1]);
  f[4] = __float_as_int(lp[2]);
  f[5] = __float_as_int(ok ? ms + ml : 0.0f);
}

constexpr uint32_t kBoxEmpty = 0x000000ffu;  // x0 = 255 > x1 = 0

// Triangle i of light l: the triangle's cell box and near bound on each face, or the catch-all list. SCATTER = false
// counts the cells, true writes the entries (the same arithmetic, so the same cells).
// LARGE = false (pb_bin, one thread per triangle): the cells of every face's box, but a box of more than
// b.large_min cells is left to pb_bin_large: the count pass appends (triangle, face) to the light's work list, the
// scatter pass skips it (the list is still there). LARGE = true (pb_bin_large, one wave per record, every lane with
// the same i): face fc_only alone, the lanes striding over its box's cells. Both run this one body, so a cell is
// kept, and its entry formed, by the same arithmetic whoever emits it: the set of entries is the serial loop's, and
// pb_sort's (near, triangle) order makes the lists identical.
template <bool SCATTER, bool LARGE>
__device__ __forceinline__ void pb_tri(const PbBuild& b, int i, int l, int fc_only, int lane) {
  int* f = b.info + l * kPointBinsInfo;
  const int R = b.R, ncell = 6 * R * R;
  int* cnt = b.cnt + (size_t)l * (ncell + 1);
  const int2* hdr = b.hdr + (size_t)l * (ncell + 1);
  uint4* tmp = b.tmp;
  auto emit = [&](int cell, float near, uint32_t sub) {
    const int slot = atomicAdd(cnt + cell, 1);
    if (SCATTER) {
      const int pos = hdr[cell].x + slot;
      if (pos >= 0 && pos < b.cap) tmp[pos] = make_uint4((uint32_t)i, __float_as_uint(near), sub, 0u);
    }
  };
  const TriGeom tg = tri_load(b.sc.tri_geom, i);
  const v3 N = xyz(tg.n), v[3] = {xyz(tg.a), xyz(tg.b), xyz(tg.c)};
  const float big = 3.0e38f;
  const bool nfin = fabsf(N.x) <= big && fabsf(N.y) <= big && fabsf(N.z) <= big;  // (false for NaN too)
  // a triangle in no leaf is never tested by the reference; with a non-finite N hitTriangle rejects every ray
  if (b.sc.tri_leaf[i] < 0 || !nfin) return;
  const v3 L = mk(__int_as_float(f[2]), __int_as_float(f[3]), __int_as_float(f[4]));
  const float Mtot = __int_as_float(f[5]);
  bool fin = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) fin = fin && fabsf(v[k].x) <= big && fabsf(v[k].y) <= big && fabsf(v[k].z) <= big;
  const v3 E[3] = {sub(v[1], v[0]), sub(v[2], v[1]), sub(v[0], v[2])};
  bool perp = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) perp = perp && fabsf(dot(N, E[k])) <= 1.0e-3f * length(E[k]);
  const float dev = fmaxf(fabsf(dot(N, E[0])), fabsf(dot(N, E[2])));  // the vertices' distance from N.x = N.p1
  const float e = 3.2e-5f * Mtot + 2.0f * dev, r0 = 0.01f * Mtot;
  bool catchall = !fin || !perp || !(e == e);
  // every point of the triangle lies at least ds from the light: its distance from the centroid's sphere
  const v3 c = muls(add(add(v[0], v[1]), v[2]), 1.0f / 3.0f);
  const float rad = fmaxf(length(sub(v[0], c)), fmaxf(length(sub(v[1], c)), length(sub(v[2], c))));
  const float ds = fmaxf(length(sub(c, L)) - rad * 1.00001f, 0.0f);
  uint32_t box[6];
  float nearf[6], ext[6][4], fwf[6];  // per face: cell box, near bound, the widened projection's extent in cell
                                      // coordinates, the widening
  float3 A[16], B[16];
  // the triangle clipped to face fc's widened frustum, in A: vertices (x, y, w)
  auto clip_face = [&](int fc) {
    const int a = fc >> 1;
    const float sg = (fc & 1) ? -1.0f : 1.0f;
    for (int k = 0; k < 3; ++k) {
      const float q[3] = {v[k].x - L.x, v[k].y - L.y, v[k].z - L.z};
      A[k] = make_float3(q[(a + 1) % 3], q[(a + 2) % 3], sg * q[a]);
    }
    int n = clip_plane(A, 3, B, 0, 1.0f);
    n = clip_plane(B, n, A, 0, -1.0f);
    n = clip_plane(A, n, B, 1, 1.0f);
    return clip_plane(B, n, A, 1, -1.0f);
  };
  // cell coordinate of the direction (x, y, w): the cell is floor((x / w + 1) R / 2) (wf_shadow_point_bins)
  auto cell_x = [&](const float3& p) { return (p.x / p.z + 1.0f) * 0.5f * (float)R; };
  auto cell_y = [&](const float3& p) { return (p.y / p.z + 1.0f) * 0.5f * (float)R; };
  for (int fc = 0; fc < 6 && !catchall; ++fc) {
    box[fc] = kBoxEmpty;
    nearf[fc] = 0.0f;
    fwf[fc] = 0.0f;
    const int n = clip_face(fc);
    if (n <= 0) continue;  // nothing of it in this face's widened frustum
    float x0 = 3.0e38f, y0 = 3.0e38f, x1 = -3.0e38f, y1 = -3.0e38f, wmin = 3.0e38f;
    bool bad = false;
    for (int k = 0; k < n; ++k) {
      const float w = A[k].z;
      const float px = cell_x(A[k]), py = cell_y(A[k]);
      bad = bad || !(w > 0.0f) || !(px == px && py == py);
      wmin = fminf(wmin, w);
      x0 = fminf(x0, px); x1 = fmaxf(x1, px);
      y0 = fminf(y0, py); y1 = fmaxf(y1, py);
    }
    if (bad || wmin < r0 || !(e < 0.002f * wmin)) {
      catchall = true;
      break;
    }
    // the angle e / wmin moves a direction's x / w by under 3.5 times itself (w >= |direction| / sqrt 3 on its face
    // and just across its edges); 0.02 of a cell for the rounding of both sides' cell coordinates
    const float fw = 3.5f * (e / wmin) * 0.5f * (float)R + 0.02f;
    const float lim = 1.0e6f;
    const int cx0 = max((int)floorf(fmaxf(x0 - fw, -lim)), 0), cx1 = min((int)floorf(fminf(x1 + fw, lim)), R - 1);
    const int cy0 = max((int)floorf(fmaxf(y0 - fw, -lim)), 0), cy1 = min((int)floorf(fminf(y1 + fw, lim)), R - 1);
    if (cx0 > cx1 || cy0 > cy1) continue;  // only in the widened rim
    box[fc] = (uint32_t)cx0 | ((uint32_t)cx1 << 8) | ((uint32_t)cy0 << 16) | ((uint32_t)cy1 << 24);
    ext[fc][0] = fmaxf(x0 - fw, -lim); ext[fc][1] = fminf(x1 + fw, lim);
    ext[fc][2] = fmaxf(y0 - fw, -lim); ext[fc][3] = fminf(y1 + fw, lim);
    fwf[fc] = fw;
    // a point the ray can be found to hit lies within e of a point of the triangle inside this face's frustum, which
    // is at least max(ds, wmin) from the light
    nearf[fc] = fmaxf(fmaxf(ds, wmin) * 0.99999f - e, 0.0f);
  }
  if (catchall) {
    if (!LARGE) emit(ncell, 0.0f, 0xff00ff00u);  // (no record names a catch-all triangle)
    return;
  }
  for (int fc = 0; fc < 6; ++fc) {
    if (LARGE && fc != fc_only) continue;
    const uint32_t bx = box[fc];
    const int cx0 = bx & 255u, cx1 = (bx >> 8) & 255u, cy0 = (bx >> 16) & 255u, cy1 = bx >> 24;
    if (cx0 > cx1) continue;
    const int bw = cx1 - cx0 + 1, ncells = bw * (cy1 - cy0 + 1);
    if (LARGE != (ncells > b.large_min)) {  // the other kernel's box
      if (!LARGE && !SCATTER) {
        const int slot = atomicAdd(f + 7, 1);
        if (slot < b.lrg_cap) b.lrg[(size_t)l * b.lrg_cap + slot] = ((uint32_t)i << 3) | (uint32_t)fc;
      }
      continue;
    }
    // tight: of the box's cells only those the projected polygon, widened by fw, reaches (pb_overlap.h); the box's
    // every cell when it has at most two or the polygon is degenerate (edges.n = 0 keeps all)
    PbEdges edges;
    edges.n = 0;
    if (b.tight && (cx1 - cx0 + 1) * (cy1 - cy0 + 1) > 2) {
      const int n = clip_face(fc);  // (the same arithmetic as above: the same polygon)
      float px[kPbMaxVerts], py[kPbMaxVerts];
      for (int k = 0; k < n && k < kPbMaxVerts; ++k) {
        px[k] = cell_x(A[k]);
        py[k] = cell_y(A[k]);
      }
      pb_edges(px, py, n, &edges);
    }
    // the extent inside each cell in 1 / 256 of a cell: (x0, x1, y0, y1), 8 bits each; pb_sort keeps the high 4
    auto q = [](float v) { return (uint32_t)min(max((int)floorf(v * 256.0f), 0), 255); };
    auto cell = [&](int cx, int cy) {
      if (pb_cell_kept(edges, fwf[fc], cx, cy, R))
        emit((fc * R + cy) * R + cx, nearf[fc],
             q(ext[fc][0] - (float)cx) | (q(ext[fc][1] - (float)cx) << 8) | (q(ext[fc][2] - (float)cy) << 16) |
                 (q(ext[fc][3] - (float)cy) << 24));
    };
    if (LARGE) {
      for (int c = lane; c < ncells; c += 64) cell(cx0 + c % bw, cy0 + c / bw);
    } else {
      for (int cy = cy0; cy <= cy1; ++cy)
        for (int cx = cx0; cx <= cx1; ++cx) cell(cx, cy);
    }
  }
}

// One thread per (triangle, light blockIdx.y + l0).
template <bool SCATTER>
__global__ void __launch_bounds__(256) pb_bin(PbBuild b) {
  const int i = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y + b.l0;
  if (i >= b.sc.ntris) return;
  if (b.info[l * kPointBinsInfo]) return;  // no usable bins for this light
  pb_tri<SCATTER, false>(b, i, l, 0, 0);
}

// One wave per record of light blockIdx.y + l0's work list, the grid's waves striding over the records (their count
// is known on the device only: info[l][7], complete since the count pass's pb_bin ended).
constexpr int kPbLargeBlocks = 256;
template <bool SCATTER>
__global__ void __launch_bounds__(256) pb_bin_large(PbBuild b) {
  const int l = blockIdx.y + b.l0;
  const int* f = b.info + l * kPointBinsInfo;
  if (f[0]) return;
  const int nrec = min(f[7], b.lrg_cap);
  const int lane = threadIdx.x & 63, nw = gridDim.x * 4;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < nrec; r += nw) {
    const uint32_t rec = b.lrg[(size_t)l * b.lrg_cap + r];
    const int i = (int)(rec >> 3), fc = (int)(rec & 7u);
    if (i < b.sc.ntris && fc < 6) pb_tri<SCATTER, true>(b, i, l, fc, lane);
  }
}

// One block per light (blockIdx.x + l0): headers (first entry, entries) from the cell counts, which are zeroed for the scatter; a
// light whose entries exceed `cap` gets no bins.
__global__ void __launch_bounds__(kScanThreads) pb_scan(PbBuild b) {
  __shared__ int part[kScanThreads];
  const int l = blockIdx.x + b.l0, n1 = 6 * b.R * b.R + 1, t = threadIdx.x;
  int* cnt = b.cnt + (size_t)l * n1;
  int2* hdr = b.hdr + (size_t)l * n1;
  const int per = (n1 + kScanThreads - 1) / kScanThreads, lo = min(t * per, n1), hi = min(lo + per, n1);
  long long sum = 0;
  for (int c = lo; c < hi; ++c) sum += cnt[c];
  part[t] = (int)min(sum, (long long)0x3fffffff);
  __syncthreads();
  for (int o = 1; o < kScanThreads; o <<= 1) {  // inclusive scan (saturating: an overflow stays one)
    const int add = t >= o ? part[t - o] : 0;
    __syncthreads();
    part[t] = min(part[t] + add, 0x3fffffff);
    __syncthreads();
  }
  const int total = part[kScanThreads - 1];
  int off = t > 0 ? part[t - 1] : 0;
  for (int c = lo; c < hi; ++c) {
    const int k = cnt[c];
    hdr[c] = make_int2(off, k);
    if (c == n1 - 1) b.info[l * kPointBinsInfo + 6] = k;  // the catch-all list's entries
    off = min(off + k, 0x3fffffff);
    cnt[c] = 0;
  }
  if (t == 0) {
    int* f = b.info + l * kPointBinsInfo;
    f[1] = total;
    if (total > b.cap) f[0] = 1;
  }
}

// One wave per cell: its entries from scatter order into ascending (near, triangle) order, by rank, packed to the 8
// bytes the trace kernel reads: near's high 16 bits (near >= 0: a lower bound that keeps the order) and the sub-cell
// box in 1 / 16 of a cell (the floor of the scatter's 1 / 256: floor(floor(256 v) / 16) = floor(16 v)).
__global__ void __launch_bounds__(256) pb_sort(PbBuild b) {
  const int l = blockIdx.y + b.l0, n1 = 6 * b.R * b.R + 1;
  const int cell = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (cell >= n1 || b.info[l * kPointBinsInfo]) return;
  const int2 h = b.hdr[(size_t)l * n1 + cell];
  const uint4* src = b.tmp + h.x;
  uint2* dst = b.ent + (size_t)l * b.cap + h.x;
  for (int i = lane; i < h.y; i += 64) {
    const uint4 me = src[i];
    int rank = 0;
    for (int j = 0; j < h.y; ++j) {
      const uint4 o = src[j];
      rank += (o.y < me.y || (o.y == me.y && o.x < me.x)) ? 1 : 0;
    }
    const uint32_t sb = me.z;
    const uint32_t box16 = ((sb >> 4) & 15u) | (((sb >> 12) & 15u) << 4) | (((sb >> 20) & 15u) << 8) | ((sb >> 28) << 12);
    dst[rank] = make_uint2(me.x, (me.y >> 16) | (box16 << 16));
  }
}

// (a record packs the triangle into 29 bits)
inline int pb_large_min(int ntris) { return ntris < (1 << 29) ? kPbLargeCells : 0x7fffffff; }

}  // namespace

size_t point_bins_bytes(int ntris, int nl, int R, int tight) { return pb_layout(ntris, nl, R, tight).total; }

int launch_point_bins_build(const SceneDev& sc, int nl, int R, int tight, void* base, PointBinsDev* out,
                            hipStream_t s) {
  if (nl < 1 || nl > kPointBins || R < 1 || R > kPointBinsMaxR || !base || !sc.lights || !sc.tri_leaf)
    return (int)hipErrorInvalidValue;
  const PbLayout lay = pb_layout(sc.ntris, nl, R, tight);
  char* c = (char*)base;
  PbBuild b{sc, (int*)(c + lay.info), (int*)(c + lay.cnt), (int2*)(c + lay.hdr), (uint4*)(c + lay.tmp),
            (uint2*)(c + lay.ent), R, nl, lay.cap, tight ? 1 : 0, 0, nl, (uint32_t*)(c + lay.lrg), lay.lrg_cap,
            pb_large_min(sc.ntris)};
  hipError_t e = hipMemsetAsync(base, 0, lay.hdr, s);  // info and the cell counts
  if (e != hipSuccess) return (int)e;
  const int gt = (sc.ntris + 255) / 256, n1 = 6 * R * R + 1;
  if (gt > 0) hipLaunchKernelGGL(pb_extent, dim3(gt), dim3(256), 0, s, b);
  hipLaunchKernelGGL(pb_lights, dim3(1), dim3(64), 0, s, b);
  if (gt > 0) hipLaunchKernelGGL(pb_bin<false>, dim3(gt, nl), dim3(256), 0, s, b);
  if (gt > 0) hipLaunchKernelGGL(pb_bin_large<false>, dim3(kPbLargeBlocks, nl), dim3(256), 0, s, b);
  hipLaunchKernelGGL(pb_scan, dim3(nl), dim3(kScanThreads), 0, s, b);  // (b.l0 = 0: every light)
  for (b.l0 = 0; b.l0 < nl; ++b.l0) {  // one scatter buffer serves every light in turn
    if (gt > 0) hipLaunchKernelGGL(pb_bin<true>, dim3(gt, 1), dim3(256), 0, s, b);
    if (gt > 0) hipLaunchKernelGGL(pb_bin_large<true>, dim3(kPbLargeBlocks, 1), dim3(256), 0, s, b);
    hipLaunchKernelGGL(pb_sort, dim3((n1 + 3) / 4, 1), dim3(256), 0, s, b);
  }
  *out = PointBinsDev{b.hdr, b.ent, b.info, R, nl, lay.cap};
  return (int)hipGetLastError();
}

// The lists of light l alone, in place, around the position sc.lights holds for it now: the full build's kernels
// restricted to that light (its info record, cell counts, headers and entry section; the scatter buffer is shared and
// the stream orders its users). The scene's magnitude (pb_extent) is a function of the triangles, which have not
// changed, and stays. The other lights' sections are not touched. The caller orders this after every draw that reads
// the bins (capi_draw_pt.hip point_bins_for).
int launch_point_bins_rebuild_light(const SceneDev& sc, int nl, int R, int tight, void* base, int l, hipStream_t s) {
  if (nl < 1 || nl > kPointBins || R < 1 || R > kPointBinsMaxR || !base || !sc.lights || !sc.tri_leaf || l < 0 ||
      l >= nl)
    return (int)hipErrorInvalidValue;
  const PbLayout lay = pb_layout(sc.ntris, nl, R, tight);
  char* c = (char*)base;
  PbBuild b{sc, (int*)(c + lay.info), (int*)(c + lay.cnt), (int2*)(c + lay.hdr), (uint4*)(c + lay.tmp),
            (uint2*)(c + lay.ent), R, nl, lay.cap, tight ? 1 : 0, l, 1, (uint32_t*)(c + lay.lrg), lay.lrg_cap,
            pb_large_min(sc.ntris)};
  const int gt = (sc.ntris + 255) / 256, n1 = 6 * R * R + 1;
  // this light's cell counts (the last scatter left its fill counts there) and its info record
  hipError_t e = hipMemsetAsync(b.cnt + (size_t)l * n1, 0, (size_t)n1 * sizeof(int), s);
  if (e == hipSuccess) e = hipMemsetAsync(b.info + l * kPointBinsInfo, 0, kPointBinsInfo * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(pb_lights, dim3(1), dim3(64), 0, s, b);
  if (gt > 0) hipLaunchKernelGGL(pb_bin<false>, dim3(gt, 1), dim3(256), 0, s, b);
  if (gt > 0) hipLaunchKernelGGL(pb_bin_large<false>, dim3(kPbLargeBlocks, 1), dim3(256), 0, s, b);
  hipLaunchKernelGGL(pb_scan, dim3(1), dim3(kScanThreads), 0, s, b);
  if (gt > 0) hipLaunchKernelGGL(pb_bin<true>, dim3(gt, 1), dim3(256), 0, s, b);
  if (gt > 0) hipLaunchKernelGGL(pb_bin_large<true>, dim3(kPbLargeBlocks, 1), dim3(256), 0, s, b);
  hipLaunchKernelGGL(pb_sort, dim3((n1 + 3) / 4, 1), dim3(256), 0, s, b);
  return (int)hipGetLastError();
}

// info[l][0] = 2: light l moved and its lists are pending; both trace kernels walk for any non-zero value
int launch_point_bins_mark_moved(const PointBinsDev& pb, int l, hipStream_t s) {
  if (!pb.info || l < 0 || l >= pb.nl) return (int)hipErrorInvalidValue;
  return (int)hipMemsetD32Async((hipDeviceptr_t)(pb.info + l * kPointBinsInfo), 2, 1, s);
}

// where light l's headers and entries lie in a build's allocation (pt_debug_point_bins_read)
void point_bins_sections(int ntris, int nl, int R, int tight, int l, size_t* hdr_off, size_t* ent_off) {
  const PbLayout lay = pb_layout(ntris, nl, R, tight);
  *hdr_off = lay.hdr + (size_t)l * ((size_t)6 * R * R + 1) * sizeof(int2);
  *ent_off = lay.ent + (size_t)l * lay.cap * sizeof(uint2);
}

}  // namespace ptk

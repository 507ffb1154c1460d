// host_trees.cpp — the host tree builder (host_trees.h): the reference tree packed for the kernels, the SAH trees
// built for speed (binned / sweep SAH, treelet restructuring, the 4-wide collapse, fine leaves) and the checks of
// pt_tree_check. Plain C++17 over std::vector: no HIP header and no library state, so it also builds with a host
// compiler alone into a stand-alone program (tools/host_trees_check.cpp).
#include "host_trees.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>

#include "../../include/ptsvgf.h"

namespace ptk {

static int err(std::string* msg, int code, const char* m) {
  if (msg) *msg = m;
  return code;
}

// ---------------------------------------------------------------- packing ---
namespace {
struct NodeRaw {
  int left, right, n, index;
  float AA[3], BB[3];
};
}  // namespace

// *need: deepest interior level (root = 1) = the most stack entries a walk holds
int pack_bvh(const float* node_enc, int nnodes, std::vector<float4>& out, int* root_ref, int ntris, int* need,
             std::string* msg) {
  if (nnodes < 2) return err(msg, PT_ERR_FORMAT, "BVH needs the dummy node 0 and a root node 1");
  std::vector<NodeRaw> nd(nnodes);
  for (int i = 0; i < nnodes; ++i) {
    const float* f = node_enc + (size_t)i * 12;
    nd[i].left = (int)f[0];
    nd[i].right = (int)f[1];
    nd[i].n = (int)f[3];
    nd[i].index = (int)f[4];
    for (int k = 0; k < 3; ++k) { nd[i].AA[k] = f[6 + k]; nd[i].BB[k] = f[9 + k]; }
  }
  std::vector<int> idx(nnodes, -1);
  std::vector<int> order;
  // iterative DFS (depth check: stack needs one slot per interior level)
  struct Item { int id, depth; };
  std::vector<Item> st;
  auto leaf_ref = [&](int id, int* ref) -> int {
    const NodeRaw& n = nd[id];
    if (n.n > 15) return err(msg, PT_ERR_FORMAT, "BVH leaf holds more than 15 triangles");
    if (n.index < 0 || n.index + n.n > ntris) return err(msg, PT_ERR_FORMAT, "BVH leaf range out of bounds");
    *ref = -(n.index * 16 + n.n) - 1;
    return PT_OK;
  };
  *need = 0;
  if (nd[1].n > 0) {
    int r;
    if (leaf_ref(1, &r) != PT_OK) return PT_ERR_FORMAT;
    *root_ref = r;
    out.clear();
    return PT_OK;
  }
  st.push_back({1, 1});
  while (!st.empty()) {
    Item it = st.back();
    st.pop_back();
    // the reference walks with int stack[256] (path_tracing.frag:378); deeper trees are undefined there
    if (it.depth >= kRefStack) return err(msg, PT_ERR_FORMAT, "BVH deeper than the reference's stack[256]");
    *need = std::max(*need, it.depth);
    idx[it.id] = (int)order.size();
    order.push_back(it.id);
    const NodeRaw& n = nd[it.id];
    if (n.left <= 0 || n.right <= 0 || n.left >= nnodes || n.right >= nnodes)
      return err(msg, PT_ERR_FORMAT, "BVH interior node with an invalid child");
    if (nd[n.right].n <= 0) st.push_back({n.right, it.depth + 1});
    if (nd[n.left].n <= 0) st.push_back({n.left, it.depth + 1});
  }
  out.assign(order.size() * 4, float4{0, 0, 0, 0});
  for (size_t k = 0; k < order.size(); ++k) {
    const NodeRaw& n = nd[order[k]];
    const NodeRaw& L = nd[n.left];
    const NodeRaw& R = nd[n.right];
    int rl, rr;
    if (L.n > 0) { if (leaf_ref(n.left, &rl) != PT_OK) return PT_ERR_FORMAT; } else rl = idx[n.left];
    if (R.n > 0) { if (leaf_ref(n.right, &rr) != PT_OK) return PT_ERR_FORMAT; } else rr = idx[n.right];
    float4* q = &out[4 * k];
    q[0] = float4{L.AA[0], L.AA[1], L.AA[2], L.BB[0]};
    q[1] = float4{L.BB[1], L.BB[2], R.AA[0], R.AA[1]};
    q[2] = float4{R.AA[2], R.BB[0], R.BB[1], R.BB[2]};
    float a, b;
    memcpy(&a, &rl, 4);
    memcpy(&b, &rr, 4);
    q[3] = float4{a, b, 0, 0};
  }
  *root_ref = 0;
  return PT_OK;
}

// ------------------------------------------------------ binned SAH trees ---
// Trees whose answer does not depend on their shape, built for speed instead of
// reference compatibility (the reference's buildBVHwithSAH caps costs at INF =
// 114514 and falls back to median-x splits near the root of a 30k-triangle
// scene):
//  * the G-buffer tree over the raster triangles: its walk keeps the closest t
//    with ties to the lower original index and widened boxes only cull, so any
//    tree gives the same pixel;
//  * the any-hit (shadow) tree over the REFERENCE tree's leaves: its leaves are
//    exactly the reference leaves (same triangle ranges, same boxes) and every
//    interior box is an exact min/max union of them. A triangle is tested iff its
//    leaf box passes the slab test in either tree (an enclosing box passes
//    whenever an enclosed one does: slab rounding is monotone), so shadow
//    verdicts are those of the reference tree.
// A primitive is one triangle (G-buffer) or one reference leaf (any-hit).
namespace {
struct SahPrim {
  float lo[3], hi[3];
  int weight;  // triangles it holds (SAH intersection cost)
  int ref;     // leaf ref it emits alone (any-hit tree), or its index (G-buffer)
};
struct SahNode {
  float lo[3], hi[3];
  int left = -1, right = -1;  // children (interior)
  int first = 0, n = 0;       // primitive range (leaf)
  int ref = 0;                // leaf: its ref, when `direct` (a fine leaf of refine_leaves) instead of leaf_ref()
  bool direct = false;
  bool keep = false;          // interior node whose box must be tested as is (a refined reference leaf): pack_wide
};
}  // namespace

static float sah_area(const float* lo, const float* hi) {
  const float dx = std::max(hi[0] - lo[0], 0.0f), dy = std::max(hi[1] - lo[1], 0.0f), dz = std::max(hi[2] - lo[2], 0.0f);
  return dx * dy + dy * dz + dz * dx;
}

// Exact (full-sweep) SAH split of pr[l, r): per axis the primitives sorted by centroid, every cut priced; pr is
// left sorted along the best axis and *m is the cut. Returns the best cost (INFINITY: no split).
static float sah_sweep(std::vector<SahPrim>& pr, int l, int r, int* m) {
  const int n = r - l;
  std::vector<float> rarea((size_t)n);
  std::vector<int> rw((size_t)n);
  float best = INFINITY;
  int bax = -1, bcut = 0;
  auto by_axis = [&](int a) {
    std::sort(pr.begin() + l, pr.begin() + r, [a](const SahPrim& x, const SahPrim& y) {
      const float cx = x.lo[a] + x.hi[a], cy = y.lo[a] + y.hi[a];
      return cx < cy || (cx == cy && x.ref < y.ref);
    });
  };
  for (int a = 0; a < 3; ++a) {
    by_axis(a);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int w = 0;
    for (int i = n - 1; i >= 1; --i) {
      const SahPrim& q = pr[l + i];
      for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], q.lo[k]); hi[k] = std::max(hi[k], q.hi[k]); }
      w += q.weight;
      rarea[i] = sah_area(lo, hi);
      rw[i] = w;
    }
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    w = 0;
    for (int i = 0; i + 1 < n; ++i) {
      const SahPrim& q = pr[l + i];
      for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], q.lo[k]); hi[k] = std::max(hi[k], q.hi[k]); }
      w += q.weight;
      const float c = sah_area(lo, hi) * w + rarea[i + 1] * rw[i + 1];
      if (c < best) { best = c; bax = a; bcut = i + 1; }
    }
  }
  if (bax < 0) return INFINITY;
  if (bax != 2) by_axis(bax);
  *m = l + bcut;
  return best;
}

// Build-quality switch (PTSVGF_SAH_SWEEP, read once): 1 (default) = exact sweep SAH, 0 = 16-bin SAH
// (measured 4K 6.885 -> 6.79 ms, 1080p 2.72 -> 2.64 ms with the sweep, tools/exp_env_ab.sh).
static bool sah_use_sweep() {
  static const bool on = [] {
    const char* e = getenv("PTSVGF_SAH_SWEEP");
    return !e || atoi(e) != 0;
  }();
  return on;
}

// 16-bin SAH over primitive centroids (cost: 1 per node visit, `weight` per primitive test), or the exact sweep.
// max_leaf: the most primitives a leaf may hold (leaves also stop at 15 triangles, the leaf ref's limit).
static int ceil_log2(int n) {
  int k = 0;
  while ((1 << k) < n) ++k;
  return k;
}

// depth: this node's level (root = 1). Once the SAH splits could take the tree past the LDS stack, the rest of the
// range is halved by index (sorted along the widest centroid axis), so every tree fits the stack: interior levels
// stay below kStack - 1 whatever the geometry (coincident centroids make SAH peel one primitive per level).
// reserve: stack levels kept free below the leaves (the any-hit tree's fine subtrees, refine_leaves)
static int sah_build(std::vector<SahPrim>& pr, int l, int r, int max_leaf, std::vector<SahNode>& nodes, int depth = 1,
                     int reserve = 0) {
  const int id = (int)nodes.size();
  nodes.emplace_back();
  SahNode nd;
  float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int a = 0; a < 3; ++a) { nd.lo[a] = INFINITY; nd.hi[a] = -INFINITY; }
  int w = 0;
  for (int i = l; i < r; ++i) {
    for (int a = 0; a < 3; ++a) {
      nd.lo[a] = std::min(nd.lo[a], pr[i].lo[a]);
      nd.hi[a] = std::max(nd.hi[a], pr[i].hi[a]);
      const float c = 0.5f * (pr[i].lo[a] + pr[i].hi[a]);
      clo[a] = std::min(clo[a], c);
      chi[a] = std::max(chi[a], c);
    }
    w += pr[i].weight;
  }
  const int n = r - l;
  constexpr int kBins = 16;
  float best = INFINITY;
  int bax = -1, bsplit = 0, msweep = -1;
  const bool sweep = sah_use_sweep();
  if (sweep && n > 1) {
    best = sah_sweep(pr, l, r, &msweep);
    if (best < INFINITY) bax = 0;
  }
  if (!sweep && n > 1) {
    for (int a = 0; a < 3; ++a) {
      const float ext = chi[a] - clo[a];
      if (!(ext > 0.0f)) continue;
      float blo[kBins][3], bhi[kBins][3];
      int bw[kBins] = {0}, bn[kBins] = {0};
      for (int b = 0; b < kBins; ++b)
        for (int k = 0; k < 3; ++k) { blo[b][k] = INFINITY; bhi[b][k] = -INFINITY; }
      for (int i = l; i < r; ++i) {
        const float c = 0.5f * (pr[i].lo[a] + pr[i].hi[a]);
        const int b = std::min(kBins - 1, (int)((c - clo[a]) / ext * kBins));
        ++bn[b];
        bw[b] += pr[i].weight;
        for (int k = 0; k < 3; ++k) { blo[b][k] = std::min(blo[b][k], pr[i].lo[k]); bhi[b][k] = std::max(bhi[b][k], pr[i].hi[k]); }
      }
      float rlo[kBins][3], rhi[kBins][3];
      int rw[kBins], rn[kBins];
      for (int b = kBins - 1; b >= 0; --b) {
        for (int k = 0; k < 3; ++k) {
          rlo[b][k] = b + 1 < kBins ? std::min(rlo[b + 1][k], blo[b][k]) : blo[b][k];
          rhi[b][k] = b + 1 < kBins ? std::max(rhi[b + 1][k], bhi[b][k]) : bhi[b][k];
        }
        rw[b] = (b + 1 < kBins ? rw[b + 1] : 0) + bw[b];
        rn[b] = (b + 1 < kBins ? rn[b + 1] : 0) + bn[b];
      }
      float llo[3] = {INFINITY, INFINITY, INFINITY}, lhi[3] = {-INFINITY, -INFINITY, -INFINITY};
      int lw = 0, ln = 0;
      for (int b = 0; b + 1 < kBins; ++b) {
        for (int k = 0; k < 3; ++k) { llo[k] = std::min(llo[k], blo[b][k]); lhi[k] = std::max(lhi[k], bhi[b][k]); }
        lw += bw[b];
        ln += bn[b];
        if (ln == 0 || rn[b + 1] == 0) continue;
        const float c = sah_area(llo, lhi) * lw + sah_area(rlo[b + 1], rhi[b + 1]) * rw[b + 1];
        if (c < best) { best = c; bax = a; bsplit = b; }
      }
    }
  }
  const float area = sah_area(nd.lo, nd.hi);
  const bool fits = n <= max_leaf && w <= 15;
  if (n == 1 || (fits && (bax < 0 || !(area > 0.0f) || 1.0f + best / area >= (float)w))) {
    nd.first = l;
    nd.n = n;
    nodes[id] = nd;
    return id;
  }
  int m;
  if (depth + ceil_log2(n) + reserve >= kStack - 2) {  // depth cap: balanced halves from here on
    int ax = 0;
    for (int a = 1; a < 3; ++a)
      if (chi[a] - clo[a] > chi[ax] - clo[ax]) ax = a;
    std::sort(pr.begin() + l, pr.begin() + r, [ax](const SahPrim& x, const SahPrim& y) {
      const float cx = x.lo[ax] + x.hi[ax], cy = y.lo[ax] + y.hi[ax];
      return cx < cy || (cx == cy && x.ref < y.ref);
    });
    m = l + n / 2;
  } else if (sweep && msweep > l) {
    m = msweep;
  } else if (!sweep && bax >= 0) {
    const float ext = chi[bax] - clo[bax];
    m = (int)(std::partition(pr.begin() + l, pr.begin() + r, [&](const SahPrim& q) {
          const float c = 0.5f * (q.lo[bax] + q.hi[bax]);
          return std::min(kBins - 1, (int)((c - clo[bax]) / ext * kBins)) <= bsplit;
        }) - pr.begin());
  } else {
    m = l + n / 2;  // coincident centroids: halve the range
  }
  nd.left = sah_build(pr, l, m, max_leaf, nodes, depth + 1, reserve);
  nd.right = sah_build(pr, m, r, max_leaf, nodes, depth + 1, reserve);
  nodes[id] = nd;
  return id;
}

// Treelet restructuring of a built SahNode tree (PTSVGF_TREELET = passes, read once; default 1, 0 = off): for every interior node,
// bottom up, its treelet of up to 7 leaves (the root's descendants, the largest interior one opened first) is rebuilt
// as the binary tree of least SAH cost over those leaves (a dynamic program over the 127 leaf subsets), when that
// is cheaper. Boxes are unions again afterwards, so every walk's candidates stay the reference's (the containment
// argument of pack_wide); a tree that would grow past the stack's depth budget is left as it was.
// Bench scene (profiles/r06/treelet/): SAH cost / root area 121.56 -> 117.50 with one pass (117.00 with three); at 4K
// shadow visits -2.4 % / -3.1 % (default / surface view), bounce visits -1.0 % / -0.3 % (three passes: the surface
// view's shadow visits +0.4 %, so one pass); same bits; same box, three alternating repetitions: 227.7 / 228.4 / 227.6
// -> 225.8 / 228.1 / 227.7 fps at 4K (within noise), surface view 79.35 / 78.48 / 79.37 -> 80.02 / 80.63 / 80.13.
static int treelet_passes() {
  static const int n = [] {
    const char* e = getenv("PTSVGF_TREELET");
    return e ? std::max(0, atoi(e)) : 1;
  }();
  return n;
}

static void post_order(const std::vector<SahNode>& nodes, int root, std::vector<int>& order) {
  order.clear();
  std::vector<std::pair<int, bool>> st{{root, false}};
  while (!st.empty()) {
    auto [id, done] = st.back();
    st.pop_back();
    if (done || nodes[id].n > 0) { order.push_back(id); continue; }
    st.push_back({id, true});
    st.push_back({nodes[id].right, false});
    st.push_back({nodes[id].left, false});
  }
}

// SAH cost of node id's subtree (interior: its area + its children's; leaf: area x triangles), sah_build's model
static double sah_tree_cost(const std::vector<SahNode>& nodes, const std::vector<SahPrim>& pr, std::vector<double>& c) {
  std::vector<int> order;
  post_order(nodes, 0, order);
  c.assign(nodes.size(), 0.0);
  for (int id : order) {
    const SahNode& x = nodes[id];
    const double a = sah_area(x.lo, x.hi);
    if (x.n > 0) {
      int w = 0;
      for (int i = x.first; i < x.first + x.n; ++i) w += pr[i].weight;
      c[id] = a * w;
    } else {
      c[id] = a + c[x.left] + c[x.right];
    }
  }
  return c[0];
}

static int tree_depth(const std::vector<SahNode>& nodes) {
  int best = 0;
  std::vector<std::pair<int, int>> st{{0, 1}};
  while (!st.empty()) {
    auto [id, d] = st.back();
    st.pop_back();
    best = std::max(best, d);
    if (nodes[id].n == 0) {
      st.push_back({nodes[id].left, d + 1});
      st.push_back({nodes[id].right, d + 1});
    }
  }
  return best;
}

static void treelet_optimize(std::vector<SahNode>& nodes, const std::vector<SahPrim>& pr, int passes, int reserve,
                             double* sah_before = nullptr, double* sah_after = nullptr) {
  if (passes <= 0 || nodes.empty() || nodes[0].n > 0) {
    std::vector<double> c;
    const double v = nodes.empty() ? 0.0 : sah_tree_cost(nodes, pr, c) / std::max(1e-30, (double)sah_area(nodes[0].lo, nodes[0].hi));
    if (sah_before) *sah_before = v;
    if (sah_after) *sah_after = v;
    return;
  }
  const std::vector<SahNode> orig = nodes;
  constexpr int KMAX = 10;
  static const int K = [KMAX] {  // treelet leaves (PTSVGF_TREELET_LEAVES, 3..10, default 7)
    const char* e = getenv("PTSVGF_TREELET_LEAVES");
    return e ? std::min(KMAX, std::max(3, atoi(e))) : 7;
  }();
  std::vector<double> cost;
  const double before = sah_tree_cost(nodes, pr, cost);
  std::vector<int> order;
  for (int pass = 0; pass < passes; ++pass) {
    bool changed = false;
    post_order(nodes, 0, order);
    for (int r : order) {
      if (nodes[r].n > 0) continue;
      // its subtree may have changed below (children come first in post order)
      cost[r] = sah_area(nodes[r].lo, nodes[r].hi) + cost[nodes[r].left] + cost[nodes[r].right];
      int T[KMAX], nt = 2, I[KMAX], ni = 1;
      T[0] = nodes[r].left;
      T[1] = nodes[r].right;
      I[0] = r;
      while (nt < K) {  // open the largest interior treelet leaf
        int b = -1;
        float ba = -1.0f;
        for (int i = 0; i < nt; ++i)
          if (nodes[T[i]].n == 0) {
            const float a = sah_area(nodes[T[i]].lo, nodes[T[i]].hi);
            if (a > ba) { ba = a; b = i; }
          }
        if (b < 0) break;
        const int x = T[b];
        I[ni++] = x;
        T[b] = nodes[x].left;
        T[nt++] = nodes[x].right;
      }
      if (nt < 3) continue;
      const int full = (1 << nt) - 1;
      static thread_local std::vector<double> area(1 << KMAX), best(1 << KMAX);
      static thread_local std::vector<int> split(1 << KMAX);
      for (int S = 1; S <= full; ++S) {
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < nt; ++i)
          if (S >> i & 1)
            for (int k = 0; k < 3; ++k) {
              lo[k] = std::min(lo[k], nodes[T[i]].lo[k]);
              hi[k] = std::max(hi[k], nodes[T[i]].hi[k]);
            }
        area[S] = sah_area(lo, hi);
        if ((S & (S - 1)) == 0) {
          int i = 0;
          while (!(S >> i & 1)) ++i;
          best[S] = cost[T[i]];
          split[S] = 0;
          continue;
        }
        double b = INFINITY;
        int bp = 0;
        const int low = S & -S;  // P holds S's lowest leaf: each unordered split once
        for (int P = (S - 1) & S; P > 0; P = (P - 1) & S) {
          if (!(P & low)) continue;
          const double c = best[P] + best[S ^ P];
          if (c < b) { b = c; bp = P; }
        }
        best[S] = area[S] + b;
        split[S] = bp;
      }
      if (!(best[full] < cost[r] * (1.0 - 1e-6))) continue;
      // rebuild: the treelet's interior nodes I (r stays the root), leaves T
      int next = 1;
      std::function<int(int, bool)> make = [&](int S, bool root) -> int {
        if ((S & (S - 1)) == 0) {
          int i = 0;
          while (!(S >> i & 1)) ++i;
          return T[i];
        }
        const int id = root ? r : I[next++];
        const int L = make(split[S], false), R = make(S ^ split[S], false);
        SahNode nd = nodes[id];
        nd.n = 0;
        nd.left = L;
        nd.right = R;
        for (int k = 0; k < 3; ++k) {
          nd.lo[k] = std::min(nodes[L].lo[k], nodes[R].lo[k]);
          nd.hi[k] = std::max(nodes[L].hi[k], nodes[R].hi[k]);
        }
        nodes[id] = nd;
        cost[id] = sah_area(nd.lo, nd.hi) + cost[L] + cost[R];
        return id;
      };
      make(full, true);
      changed = true;
    }
    if (!changed) break;
  }
  const double after = sah_tree_cost(nodes, pr, cost);
  const int depth = tree_depth(nodes);
  const bool keep = depth + reserve < kStack - 2;
  if (!keep) nodes = orig;
  const double root_area = std::max(1e-30, (double)sah_area(orig[0].lo, orig[0].hi));
  if (sah_before) *sah_before = before / root_area;
  if (sah_after) *sah_after = (keep ? after : before) / root_area;
  if (getenv("PTSVGF_WIDE_STATS"))
    fprintf(stderr, "ptsvgf: treelet restructuring (%d passes): SAH cost / root area %.4f -> %.4f, depth %d%s\n", passes,
            before / std::max(1e-30, (double)sah_area(orig[0].lo, orig[0].hi)),
            after / std::max(1e-30, (double)sah_area(orig[0].lo, orig[0].hi)), depth,
            keep ? "" : " (too deep for the stack: not used)");
}

// Pack a SahNode tree in pack_bvh's layout (DFS order, 4 x float4 per interior node).
// leaf_ref(first, n) gives the ref of a leaf holding primitives [first, first + n).
static int pack_sah(const std::vector<SahNode>& nodes, const std::function<int(int, int)>& leaf_ref,
                    std::vector<float4>& out, int* root_ref, int* need, std::string* msg) {
  *need = 0;
  out.clear();
  if (nodes[0].n > 0) {
    *root_ref = leaf_ref(nodes[0].first, nodes[0].n);
    return PT_OK;
  }
  std::vector<int> idx(nodes.size(), -1), order;
  struct Item { int id, depth; };
  std::vector<Item> st{{0, 1}};
  while (!st.empty()) {
    const Item it = st.back();
    st.pop_back();
    if (it.depth >= kStack) return err(msg, PT_ERR_FORMAT, "SAH tree deeper than the traversal stack");
    *need = std::max(*need, it.depth);
    idx[it.id] = (int)order.size();
    order.push_back(it.id);
    const SahNode& n = nodes[it.id];
    if (nodes[n.right].n == 0) st.push_back({n.right, it.depth + 1});
    if (nodes[n.left].n == 0) st.push_back({n.left, it.depth + 1});
  }
  out.assign(order.size() * 4, float4{0, 0, 0, 0});
  for (size_t k = 0; k < order.size(); ++k) {
    const SahNode& n = nodes[order[k]];
    const SahNode& L = nodes[n.left];
    const SahNode& R = nodes[n.right];
    const int rl = L.n > 0 ? (L.direct ? L.ref : leaf_ref(L.first, L.n)) : idx[n.left];
    const int rr = R.n > 0 ? (R.direct ? R.ref : leaf_ref(R.first, R.n)) : idx[n.right];
    float4* q = &out[4 * k];
    q[0] = float4{L.lo[0], L.lo[1], L.lo[2], L.hi[0]};
    q[1] = float4{L.hi[1], L.hi[2], R.lo[0], R.lo[1]};
    q[2] = float4{R.lo[2], R.hi[0], R.hi[1], R.hi[2]};
    float a, b;
    memcpy(&a, &rl, 4);
    memcpy(&b, &rr, 4);
    q[3] = float4{a, b, 0, 0};
  }
  *root_ref = 0;
  return PT_OK;
}

static int ref_first_of(int ref) { return (-(ref + 1)) >> 4; }
static int ref_count_of(int ref) { return (-(ref + 1)) & 15; }

// 4-wide form of a SahNode tree (the traversal kernels' WIDE walks): each 4-wide node holds up to four descendants of
// one binary node, the largest interior child opened first, never a `keep` node (a refined reference leaf keeps its
// exact box as a child box, refine_leaves). An opened node's box is only skipped, and it encloses the boxes that
// replace it (a union, or the widened fine boxes below a reference leaf, which only cull): a ray passing a kept box
// passed the skipped one too (slab rounding is monotone under containment), so the candidate triangles, and with
// them every closest t and any-hit verdict, are the binary tree's. Exact ties are re-walked on the reference tree.
// Layout (kWideStride x float4: 7 used = 112 B, padded to 128 B at 8): lo.x[4] hi.x[4] lo.y[4] hi.y[4] lo.z[4] hi.z[4] refs[4]; refs >= 0 node index,
// < 0 leaf, kNoneRef an empty slot. *need: the most stack entries a walk can hold (sum over a path of the
// children pushed beside the one taken); the kernels check pushes against their stack anyway.
// Which binary nodes a 4-wide node opens (PTSVGF_WIDE_COLLAPSE, read once): 0 = greedy (until round 6), the largest
// interior child opened until four slots are used; 1 = SAH-optimal, a dynamic program over the binary tree that picks
// the grouping with the least summed surface area of 4-wide nodes (each such node is one node step of a walk that
// reaches it; the leaves, hence their triangle tests, are the same either way); 2 = SAH-optimal for the any-hit
// (shadow) walks and greedy for the closest-hit walks, two trees in one buffer (SceneDev::root4c; the default);
// 3 = the reverse. Every form keeps `keep` nodes closed, so each is result-preserving by the argument above.
// Measured at 4K (profiles/r06/wide_collapse/, one box, two alternating repetitions): greedy 225.2 / 227.2 fps,
// surface view 78.0 / 78.3; SAH-optimal for both 231.1 / 229.6 and 76.6 / 76.1 (shadow visits -1.5 % / -7.1 %, but
// the surface view's closest-hit visits +7.8 %: the nearest-first, pruned walk is not what the area sum prices);
// mode 2 228.0 / 228.4 and 79.3 / 78.7. Same bits in every mode (planes digest, the wide-tree parity tests).
static int wide_collapse_mode() {
  static const int m = [] {
    const char* e = getenv("PTSVGF_WIDE_COLLAPSE");
    return e ? atoi(e) : 2;
  }();
  return m;
}

// The dynamic program of wide_collapse_mode() 1. For a binary node x: best[x] = A(x) + D(x, 4) (x as a 4-wide node);
// S(x, j) = the least cost of x's subtree given j slots of the enclosing 4-wide node (one slot: x itself, a leaf at
// cost 0 or a 4-wide node at best[x]; more: opened, its children sharing the slots); D(x, i) = min over j of
// S(left, j) + S(right, i - j), in one pass over the nodes in post order.
namespace {
struct WideCollapse {
  std::vector<float> best;
  std::vector<std::array<float, 5>> S, D;
  std::vector<std::array<signed char, 5>> dsplit;  // D(x, i): slots given to the left child
  std::vector<std::array<bool, 5>> sopen;          // S(x, j): opened (else one slot)
  explicit WideCollapse(const std::vector<SahNode>& nodes) {
    const size_t n = nodes.size();
    best.assign(n, 0.0f);
    S.assign(n, {});
    D.assign(n, {});
    dsplit.assign(n, {});
    sopen.assign(n, {});
    std::vector<int> order;  // children before parents (ids need not be: treelet_optimize reuses them)
    post_order(nodes, 0, order);
    for (int k : order) {
      const SahNode& x = nodes[k];
      const bool leaf = x.n > 0;
      if (!leaf) {
        for (int i = 2; i <= 4; ++i) {
          float b = INFINITY;
          int bj = 1;
          for (int j = 1; j < i; ++j) {
            const float c = S[x.left][j] + S[x.right][i - j];
            if (c < b) { b = c; bj = j; }
          }
          D[k][i] = b;
          dsplit[k][i] = (signed char)bj;
        }
        best[k] = sah_area(x.lo, x.hi) + D[k][4];
      }
      const float slot = leaf ? 0.0f : best[k];
      for (int j = 1; j <= 4; ++j) {
        const bool open = !leaf && !x.keep && j >= 2 && D[k][j] < slot;
        S[k][j] = open ? D[k][j] : slot;
        sopen[k][j] = open;
      }
    }
  }
  // the children of a 4-wide node rooted at binary node id
  int children(const std::vector<SahNode>& nodes, int id, int* ch) const {
    int nc = 0;
    std::function<void(int, int)> cover = [&](int x, int j) {
      if (!sopen[x][j]) { ch[nc++] = x; return; }
      expand(nodes, x, j, cover);
    };
    expand(nodes, id, 4, cover);
    return nc;
  }
  void expand(const std::vector<SahNode>& nodes, int x, int i, const std::function<void(int, int)>& cover) const {
    const int j = dsplit[x][i];
    cover(nodes[x].left, j);
    cover(nodes[x].right, i - j);
  }
};
}  // namespace

static int pack_wide(const std::vector<SahNode>& nodes, const std::function<int(int, int)>& leaf_ref,
                     std::vector<float4>& out, int* root_ref, int* need, bool dp, double* area_out = nullptr) {
  out.clear();
  *need = 0;
  auto ref_of = [&](const SahNode& L) { return L.direct ? L.ref : leaf_ref(L.first, L.n); };
  if (nodes[0].n > 0) {
    *root_ref = ref_of(nodes[0]);
    return PT_OK;
  }
  std::unique_ptr<WideCollapse> wc(dp ? new WideCollapse(nodes) : nullptr);
  static const int order_key = [] {
    const char* e = getenv("PTSVGF_WIDE_ORDER_KEY");
    return e ? atoi(e) : 0;
  }();
  std::vector<double> tris_below(nodes.size(), 0.0);  // triangles in each subtree (order_key 1 / 2)
  if (order_key) {
    std::vector<int> po;
    post_order(nodes, 0, po);
    for (int id : po) {
      const SahNode& x = nodes[id];
      tris_below[id] = x.n > 0 ? (double)ref_count_of(ref_of(x)) : tris_below[x.left] + tris_below[x.right];
    }
  }
  double area_sum = 0.0;  // summed surface area of the 4-wide nodes (PTSVGF_WIDE_STATS)
  std::function<int(int, int)> build = [&](int id, int acc) -> int {
    int ch[4] = {nodes[id].left, nodes[id].right, -1, -1};
    int nc = 2;
    area_sum += sah_area(nodes[id].lo, nodes[id].hi);
    if (dp) nc = wc->children(nodes, id, ch);
    while (!dp && nc < 4) {  // open the largest interior child that may be opened
      int best = -1;
      float ba = -1.0f;
      for (int c = 0; c < nc; ++c) {
        const SahNode& n = nodes[ch[c]];
        const float a = sah_area(n.lo, n.hi);
        if (n.n == 0 && !n.keep && a > ba) { ba = a; best = c; }
      }
      if (best < 0) break;
      const int b = ch[best];
      for (int c = nc; c > best + 1; --c) ch[c] = ch[c - 1];
      ch[best] = nodes[b].left;
      ch[best + 1] = nodes[b].right;
      ++nc;
    }
#if PT_WIDE_ORDER
    // slot order = build order: the first interior child is stored right after this node (depth first), so the
    // second cache line of this node's fetch holds most of it. Put the child a ray most likely enters there (largest
    // surface area). Slots only order ties between equally near children; the candidates, hence every result, are
    // the same.
    // PTSVGF_WIDE_ORDER_KEY (read once; A/B): 0 = area (default), 1 = triangles below, 2 = area x triangles below
    std::stable_sort(ch, ch + nc, [&](int x, int y) {
      const double ax = sah_area(nodes[x].lo, nodes[x].hi), ay = sah_area(nodes[y].lo, nodes[y].hi);
      if (order_key == 1) return tris_below[x] > tris_below[y];
      if (order_key == 2) return ax * tris_below[x] > ay * tris_below[y];
      return ax > ay;
    });
#endif
    const int k = (int)(out.size() / ptk::kWideStride);
    out.resize(out.size() + ptk::kWideStride, float4{0, 0, 0, 0});
    {  // empty slots: lo = +inf, hi = -inf, a box no ray enters (wide_step's signed test needs no slot check)
      float* q = (float*)&out[ptk::kWideStride * (size_t)k];
      for (int a = 0; a < 3; ++a)
        for (int c = nc; c < 4; ++c) {
          q[8 * a + c] = INFINITY;
          q[8 * a + 4 + c] = -INFINITY;
        }
    }
    const int here = acc + nc - 1;
    *need = std::max(*need, here + 1);
    int refs[4] = {kNoneRef, kNoneRef, kNoneRef, kNoneRef};
    for (int c = 0; c < nc; ++c) {
      const SahNode& n = nodes[ch[c]];
      float* q = (float*)&out[ptk::kWideStride * (size_t)k];
      for (int a = 0; a < 3; ++a) { q[8 * a + c] = n.lo[a]; q[8 * a + 4 + c] = n.hi[a]; }
      refs[c] = n.n > 0 ? ref_of(n) : build(ch[c], here);  // may reallocate `out`
    }
    memcpy(&out[ptk::kWideStride * (size_t)k + 6], refs, 16);
    return k;
  };
  build(0, 0);
  *root_ref = 0;
  if (area_out) *area_out = area_sum / std::max(1e-30, (double)sah_area(nodes[0].lo, nodes[0].hi));
  if (getenv("PTSVGF_WIDE_STATS"))
    fprintf(stderr, "ptsvgf: 4-wide tree (%s collapse): %zu nodes, summed node area / root area %.4f, stack need %d\n",
            dp ? "SAH-optimal" : "greedy", out.size() / ptk::kWideStride,
            area_sum / std::max(1e-30, (double)sah_area(nodes[0].lo, nodes[0].hi)), *need);
  return PT_OK;
}

// Fine leaves under the reference leaves (PTSVGF_FINE_LEAVES = F, the largest fine leaf; 0 = off). A reference leaf
// holds up to 8 triangles (BVH.h:77, main.cpp:96) in one box; every ray that passes that box tests all of them. Here
// each reference leaf of more than F triangles becomes an interior node over contiguous sub-ranges of its triangles
// (index order kept, so a fine leaf is a valid leaf ref), cut by SAH on their boxes, down to <= F triangles.
// Result-preserving: the reference leaf's own box is still tested exactly (it is the box the parent stores for this
// child), and a fine box is the min/max box of its triangles widened by `pad` (2^-12 of the largest coordinate
// magnitude, ~500x the float rounding of hitTriangle's hit point and of the slab arithmetic), so a ray that
// hitTriangle (:215-272) accepts for one of those triangles passes it: the fine boxes only cull triangles that cannot
// be hit, and the candidate set (and with it every closest t and any-hit verdict) is the reference leaf's. Exact ties
// are re-walked on the reference tree as before. Leaves with a non-finite vertex coordinate stay whole.
// The rounding of the hit point grows with the ray origin's magnitude and the hit distance, not with the vertices:
// bounce and shadow rays start on the scene (|origin| <= mag), primary rays at the eye. The pad covers eyes within
// kFineEyeReach x max(mag, 1) per coordinate (the rounding then stays >= 32x below the pad); pt_params walks the
// reference tree (no fine boxes) for an eye beyond that.
static int fine_leaf_max() {
  static const int f = [] {
    const char* e = getenv("PTSVGF_FINE_LEAVES");
    return e ? std::max(0, atoi(e)) : 4;
  }();
  return f;
}

static int fine_subtree(const float* tri_enc, const float* tlo, const float* thi, int a, int b, int F, float pad,
                        std::vector<SahNode>& nodes, int forced_id = -1) {
  const int id = forced_id >= 0 ? forced_id : (int)nodes.size();
  if (forced_id < 0) nodes.emplace_back();
  SahNode nd = forced_id >= 0 ? nodes[forced_id] : SahNode{};
  auto box = [&](int u, int v, float* lo, float* hi) {
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (int i = u; i < v; ++i)
      for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], tlo[3 * i + k]); hi[k] = std::max(hi[k], thi[3 * i + k]); }
    for (int k = 0; k < 3; ++k) { lo[k] -= pad; hi[k] += pad; }
  };
  if (forced_id < 0) box(a, b, nd.lo, nd.hi);  // the subtree root keeps the reference leaf's exact box
  if (b - a <= F) {
    nd.n = b - a;
    nd.direct = true;
    nd.ref = -(a * 16 + (b - a)) - 1;
    nodes[id] = nd;
    return id;
  }
  float best = INFINITY;
  int m = a + (b - a) / 2;
  for (int c = a + 1; c < b; ++c) {
    float l0[3], l1[3], r0[3], r1[3];
    box(a, c, l0, l1);
    box(c, b, r0, r1);
    const float cost = sah_area(l0, l1) * (c - a) + sah_area(r0, r1) * (b - c);
    if (cost < best) { best = cost; m = c; }
  }
  nd.n = 0;
  nd.direct = false;
  nd.left = fine_subtree(tri_enc, tlo, thi, a, m, F, pad, nodes);
  nd.right = fine_subtree(tri_enc, tlo, thi, m, b, F, pad, nodes);
  nodes[id] = nd;
  return id;
}

// Returns the coordinate magnitude the pad was sized for (0: no fine leaves).
static float refine_leaves(std::vector<SahNode>& nodes, const std::vector<SahPrim>& pr, const float* tri_enc,
                           int ntris, int F) {
  if (F <= 0 || !tri_enc) return 0.0f;
  std::vector<float> tlo((size_t)ntris * 3), thi((size_t)ntris * 3);
  std::vector<char> finite((size_t)ntris);
  float mag = 0.0f;
  for (int i = 0; i < ntris; ++i) {
    const float* f = tri_enc + (size_t)i * 45;  // Triangle_encoded: p1 p2 p3 first (Triangle.h:12-24)
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const float v0 = f[k], v1 = f[3 + k], v2 = f[6 + k];
      ok = ok && std::isfinite(v0) && std::isfinite(v1) && std::isfinite(v2);
      tlo[3 * i + k] = std::min(v0, std::min(v1, v2));
      thi[3 * i + k] = std::max(v0, std::max(v1, v2));
    }
    finite[i] = ok;
    if (ok)
      for (int k = 0; k < 9; ++k) mag = std::max(mag, std::fabs(f[k]));
  }
  const float pad = std::max(mag, 1.0f) * (1.0f / 4096.0f);
  const size_t n0 = nodes.size();
  bool any = false;
  for (size_t id = 0; id < n0; ++id) {
    if (nodes[id].n <= 0) continue;
    const int ref = pr[nodes[id].first].ref;
    const int first = ref_first_of(ref), cnt = ref_count_of(ref);
    if (cnt <= F) continue;
    bool ok = true;
    for (int i = first; i < first + cnt; ++i) ok = ok && finite[i];
    if (!ok) continue;
    SahNode root = nodes[id];  // exact reference-leaf box, stored by the parent for this child
    root.n = 0;
    root.keep = true;
    nodes[id] = root;
    fine_subtree(tri_enc, tlo.data(), thi.data(), first, first + cnt, F, pad, nodes, (int)id);
    any = true;
  }
  return any ? std::max(mag, 1.0f) : 0.0f;
}

// Any-hit tree over the leaves of the reference tree (see above), with fine leaves under them (refine_leaves).
int build_anyhit_tree(const float* node_enc, int nnodes, int ntris, const float* tri_enc, std::vector<float4>& out,
                      int* root_ref, int* need, std::string* msg, std::vector<float4>* wide, int* root_wide,
                      int* need_wide, float* fine_mag, int* root_closest, int collapse, int treelet, double* stats) {
  // collapse / treelet: PTSVGF_WIDE_COLLAPSE / PTSVGF_TREELET when < 0; stats (pt_tree_check): SAH cost / root area
  // before and after the treelet pass, summed 4-wide node area / root area of the any-hit and closest-hit trees
  if (collapse < 0) collapse = wide_collapse_mode();
  if (treelet < 0) treelet = treelet_passes();
  double st_[4] = {0, 0, 0, 0};
  double* st = stats ? stats : st_;
  std::vector<SahPrim> pr;
  for (int i = 1; i < nnodes; ++i) {
    const float* f = node_enc + (size_t)i * 12;
    const int n = (int)f[3], first = (int)f[4];
    if (n <= 0) continue;
    if (n > 15 || first < 0 || first + n > ntris) return err(msg, PT_ERR_FORMAT, "BVH leaf out of range");
    SahPrim q;
    for (int a = 0; a < 3; ++a) { q.lo[a] = f[6 + a]; q.hi[a] = f[9 + a]; }
    q.weight = n;
    q.ref = -(first * 16 + n) - 1;
    pr.push_back(q);
  }
  if (pr.empty()) return err(msg, PT_ERR_FORMAT, "BVH without leaves");
  std::vector<SahNode> nodes;
  nodes.reserve(2 * pr.size());
  const int F = fine_leaf_max();
  sah_build(pr, 0, (int)pr.size(), 1, nodes, 1, F > 0 ? ceil_log2(16) : 0);  // a fine subtree is <= 4 levels deep
  treelet_optimize(nodes, pr, treelet, F > 0 ? ceil_log2(16) : 0, &st[0], &st[1]);
  const float mag = refine_leaves(nodes, pr, tri_enc, ntris, F);
  if (fine_mag) *fine_mag = mag;
  auto leaf_ref = [&](int first, int) { return pr[first].ref; };
  const int rc = pack_sah(nodes, leaf_ref, out, root_ref, need, msg);
  if (rc != PT_OK || !wide) return rc;
  const int mode = collapse;
  const int rw = pack_wide(nodes, leaf_ref, *wide, root_wide, need_wide, mode == 1 || mode == 2, &st[2]);
  st[3] = st[2];
  if (root_closest) *root_closest = *root_wide;
  if (rw != PT_OK || !root_closest || (mode != 2 && mode != 3) || *root_wide < 0) return rw;
  // the closest-hit walks' tree, appended: its node indices shifted past the any-hit tree's
  std::vector<float4> second;
  int root2 = 0, need2 = 0;
  const int r2 = pack_wide(nodes, leaf_ref, second, &root2, &need2, mode == 3, &st[3]);
  if (r2 != PT_OK) return r2;
  const int base = (int)(wide->size() / ptk::kWideStride);
  for (size_t k = 0; k + ptk::kWideStride <= second.size(); k += ptk::kWideStride) {
    int refs[4];
    memcpy(refs, &second[k + 6], 16);
    for (int c = 0; c < 4; ++c)
      if (refs[c] >= 0) refs[c] += base;
    memcpy(&second[k + 6], refs, 16);
  }
  *root_closest = root2 + base;
  wide->insert(wide->end(), second.begin(), second.end());
  *need_wide = std::max(*need_wide, need2);
  return PT_OK;
}

// pt_tree_check (include/ptsvgf.h): the trees build_anyhit_tree makes for a reference tree, checked on the host
// against the properties the walks' result preservation rests on. Host only: no device, no pt_init.
namespace {
struct TreeCheck {
  const float* node_enc;
  int nnodes;
  const float* tri_enc;
  int ntris;
  std::vector<int> cover;  // per triangle: leaves of the checked tree holding it
  std::vector<char> inref; // per triangle: held by a reference leaf
  std::map<std::array<uint32_t, 6>, int> refbox;  // reference leaf boxes (bits) -> triangle count
  bool contain_ok = true, leaf_ok = true;
  int depth = 0;
  static std::array<uint32_t, 6> key(const float* lo, const float* hi) {
    std::array<uint32_t, 6> k;
    for (int a = 0; a < 3; ++a) { memcpy(&k[a], &lo[a], 4); memcpy(&k[3 + a], &hi[a], 4); }
    return k;
  }
  void init() {
    cover.assign((size_t)ntris, 0);
    inref.assign((size_t)ntris, 0);
    for (int i = 1; i < nnodes; ++i) {
      const float* f = node_enc + (size_t)i * 12;
      const int n = (int)f[3], first = (int)f[4];
      if (n <= 0) continue;
      for (int t = first; t < first + n && t < ntris; ++t) inref[(size_t)t] = 1;
      refbox[key(f + 6, f + 9)] = n;
    }
  }
  static bool inside(const float* lo, const float* hi, const float* plo, const float* phi) {
    for (int a = 0; a < 3; ++a)
      if (lo[a] < plo[a] || hi[a] > phi[a]) return false;
    return true;
  }
  // a leaf ref below a box: its triangles marked; each triangle's vertex box inside the box
  void leaf(int ref, const float* lo, const float* hi) {
    const int first = ref_first_of(ref), cnt = ref_count_of(ref);
    for (int t = first; t < first + cnt; ++t) {
      if (t < 0 || t >= ntris) { leaf_ok = false; continue; }
      ++cover[(size_t)t];
      const float* v = tri_enc + (size_t)t * 45;
      for (int a = 0; a < 3; ++a) {
        const float tl = std::min(v[a], std::min(v[3 + a], v[6 + a])), th = std::max(v[a], std::max(v[3 + a], v[6 + a]));
        if (std::isfinite(tl) && std::isfinite(th) && (tl < lo[a] || th > hi[a])) contain_ok = false;
      }
    }
  }
  // a child slot box (lo, hi) holding a subtree; `fine`: the box is a reference leaf's (its fine boxes, widened, need
  // not lie inside it: each fine leaf's box must hold its triangles instead)
  bool is_ref_leaf_box(const float* lo, const float* hi) const { return refbox.count(key(lo, hi)) != 0; }
  bool partition_ok() const {
    for (int t = 0; t < ntris; ++t)
      if (cover[(size_t)t] != (inref[(size_t)t] ? 1 : 0)) return false;
    return true;
  }
  void walk_binary(const std::vector<float4>& bvh, int ref, const float* lo, const float* hi, bool fine, int d) {
    depth = std::max(depth, d);
    if (ref < 0) { leaf(ref, lo, hi); return; }
    const float* q = (const float*)&bvh[4 * (size_t)ref];
    const float L0[3] = {q[0], q[1], q[2]}, L1[3] = {q[3], q[4], q[5]};
    const float R0[3] = {q[6], q[7], q[8]}, R1[3] = {q[9], q[10], q[11]};
    int rl, rr;
    memcpy(&rl, &q[12], 4);
    memcpy(&rr, &q[13], 4);
    for (int s = 0; s < 2; ++s) {
      const float* cl = s ? R0 : L0;
      const float* ch = s ? R1 : L1;
      if (!fine && lo && !inside(cl, ch, lo, hi)) contain_ok = false;
      walk_binary(bvh, s ? rr : rl, cl, ch, fine || is_ref_leaf_box(cl, ch), d + 1);
    }
  }
  void walk_wide(const std::vector<float4>& w, int ref, const float* lo, const float* hi, bool fine, int d) {
    depth = std::max(depth, d);
    if (ref < 0) { leaf(ref, lo, hi); return; }
    const float* q = (const float*)&w[(size_t)ptk::kWideStride * ref];
    int refs[4];
    memcpy(refs, q + 24, 16);
    for (int c = 0; c < 4; ++c) {
      if (refs[c] == kNoneRef) continue;
      const float cl[3] = {q[c], q[8 + c], q[16 + c]}, ch[3] = {q[4 + c], q[12 + c], q[20 + c]};
      if (!fine && lo && !inside(cl, ch, lo, hi)) contain_ok = false;
      walk_wide(w, refs[c], cl, ch, fine || is_ref_leaf_box(cl, ch), d + 1);
    }
  }
};
}  // namespace

int tree_check(const float* node_enc, int nnodes, const float* tri_enc, int ntris, int collapse, int treelet,
               double* out, int nout, std::string* msg) {
  if (!node_enc || !tri_enc || !out || nnodes < 2 || ntris < 1) return err(msg, PT_ERR_ARG, "trees and output needed");
  if (nout < PT_TREE_CHECK_COUNT) return err(msg, PT_ERR_ARG, "output holds fewer than PT_TREE_CHECK_COUNT values");
  if (collapse < 0 || collapse > 3 || treelet < 0) return err(msg, PT_ERR_ARG, "collapse in 0..3, treelet >= 0");
  std::vector<float4> bin, wide;
  int root_any = 0, need_any = 0, root4 = 0, need4 = 0, root4c = 0;
  float mag = 0.0f;
  double st[4] = {0, 0, 0, 0};
  const int rc = build_anyhit_tree(node_enc, nnodes, ntris, tri_enc, bin, &root_any, &need_any, msg, &wide, &root4,
                                   &need4, &mag, &root4c, collapse, treelet, st);
  if (rc != PT_OK) return rc;
  double ok[3];
  int depth[3];
  bool contain = true;
  for (int k = 0; k < 3; ++k) {
    TreeCheck tc{node_enc, nnodes, tri_enc, ntris};
    tc.init();
    if (k == 0) tc.walk_binary(bin, root_any, nullptr, nullptr, false, 1);
    else tc.walk_wide(wide, k == 1 ? root4 : root4c, nullptr, nullptr, false, 1);
    ok[k] = tc.partition_ok() && tc.leaf_ok ? 1.0 : 0.0;
    depth[k] = tc.depth;
    contain = contain && tc.contain_ok;
  }
  const double vals[PT_TREE_CHECK_COUNT] = {ok[0], ok[1], ok[2], contain ? 1.0 : 0.0, st[0], st[1], st[2], st[3],
                                            (double)(wide.size() / ptk::kWideStride), (double)depth[0],
                                            (double)need4, root4c != root4 ? 1.0 : 0.0};
  for (int i = 0; i < PT_TREE_CHECK_COUNT; ++i) out[i] = vals[i];
  return PT_OK;
}

// a child box of a 4-wide tree (pack_wide) has a NaN coordinate (SceneGPU::nan4)
bool wide_has_nan(const std::vector<float4>& bvh4) {
  bool nan = false;
  for (size_t k = 0; k + ptk::kWideStride <= bvh4.size(); k += ptk::kWideStride) {
    const float* q = (const float*)&bvh4[k];
    int refs[4];
    memcpy(refs, q + 24, 16);
    for (int c = 0; c < 4; ++c)
      for (int i = 0; i < 6; ++i) nan = nan || (refs[c] != kNoneRef && std::isnan(q[4 * i + c]));
  }
  return nan;
}

// The reference tree's leaves with their own boxes (the primary-ray tile rasteriser's items). The caller has checked
// the leaf ranges (pack_bvh).
void collect_leaves(const float* ne, size_t nnodes, std::vector<float4>& lv) {
  lv.clear();
  for (size_t i = 1; i < nnodes; ++i) {
    const float* f = ne + i * 12;
    const int n = (int)f[3], first = (int)f[4];
    if (n <= 0) continue;
    const int ref = -(first * 16 + n) - 1;
    float rf;
    memcpy(&rf, &ref, 4);
    lv.push_back(float4{f[6], f[7], f[8], rf});
    lv.push_back(float4{f[9], f[10], f[11], 0.0f});
  }
}

// SAH tree over the raster triangles (sah_build: the walk's answer does not depend on the tree);
// order = the triangles in leaf order, by original index (the depth-test tie rule keeps it as objIndex)
int build_raster_tree(const float* verts, int ntris, std::vector<int>& order, std::vector<float4>& bvh, int* root_ref,
                      int* need, std::string* msg) {
  std::vector<SahPrim> pr((size_t)ntris);
  for (int i = 0; i < ntris; ++i) {
    const float* q = verts + (size_t)i * 18;
    for (int a = 0; a < 3; ++a) {
      pr[i].lo[a] = std::min(q[a], std::min(q[6 + a], q[12 + a]));
      pr[i].hi[a] = std::max(q[a], std::max(q[6 + a], q[12 + a]));
    }
    pr[i].weight = 1;
    pr[i].ref = i;
  }
  std::vector<SahNode> tree;
  tree.reserve(2 * (size_t)ntris);
  sah_build(pr, 0, ntris, 8, tree);  // leaves of <= 8 (measured: 2 and 4 slower, tools/exp_tree_ab.sh)
  order.resize((size_t)ntris);
  for (int k = 0; k < ntris; ++k) order[k] = pr[k].ref;
  return pack_sah(tree, [](int first, int n) { return -(first * 16 + n) - 1; }, bvh, root_ref, need, msg);
}

int pack_wide_encoded(const float* ne, int nnodes, std::vector<float4>& wide, int* root_ref, int* need) {
  std::vector<SahNode> sn((size_t)nnodes - 1);  // encoded node i is SahNode i - 1: the root is node 0
  for (int i = 1; i < nnodes; ++i) {
    const float* f = ne + (size_t)i * 12;
    SahNode& x = sn[(size_t)i - 1];
    for (int a = 0; a < 3; ++a) { x.lo[a] = f[6 + a]; x.hi[a] = f[9 + a]; }
    x.n = std::max((int)f[3], 0);
    x.first = (int)f[4];
    if (x.n == 0) { x.left = (int)f[0] - 1; x.right = (int)f[1] - 1; }
  }
  return pack_wide(sn, [](int first, int cnt) { return -(first * 16 + cnt) - 1; }, wide, root_ref, need, false);
}

}  // namespace ptk

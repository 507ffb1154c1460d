// Host-side check of the tree builder (path-tracing-svgf_amd/csrc/host_trees.cpp) under the host sanitizers: a
// stand-alone program over scenes of the host scene library, no device is touched and no HIP compiler is needed.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off
//       -Ipath-tracing-svgf_amd/csrc tools/host_trees_check.cpp path-tracing-svgf_amd/csrc/host_trees.cpp
//       path-tracing-svgf_amd/csrc/scene_prep.cpp -o /tmp/host_trees_check && /tmp/host_trees_check
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/ptsvgf.h"
#include "../include/ptsvgf_scene.h"
#include "host_trees.h"

using namespace ptk;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++fails;                                                    \
    }                                                             \
  } while (0)

struct Encoded {
  std::vector<float> tri, node, raster;  // 45 floats per triangle, 12 per node (dummy node 0 included), 18 per triangle
  int ntris() const { return (int)(tri.size() / 45); }
  int nnodes() const { return (int)(node.size() / 12); }
};

template <class Gen>
static Encoded scene_of(Gen gen) {
  int nv = 0, nt = 0;
  CHECK(gen(&nv, &nt, nullptr, nullptr) == 0);
  std::vector<float> pos((size_t)nv * 3);
  std::vector<int> idx((size_t)nt * 3);
  CHECK(gen(&nv, &nt, pos.data(), idx.data()) == 0);
  float mat[PTS_MATERIAL_FLOATS] = {0, 0, 0, 0.8f, 0.8f, 0.8f, 0, 0, 0.5f, 0, 0.5f, 0, 0, 0.5f, 0, 1, 1, 0};
  const float one[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  pts_scene* s = pts_scene_create();
  CHECK(s != nullptr);
  CHECK(pts_scene_add_mesh(s, pos.data(), nullptr, nv, idx.data(), nt, mat, one, 1, 0) == 0);
  CHECK(pts_scene_build_bvh(s, 8) == 0);
  int64_t c[6] = {};
  CHECK(pts_scene_counts(s, c) == 0);
  Encoded e;
  e.tri.assign((size_t)c[0] * 45, 0.0f);
  e.node.assign((size_t)c[1] * 12, 0.0f);
  e.raster.assign((size_t)c[5], 0.0f);
  CHECK(pts_scene_encode(s, e.tri.data(), e.node.data(), e.raster.data()) == 0);
  pts_scene_destroy(s);
  return e;
}

// n copies of one triangle, eight per reference leaf under a balanced reference tree: every box is the same box and
// every centroid the same point, so each cut of a SAH split costs the same, the first is taken, and the splits peel
// one primitive per level until the depth cap halves the rest
static Encoded coincident(int n) {
  Encoded e;
  e.tri.assign((size_t)n * 45, 0.0f);
  e.raster.assign((size_t)n * 18, 0.0f);
  for (int i = 0; i < n; ++i) {
    const float p[9] = {-1, -1, 0, 1, -1, 0, 0, 1, 0};
    std::memcpy(&e.tri[(size_t)i * 45], p, sizeof(p));
    for (int v = 0; v < 3; ++v) {
      std::memcpy(&e.raster[(size_t)i * 18 + 6 * v], p + 3 * v, 12);
      e.raster[(size_t)i * 18 + 6 * v + 5] = 1.0f;
    }
  }
  e.node.assign(12, 0.0f);  // the dummy node 0
  struct Build {
    Encoded& e;
    int make(int a, int b) {  // triangles [a, b)
      const int id = (int)(e.node.size() / 12);
      e.node.resize(e.node.size() + 12, 0.0f);
      const float box[6] = {-1, -1, 0, 1, 1, 0};
      const bool leaf = b - a <= 8;
      int l = 0, r = 0;
      if (!leaf) {
        l = make(a, (a + b) / 2);
        r = make((a + b) / 2, b);
      }
      float* f = &e.node[(size_t)id * 12];
      f[0] = (float)l;
      f[1] = (float)r;
      f[3] = leaf ? (float)(b - a) : 0.0f;
      f[4] = leaf ? (float)a : 0.0f;
      std::memcpy(f + 6, box, sizeof(box));
      return id;
    }
  } build{e};
  CHECK(build.make(0, n) == 1);
  return e;
}

static void check_scene(const char* name, const Encoded& e) {
  const int ntris = e.ntris(), nnodes = e.nnodes();
  CHECK(ntris > 0 && nnodes > 1);
  for (int collapse = 0; collapse <= 3; ++collapse)
    for (int treelet = 0; treelet <= 1; ++treelet) {
      double out[PT_TREE_CHECK_COUNT] = {};
      std::string msg;
      const int rc = tree_check(e.node.data(), nnodes, e.tri.data(), ntris, collapse, treelet, out,
                                PT_TREE_CHECK_COUNT, &msg);
      if (rc != PT_OK) std::printf("%s: tree_check(%d, %d): %s\n", name, collapse, treelet, msg.c_str());
      CHECK(rc == PT_OK);
      CHECK(out[0] == 1.0 && out[1] == 1.0 && out[2] == 1.0);  // the three partitions
      CHECK(out[3] == 1.0);                                    // containment
      CHECK(out[9] < (double)kStack);                          // depth of the binary tree
      if (collapse == 2 && treelet == 1) std::printf("%s: any-hit tree depth %d\n", name, (int)out[9]);
      CHECK(out[5] <= out[4] * (1 + 1e-9));                    // the treelet pass does not raise the SAH cost
    }
  // the reference tree itself, packed
  {
    std::vector<Float4> bvh, leaves;
    int root = 0, need = 0;
    std::string msg;
    CHECK(pack_bvh(e.node.data(), nnodes, bvh, &root, ntris, &need, &msg) == PT_OK);
    CHECK(need < kRefStack);
    collect_leaves(e.node.data(), (size_t)nnodes, leaves);
    CHECK(leaves.size() % 2 == 0 && !leaves.empty());
    std::vector<Float4> wide;
    int root4 = 0, need4 = 0;
    CHECK(pack_wide_encoded(e.node.data(), nnodes, wide, &root4, &need4) == PT_OK);
    CHECK(wide.size() % kWideStride == 0 && !wide_has_nan(wide));
  }
  // the G-buffer tree over the raster triangles
  const int rtris = (int)(e.raster.size() / 18);
  std::vector<int> order;
  std::vector<Float4> bvh;
  int root = 0, need = 0;
  std::string msg;
  CHECK(build_raster_tree(e.raster.data(), rtris, order, bvh, &root, &need, &msg) == PT_OK);
  CHECK(need < kStack);
  CHECK((int)order.size() == rtris);
  std::vector<int> seen((size_t)rtris, 0), held((size_t)rtris, 0);
  for (int o : order) {
    CHECK(o >= 0 && o < rtris);
    if (o >= 0 && o < rtris) ++seen[(size_t)o];
  }
  CHECK(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }));
  const int nrec = (int)(bvh.size() / 4);
  auto leaf = [&](int ref) {
    const int first = (-(ref + 1)) >> 4, cnt = (-(ref + 1)) & 15;
    CHECK(first >= 0 && cnt >= 1 && first + cnt <= rtris);
    for (int t = std::max(first, 0); t < std::min(first + cnt, rtris); ++t) ++held[(size_t)t];
  };
  if (nrec == 0) {
    CHECK(root < 0);
    leaf(root);
  } else {
    CHECK(root == 0);
  }
  for (int k = 0; k < nrec; ++k) {
    int refs[2];
    std::memcpy(refs, &bvh[4 * (size_t)k + 3], 8);
    for (int r : refs) {
      if (r < 0) leaf(r);
      else CHECK(r > k && r < nrec);  // depth-first order: a child record follows its parent
    }
  }
  CHECK(std::all_of(held.begin(), held.end(), [](int c) { return c == 1; }));
  std::printf("%s: %d triangles, %d nodes, raster tree %d records (stack need %d)\n", name, ntris, nnodes, nrec, need);
}

int main() {
  check_scene("cornell", scene_of([](int* nv, int* nt, float* p, int* i) { return pts_gen_cornell(nv, nt, p, i); }));
  check_scene("teapot", scene_of([](int* nv, int* nt, float* p, int* i) { return pts_gen_teapot(8, nv, nt, p, i); }));
  check_scene("plant", scene_of([](int* nv, int* nt, float* p, int* i) { return pts_gen_plant(0u, 40, nv, nt, p, i); }));
  check_scene("coincident", coincident(3000));
  std::printf(fails ? "host_trees_check: %d failure(s)\n" : "host_trees_check: ok\n", fails);
  return fails ? 1 : 0;
}

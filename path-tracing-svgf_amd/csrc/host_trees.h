// host_trees.h — the host tree builder (host_trees.cpp): the packed trees the C ABI layer (capi_draw_pt.hip, capi_geometry.hip) uploads, built
// from the encoded reference tree or from raster triangles. Plain C++ over std::vector: no HIP header, no library
// state. Every function that can fail returns a PT_* code (include/ptsvgf.h) and, when `msg` is not null, its message.
#pragma once
#include <stddef.h>

#include <string>
#include <vector>

#include "pt_layout.h"

namespace ptk {

constexpr int kRefStack = 256;  // path_tracing.frag:378
// refine_leaves' fine boxes hold for ray origins within this factor of the scene's largest coordinate (host_trees.cpp)
constexpr float kFineEyeReach = 64.0f;

// The reference tree in the kernels' records (4 per interior node, DFS order).
// *need: deepest interior level (root = 1) = the most stack entries a walk holds
int pack_bvh(const float* node_enc, int nnodes, std::vector<Float4>& out, int* root_ref, int ntris, int* need,
             std::string* msg);

// Any-hit tree over the leaves of the reference tree, with fine leaves under them, and its 4-wide form(s).
// collapse / treelet: PTSVGF_WIDE_COLLAPSE / PTSVGF_TREELET when < 0; stats: see tree_check
int build_anyhit_tree(const float* node_enc, int nnodes, int ntris, const float* tri_enc, std::vector<Float4>& out,
                      int* root_ref, int* need, std::string* msg, std::vector<Float4>* wide = nullptr,
                      int* root_wide = nullptr, int* need_wide = nullptr, float* fine_mag = nullptr,
                      int* root_closest = nullptr, int collapse = -1, int treelet = -1, double* stats = nullptr);

// The G-buffer tree over raster triangles (verts: 18 floats each, pos3 + nrm3 per vertex; ntris >= 1).
// order[k]: the original index of the triangle at leaf-order position k, which a leaf ref's range counts in.
int build_raster_tree(const float* verts, int ntris, std::vector<int>& order, std::vector<Float4>& bvh, int* root_ref,
                      int* need, std::string* msg);

// The greedy 4-wide form of an encoded binary tree itself (what the device stage of pt_bvh_build has to equal).
int pack_wide_encoded(const float* node_enc, int nnodes, std::vector<Float4>& wide, int* root_ref, int* need);

// pt_tree_check (include/ptsvgf.h) without the library's lock.
int tree_check(const float* node_enc, int nnodes, const float* tri_enc, int ntris, int collapse, int treelet,
               double* out, int nout, std::string* msg);

// The reference tree's leaves with their own boxes: (box lo, leaf ref bits), (box hi, 0) per leaf.
void collect_leaves(const float* ne, size_t nnodes, std::vector<Float4>& lv);
// a child box of a 4-wide tree has a NaN coordinate
bool wide_has_nan(const std::vector<Float4>& bvh4);

}  // namespace ptk

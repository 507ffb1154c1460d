// pt_layout.h — the layout constants of the packed trees, shared by the host tree builder (host_trees.cpp, plain
// C++) and the device side (pt_device.h). No HIP header is needed to read it.
#pragma once

namespace ptk {

// One 16-byte record of a packed tree as the host builder writes it: a device float4's bytes. The builder's interface
// is spelled with this type so that it names one type whether its caller is compiled as HIP or as plain C++ (HIP's
// float4 is a typedef of a class template; a plain struct of that name is another type to the linker).
struct Float4 {
  float x, y, z, w;
};

#ifndef PT_KSTACK
#define PT_KSTACK 32
#endif
// float4s per node of the 4-wide tree (pack_wide): 7 hold the four child boxes and refs. PT_WIDE_STRIDE = 8 pads a
// node to one 128-B cache line (at 7, 112-B nodes straddle two lines for most indices): measured SLOWER, 211.5 ->
// 202.6 fps at 4K and 69.2 -> 62.9 on the surface view (three alternating repetitions, profiles/r04/wide_stride_ab.log).
#ifndef PT_WIDE_STRIDE
#define PT_WIDE_STRIDE 7
#endif
constexpr int kWideStride = PT_WIDE_STRIDE;
// PT_WIDE_ORDER = 1 (default): pack_wide stores a node's largest child first, i.e. right after the node, where the
// node's own fetch already brings most of it into L1 (host_trees.cpp). Same box, three alternating repetitions
// (profiles/r04/wide_order_ab.log): 4K 210.6 / 212.2 / 210.4 -> 213.0 / 214.2 / 213.0 fps, surface view
// 68.6 / 68.9 / 68.5 -> 69.7 / 69.7 / 69.7.
#ifndef PT_WIDE_ORDER
#define PT_WIDE_ORDER 1
#endif
constexpr int kStack = PT_KSTACK;  // traversal stack depth (host checks BVH depth < kStack)
constexpr int kNoneRef = (int)0x80000000;

}  // namespace ptk

#if !defined(__HIPCC__)  // under hipcc float4 is HIP's own
using float4 = ptk::Float4;
#endif

// kernels_environment.hip — the environment's importance cache built on the device (DESIGN.md "Environment edits",
// tests/environment_ref.py): what pts_hdr_cache (scene_prep.cpp) computes on the host, bit for bit, from the hdr texels
// of a W x H map. Every float operation here is one the host does, in the host's order: the total is one dependent
// chain of W * H adds, the marginals and the conditional CDFs are one chain per column, the searches are libstdc++'s
// lower_bound. -ffp-contract=off (Makefile) keeps the double luminance uncontracted; float division is correctly
// rounded (hipcc's default). No index is read from memory: every one is computed from W, H and a bisection whose
// probes stay below its length.
#include <hip/hip_runtime.h>

#include "pt_device.h"

namespace ptk {

namespace {

// scratch layout (floats): pdf[W * H] (first the luminances), cdfy[W * H] (row-major: row i of every column's CDF),
// margin[W], cdfx[W], total[4] (one float, padded)
struct EnvScratch {
  float *pdf, *cdfy, *margin, *cdfx, *total;
};
__host__ __device__ inline EnvScratch env_scratch(float* base, int W, int H) {
  const size_t n = ((size_t)W * H + 3) & ~(size_t)3;  // (whole float4s: the total's chain loads them)
  const size_t w = ((size_t)W + 3) & ~(size_t)3;
  return EnvScratch{base, base + n, base + 2 * n, base + 2 * n + w, base + 2 * n + 2 * w};
}

// libstdc++'s std::lower_bound over a[0 .. n): the probes and their order decide the index on plateaus, NaNs and
// columns that are not monotone
__device__ __forceinline__ int env_lower_bound(const float* a, int n, float v) {
  int first = 0, len = n;
  while (len > 0) {
    const int half = len >> 1;
    if (a[first + half] < v) {
      first += half + 1;
      len -= half + 1;
    } else {
      len = half;
    }
  }
  return first;
}

__global__ void __launch_bounds__(256) env_expand_kernel(const float* __restrict__ rgb, float4* __restrict__ hdr, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* q = rgb + 3 * (size_t)i;
  hdr[i] = make_float4(q[0], q[1], q[2], 1.0f);
}

__global__ void __launch_bounds__(256) env_lum_kernel(const float4* __restrict__ hdr, float* __restrict__ lum, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 h = hdr[i];
  lum[i] = (float)((0.2 * (double)h.x + 0.7 * (double)h.y) + 0.1 * (double)h.z);
}

// The total: ((l0 + l1) + l2) + ... in row-major order. One wave; every lane runs the same chain. A step is 1024
// addends: the lanes load them as four float4s each, coalesced, one step ahead of the adds (a step's adds take longer
// than a load from HBM), and park them in LDS; the chain reads them back as float4s (all lanes one address: a
// broadcast). Two LDS buffers, so one barrier per step orders a buffer's writes before its reads and its reads before
// the writes two steps on. The chain is the kernel's time, one add per addend at best, so nothing else may sit in it:
// the LDS reads run a group of eight float4s ahead of the adds, in two register sets (A, B) whose order the
// scheduling barriers pin, and the step is unrolled in full so that neither set is carried round a loop (carried, the
// compiler copied it: 32 moves per 64 adds). Left to itself the compiler kept one read in flight, and the chain
// waited for LDS at every fourth add (15 ms for 2 M addends against 5).
constexpr int kTotalStep = 256;  // float4s per step
__global__ void __launch_bounds__(64) env_total_kernel(const float* __restrict__ lum, int n, float* __restrict__ total) {
  __shared__ float4 buf[2][kTotalStep];
  const int l = threadIdx.x;
  const int steps = n / (4 * kTotalStep);
  const float4* v = (const float4*)lum;
  float s = 0.0f;
  float4 nx0, nx1, nx2, nx3;
  if (steps > 0) {
    nx0 = v[l];
    nx1 = v[64 + l];
    nx2 = v[128 + l];
    nx3 = v[192 + l];
  }
  for (int c = 0; c < steps; ++c) {
    float4* w = buf[c & 1];
    w[l] = nx0;
    w[64 + l] = nx1;
    w[128 + l] = nx2;
    w[192 + l] = nx3;
    if (c + 1 < steps) {
      const float4* p = v + (size_t)(c + 1) * kTotalStep + l;
      nx0 = p[0];
      nx1 = p[64];
      nx2 = p[128];
      nx3 = p[192];
    }
    __syncthreads();
    const float4* b = buf[c & 1];
    float4 A[8], B[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) A[i] = b[i];
#pragma unroll
    for (int t = 0; t < kTotalStep; t += 16) {
#pragma unroll
      for (int i = 0; i < 8; ++i) B[i] = b[t + 8 + i];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        s += A[i].x;
        s += A[i].y;
        s += A[i].z;
        s += A[i].w;
      }
      __builtin_amdgcn_sched_barrier(0);
      const int tn = (t + 16) & (kTotalStep - 1);  // (after the last group the first again: read, not added)
#pragma unroll
      for (int i = 0; i < 8; ++i) A[i] = b[tn + i];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        s += B[i].x;
        s += B[i].y;
        s += B[i].z;
        s += B[i].w;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  for (int k = steps * 4 * kTotalStep; k < n; ++k) s += lum[k];
  if (l == 0) *total = s;
}

// One thread per column j, lanes across columns (coalesced rows): pdf = lum / total in place, the column's marginal
// from 0.0f in row order, then its conditional CDF c_0 = q_0, c_i = q_i + c_{i-1} with q_i = pdf / marginal.
__global__ void __launch_bounds__(64) env_columns_kernel(float* pdf, float* __restrict__ cdfy, float* __restrict__ margin,
                                                         const float* __restrict__ total, int W, int H) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= W) return;
  const float S = *total;
  float m = 0.0f;
#pragma unroll 8
  for (int i = 0; i < H; ++i) {
    const size_t k = (size_t)i * W + j;
    const float p = pdf[k] / S;
    pdf[k] = p;
    m += p;
  }
  margin[j] = m;
  float c = 0.0f;
#pragma unroll 8
  for (int i = 0; i < H; ++i) {
    const size_t k = (size_t)i * W + j;
    const float q = pdf[k] / m;
    c = i ? q + c : q;
    cdfy[k] = c;
  }
}

// The marginal CDF: the sequential prefix sum of the W marginals, by one thread over a copy in LDS (W <= kEnvMaxSide
// floats: 32 KiB)
__global__ void __launch_bounds__(256) env_cdfx_kernel(const float* __restrict__ margin, float* __restrict__ cdfx, int W) {
  extern __shared__ float row[];
  for (int j = threadIdx.x; j < W; j += 256) row[j] = margin[j];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int j = 1; j < W; ++j) row[j] += row[j - 1];
  __syncthreads();
  for (int j = threadIdx.x; j < W; j += 256) cdfx[j] = row[j];
}

// One block per row i: x depends on the row alone, so the block finds it once, stages column x of the conditional
// CDFs in LDS (H <= kEnvMaxSide floats: 32 KiB) and every thread bisects there for its columns j.
__global__ void __launch_bounds__(256) env_invert_kernel(const float4* __restrict__ hdr, const float* __restrict__ pdf,
                                                         const float* __restrict__ cdfy, const float* __restrict__ cdfx,
                                                         float4* __restrict__ cache, float4* __restrict__ merged, int W,
                                                         int H) {
  extern __shared__ float col[];
  __shared__ int xs;
  const int i = blockIdx.x;
  if (threadIdx.x == 0) {
    const float xi_1 = (float)i / (float)H;
    const int x = env_lower_bound(cdfx, W, xi_1);
    xs = x >= W ? W - 1 : x;
  }
  __syncthreads();
  const int x = xs;
  for (int t = threadIdx.x; t < H; t += 256) col[t] = cdfy[(size_t)t * W + x];
  __syncthreads();
  const float fx = (float)x / (float)W;
  for (int j = threadIdx.x; j < W; j += 256) {
    const float xi_2 = (float)j / (float)W;
    int y = env_lower_bound(col, H, xi_2);
    if (y >= H) y = H - 1;
    const size_t k = (size_t)i * W + j;
    const float p = pdf[k];
    const float4 h = hdr[k];
    cache[k] = make_float4(fx, (float)y / (float)H, p, 1.0f);
    merged[k] = make_float4(h.x, h.y, h.z, p);
  }
}

}  // namespace

int launch_environment_expand(const float* rgb, float4* hdr, int n, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(env_expand_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rgb, hdr, n);
  return (int)hipGetLastError();
}

size_t environment_scratch_floats(int W, int H) {
  const EnvScratch e = env_scratch(nullptr, W, H);
  return (size_t)(e.total - e.pdf) + 4;
}

int launch_environment_cache(const float4* hdr, float4* cache, float4* merged, float* scratch, int W, int H,
                             hipStream_t s) {
  if (W < 1 || H < 1 || W > kEnvMaxSide || H > kEnvMaxSide) return (int)hipErrorInvalidValue;
  const int n = W * H;
  const EnvScratch e = env_scratch(scratch, W, H);
  hipLaunchKernelGGL(env_lum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, hdr, e.pdf, n);
  hipLaunchKernelGGL(env_total_kernel, dim3(1), dim3(64), 0, s, e.pdf, n, e.total);
  hipLaunchKernelGGL(env_columns_kernel, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, s, e.pdf, e.cdfy, e.margin,
                     e.total, W, H);
  hipLaunchKernelGGL(env_cdfx_kernel, dim3(1), dim3(256), (size_t)W * sizeof(float), s, e.margin, e.cdfx, W);
  hipLaunchKernelGGL(env_invert_kernel, dim3((unsigned)H), dim3(256), (size_t)H * sizeof(float), s, hdr, e.pdf, e.cdfy,
                     e.cdfx, cache, merged, W, H);
  return (int)hipGetLastError();
}

}  // namespace ptk

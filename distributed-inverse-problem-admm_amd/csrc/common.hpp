// common.hpp -- what the translation units beside the solver share (bounds.hip, relax.hip,
// metrics.hip, fbp.hip, masks.hip): the library's error path, and for the kernels that stream
// pixels (bounds, relax) or tiles (metrics) the launch shape and the two fixed-order sums.
// admm_tomo.hip does not include this file: its own HIPCHK adds the line number.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/admm_tomo.h"

namespace admm_internal {
int fail(int code, const std::string& msg);  // admm_tomo.hip: records msg for admm_last_error
}

#define HIP_TRY(expr)                                                                                        \
  do {                                                                                                       \
    hipError_t _e = (expr);                                                                                  \
    if (_e != hipSuccess)                                                                                    \
      return admm_internal::fail(ADMM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
  } while (0)

// (named namespace: the kernels keep their names in profiler output)
namespace admm {

// launch shape of the pixel-streaming kernels: one image or edge per blockIdx.y, thread t of block b
// takes pixels 1024 b + t, + 256, + 512, + 768
constexpr int kThreads = 256;
constexpr int kPer = 4;                         // pixels per thread
constexpr int kBlockPix = kThreads * kPer;      // 1024 pixels per block
constexpr int kMaxGridY = 65535;                // gridDim.y and gridDim.z
constexpr long long kMaxBlocks = 2147483647ll;  // gridDim.x

inline long long blocks_of(long long n) { return (n + kBlockPix - 1) / kBlockPix; }

inline int check_n(long long n) {
  if (n < 1 || blocks_of(n) > kMaxBlocks)
    return admm_internal::fail(ADMM_E_INVALID, "n must be in [1, 1024 * (2^31 - 1)]");
  return ADMM_OK;
}

// the over-relaxation factor of relax.hip and of bounds.hip's relaxed projection
inline int check_alpha(double alpha) {
  if (!std::isfinite(alpha) || !(alpha > 0.0 && alpha < 2.0))
    return admm_internal::fail(ADMM_E_INVALID, "alpha must be finite and in the open interval (0, 2)");
  return ADMM_OK;
}

// v[q] <- the block's sum of v[q], on every thread and in a fixed order: a shuffle-down tree at
// offsets 32 .. 1 inside each wave, then waves 0 .. 3 added ascending.  One barrier: `red` must not
// be in use by the caller.
template <int K>
__device__ __forceinline__ void block_sums(double (&v)[K], double (&red)[K][kThreads / 64]) {
#pragma unroll
  for (int q = 0; q < K; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < K; ++q) red[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < K; ++q) {
    double s = red[q][0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += red[q][w];
    v[q] = s;
  }
}

// out[r][q], r = first + blockIdx.x = the P block slots work[(r K + q) P ..] of row r, sum q:
// thread t adds slots t, t + 256, ... ascending, then the 256 thread sums are added ascending by
// one thread per sum.
template <int K>
__global__ __launch_bounds__(kThreads) void k_row_sums(const double* __restrict__ work, long long P, int first,
                                                       double* __restrict__ out) {
  __shared__ double part[K][kThreads];
  const size_t r = (size_t)first + blockIdx.x;
  const double* wk = work + r * K * (size_t)P;
  double a[K] = {};
  for (long long t = threadIdx.x; t < P; t += kThreads) {  // (the K loads of a pass are independent)
#pragma unroll
    for (int q = 0; q < K; ++q) a[q] += wk[(size_t)q * (size_t)P + (size_t)t];
  }
#pragma unroll
  for (int q = 0; q < K; ++q) part[q][threadIdx.x] = a[q];
  __syncthreads();
  if (threadIdx.x < K) {
    double s = part[threadIdx.x][0];
    for (int t = 1; t < kThreads; ++t) s += part[threadIdx.x][t];
    out[r * K + threadIdx.x] = s;
  }
}

}  // namespace admm

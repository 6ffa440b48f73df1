// bounds.hip -- projection onto the box lo <= x <= hi and its scaled dual (scope row f8,
// DESIGN.md 6.9).
//
// The reference solves eq.(1) over all of R^n (block_5_node_problem.py:21-29); attenuation is
// non-negative, bounded above and zero outside a known support.  Splitting x_i = w_i with
// w_i in [lo, hi] adds one more quadratic term (rho / 2) ||x - (w - f)||^2_{q_c} to node i's
// subproblem -- the shape of its edge terms, read by the unchanged x-update from one more row of z
// (w) and y (the scaled dual f) -- and replaces the edge midpoint of that row by the projection
//
//   l = max(lo, lo_map[p]),  h = min(hi, hi_map[p])          (a NULL map: the scalar alone)
//   t = x + f,   w' = t < l ? l : (t > h ? h : t),   f' = t - w'
//   out[v] = { sum (x - w')^2,  sum (w' - w)^2,  sum (x - P(x))^2 },   P the same clip of x
//
// per image v and pixel p: comparisons, not fmin / fmax, so that ties, +-0 and +-inf bounds have
// one defined result (t = -0 with l = 0 stays -0), and each of w', f' is one IEEE operation (the
// library is built without contraction).
//
// k_bound_project follows k_consensus<false> (kernels.hpp): one image per blockIdx.y, 1024 pixels
// per block, thread t takes pixels t, t + 256, t + 512, t + 768 of the block -- scalar 8-byte
// accesses, coalesced per wave, so rows of an odd pixel count (8-byte aligned only) need no special
// case.  x, f, w read and f, w written: 40 B per pixel-image; the maps add 16 B that every image
// of the batch shares (L2).  Each block's three sums go to its own slot of `work` (a shuffle tree
// per wave, then the waves ascending); k_bound_sum adds an image's slots in a fixed order.  No
// atomics: an image's w, f and sums depend on its pixels alone, not on nimg, its place in the
// batch or the strides.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/admm_tomo.h"

namespace admm_internal {
int fail(int code, const std::string& msg);
}

namespace {

using admm_internal::fail;

#define BHIPCHK(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t _e = (expr);                                                                               \
    if (_e != hipSuccess) return fail(ADMM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
  } while (0)

constexpr int kThreads = 256;
constexpr int kPer = 4;                      // pixels per thread
constexpr int kBlockPix = kThreads * kPer;   // 1024 pixels per block
constexpr int kMaxImg = 65535;               // gridDim.y
constexpr long long kMaxBlocks = 2147483647ll;  // gridDim.x
constexpr int kSums = 3;

}  // namespace

// (named namespace: the kernels keep their names in profiler output)
namespace admm {

static __device__ __forceinline__ double clip(double t, double l, double h) { return t < l ? l : (t > h ? h : t); }

// fixed-order sums of kSums values per thread: shuffle tree inside each wave, then the waves ascending
static __device__ __forceinline__ void block_sums(double (&v)[kSums], double (*red)[kThreads / 64]) {
#pragma unroll
  for (int q = 0; q < kSums; ++q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < kSums; ++q) red[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kSums; ++q) {
    double s = red[q][0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += red[q][w];
    v[q] = s;
  }
}

__global__ __launch_bounds__(kThreads) void k_bound_project(const double* __restrict__ x, long long x_stride,
                                                            double* __restrict__ w, double* __restrict__ f,
                                                            long long wf_stride, const double* __restrict__ lo_map,
                                                            const double* __restrict__ hi_map, double lo, double hi,
                                                            long long n, double* __restrict__ work) {
  __shared__ double red[kSums][kThreads / 64];
  const size_t v = blockIdx.y;
  const double* xv = x + v * (size_t)x_stride;
  double* wv = w + v * (size_t)wf_stride;
  double* fv = f + v * (size_t)wf_stride;
  const long long base = (long long)blockIdx.x * kBlockPix;
  double acc[kSums] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const long long p = base + u * kThreads + threadIdx.x;
    if (p < n) {
      const double xp = xv[p], fp = fv[p], wo = wv[p];
      double l = lo, h = hi;
      if (lo_map) {
        const double m = lo_map[p];
        l = m > l ? m : l;
      }
      if (hi_map) {
        const double m = hi_map[p];
        h = m < h ? m : h;
      }
      const double t = xp + fp;
      const double wn = clip(t, l, h);
      wv[p] = wn;
      fv[p] = t - wn;
      const double r = xp - wn, dw = wn - wo, vi = xp - clip(xp, l, h);
      acc[0] += r * r;
      acc[1] += dw * dw;
      acc[2] += vi * vi;
    }
  }
  block_sums(acc, red);
  if (threadIdx.x == 0) {
    const size_t P = gridDim.x;
#pragma unroll
    for (int q = 0; q < kSums; ++q) work[(v * kSums + q) * P + blockIdx.x] = acc[q];
  }
}

// out[v][q] = the P block slots of image v, sum q: thread t adds slots t, t + 256, ... ascending,
// then the 256 thread sums are added ascending by one thread per sum.
__global__ __launch_bounds__(kThreads) void k_bound_sum(const double* __restrict__ work, long long P,
                                                        double* __restrict__ out) {
  __shared__ double part[kSums][kThreads];
  const double* wk = work + (size_t)blockIdx.x * kSums * (size_t)P;
#pragma unroll
  for (int q = 0; q < kSums; ++q) {
    double a = 0.0;
    for (long long t = threadIdx.x; t < P; t += kThreads) a += wk[(size_t)q * (size_t)P + (size_t)t];
    part[q][threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double s = part[threadIdx.x][0];
    for (int t = 1; t < kThreads; ++t) s += part[threadIdx.x][t];
    out[(size_t)blockIdx.x * kSums + threadIdx.x] = s;
  }
}

}  // namespace admm

namespace {

using admm::k_bound_project;
using admm::k_bound_sum;

inline long long blocks_of(long long n) { return (n + kBlockPix - 1) / kBlockPix; }

int check_shape(long long n, int nimg) {
  if (n < 1 || blocks_of(n) > kMaxBlocks) return fail(ADMM_E_INVALID, "n must be in [1, 1024 * (2^31 - 1)]");
  if (nimg < 1 || nimg > kMaxImg) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  return ADMM_OK;
}

}  // namespace

extern "C" {

int admm_bound_project_work(long long n, int nimg, long long* n_doubles) {
  if (!n_doubles) return fail(ADMM_E_INVALID, "n_doubles is null");
  if (int rc = check_shape(n, nimg)) return rc;
  *n_doubles = (long long)kSums * blocks_of(n) * (long long)nimg;
  return ADMM_OK;
}

int admm_bound_project(const double* x, long long x_stride, double* w, double* f, long long wf_stride,
                       const double* lo_map, const double* hi_map, double lo, double hi, long long n, int nimg,
                       double* work, double* out, void* stream) {
  if (!x) return fail(ADMM_E_INVALID, "x is null");
  if (!w || !f) return fail(ADMM_E_INVALID, "w or f is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (int rc = check_shape(n, nimg)) return rc;
  if (x_stride < n || wf_stride < n) return fail(ADMM_E_INVALID, "x_stride and wf_stride must be >= n");
  if (lo != lo || hi != hi) return fail(ADMM_E_INVALID, "lo and hi must not be NaN");
  if (lo > hi) return fail(ADMM_E_INVALID, "lo > hi: the box is empty");
  hipStream_t s = (hipStream_t)stream;
  const long long P = blocks_of(n);
  hipLaunchKernelGGL(k_bound_project, dim3((unsigned)P, (unsigned)nimg), dim3(kThreads), 0, s, x, x_stride, w, f,
                     wf_stride, lo_map, hi_map, lo, hi, n, work);
  BHIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_bound_sum, dim3((unsigned)nimg), dim3(kThreads), 0, s, (const double*)work, P, out);
  BHIPCHK(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

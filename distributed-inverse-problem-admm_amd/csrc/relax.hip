// relax.hip -- over-relaxed edge and bound-constraint updates (scope row f9).
//
// Over-relaxation (Eckstein-Bertsekas; Boyd et al. 3.4.3) replaces x_i in the z- and y-updates of
// block_6_admm_loop_ver2.py:210-230 by  xh_i = alpha x_i + (1 - alpha) z_old,  0 < alpha < 2.  With
// om = 1 - alpha formed once on the host, per pixel of edge e = (a, b), a the lower endpoint:
//
//   hz  = om * z_old
//   xha = alpha * x_a + hz,   xhb = alpha * x_b + hz
//   midpoint:  aa = xha + y,  ab = xhb - y,    z' = (aa + ab) * 0.5
//   weighted:  aa = xha + y,  ab = xhb + y_b,  z' = (W_a * aa + W_b * ab) / (W_a + W_b),
//              y_b' = (y_b + xhb) - z'
//   y'  = (y + xha) - z'
//   RA2 += (x_a - z')^2,  RB2 += (x_b - z')^2,  DZ2 += (z' - z_old)^2        (the true x: r = x - z')
//
// and for the constraint slot of a bounded run (bounds.hip), whose projection is relaxed too:
//
//   xh = alpha * x + om * w,   t = xh + f,   w' = t < l ? l : (t > h ? h : t),   f' = t - w'
//   sums  (x - w')^2,  (w' - w)^2,  (x - clip(x))^2
//
// Every line is one IEEE float64 operation (the library is built without contraction).  alpha = 1
// gives om = 0, hz = +-0 and xha = x_a: the unrelaxed updates bit for bit on finite, nonzero data.
//
// The kernels have the shape of k_consensus<false> (kernels.hpp) and k_bound_project: one edge
// (image) per blockIdx.y, 1024 pixels per block, thread t takes pixels t, t + 256, t + 512, t + 768
// -- scalar 8-byte accesses, coalesced per wave, so rows of an odd pixel count need no special case.
// x_a, x_b, y, z read and y, z written: 48 B per pixel-edge, as the unrelaxed kernel (z_old, which
// that one reads for DZ2 alone, is the only new operand).  Each block's three sums go to its own slot
// of `work`, indexed by the edge's absolute slot (a shuffle tree per wave, then the waves ascending);
// k_relax_sum adds a row's slots in a fixed order.  No atomics: an edge's z', y' and sums depend on
// its own pixels alone, not on the range [e0, e1) it was launched in nor on its neighbours.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/admm_tomo.h"

namespace admm_internal {
int fail(int code, const std::string& msg);
}

namespace {

using admm_internal::fail;

#define RHIPCHK(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t _e = (expr);                                                                               \
    if (_e != hipSuccess) return fail(ADMM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
  } while (0)

constexpr int kThreads = 256;
constexpr int kPer = 4;                      // pixels per thread
constexpr int kBlockPix = kThreads * kPer;   // 1024 pixels per block
constexpr int kMaxY = 65535;                 // gridDim.y
constexpr long long kMaxBlocks = 2147483647ll;  // gridDim.x
constexpr int kSums = 3;

}  // namespace

// (named namespace: the kernels keep their names in profiler output)
namespace admm {

static __device__ __forceinline__ double rclip(double t, double l, double h) { return t < l ? l : (t > h ? h : t); }

// fixed-order sums of kSums values per thread: shuffle tree inside each wave, then the waves ascending
static __device__ __forceinline__ void relax_block_sums(double (&v)[kSums], double (*red)[kThreads / 64]) {
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

// edge slot e = e0 + blockIdx.y.  An edge whose endpoint row lies outside [0, n_rows) is left as it is
// and its sums are NaN: nothing outside x_ext is ever read.
template <bool WEIGHTED>
__global__ __launch_bounds__(kThreads) void k_consensus_relaxed(const double* __restrict__ xext, int n_rows,
                                                                double* __restrict__ y, double* __restrict__ yb,
                                                                double* __restrict__ z, const double* __restrict__ w,
                                                                const int* __restrict__ ea, const int* __restrict__ eb,
                                                                double alpha, double om, long long n, int e0,
                                                                double* __restrict__ work) {
  __shared__ double red[kSums][kThreads / 64];
  const size_t e = (size_t)e0 + blockIdx.y;
  const int ra = ea[e], rb = eb[e];
  const bool rows_ok = ra >= 0 && ra < n_rows && rb >= 0 && rb < n_rows;  // (uniform over the block)
  double acc[kSums] = {0.0, 0.0, 0.0};
  if (rows_ok) {
    const size_t eo = e * (size_t)n, ra_off = (size_t)ra * (size_t)n, rb_off = (size_t)rb * (size_t)n;
    const double* xa = xext + ra_off;
    const double* xb = xext + rb_off;
    const long long base = (long long)blockIdx.x * kBlockPix;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const long long p = base + u * kThreads + threadIdx.x;
      if (p < n) {
        const double xav = xa[p], xbv = xb[p], yv = y[eo + p], zo = z[eo + p];
        const double hz = om * zo;
        const double xha = alpha * xav + hz;
        const double xhb = alpha * xbv + hz;
        const double aa = xha + yv;
        double zn;
        if constexpr (WEIGHTED) {
          const double ybv = yb[eo + p];
          const double wa = w[ra_off + p], wb = w[rb_off + p];
          const double ab = xhb + ybv;
          zn = (wa * aa + wb * ab) / (wa + wb);
          yb[eo + p] = (ybv + xhb) - zn;
        } else {
          const double ab = xhb - yv;
          zn = (aa + ab) * 0.5;
        }
        y[eo + p] = (yv + xha) - zn;
        z[eo + p] = zn;
        const double r_a = xav - zn, r_b = xbv - zn, dz = zn - zo;
        acc[0] += r_a * r_a;
        acc[1] += r_b * r_b;
        acc[2] += dz * dz;
      }
    }
  }
  relax_block_sums(acc, red);
  if (threadIdx.x == 0) {
    const size_t P = gridDim.x;
#pragma unroll
    for (int q = 0; q < kSums; ++q) work[(e * kSums + q) * P + blockIdx.x] = rows_ok ? acc[q] : NAN;
  }
}

// k_bound_project (bounds.hip) around the relaxed image xh = alpha x + om w
__global__ __launch_bounds__(kThreads) void k_bound_project_relaxed(const double* __restrict__ x, long long x_stride,
                                                                    double* __restrict__ w, double* __restrict__ f,
                                                                    long long wf_stride,
                                                                    const double* __restrict__ lo_map,
                                                                    const double* __restrict__ hi_map, double lo,
                                                                    double hi, double alpha, double om, long long n,
                                                                    double* __restrict__ work) {
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
      const double ax = alpha * xp, ow = om * wo;
      const double xh = ax + ow;
      const double t = xh + fp;
      const double wn = rclip(t, l, h);
      wv[p] = wn;
      fv[p] = t - wn;
      const double r = xp - wn, dw = wn - wo, vi = xp - rclip(xp, l, h);
      acc[0] += r * r;
      acc[1] += dw * dw;
      acc[2] += vi * vi;
    }
  }
  relax_block_sums(acc, red);
  if (threadIdx.x == 0) {
    const size_t P = gridDim.x;
#pragma unroll
    for (int q = 0; q < kSums; ++q) work[(v * kSums + q) * P + blockIdx.x] = acc[q];
  }
}

// out[r][q], r = first + blockIdx.x = the P block slots of row r, sum q: thread t adds slots t, t + 256,
// ... ascending, then the 256 thread sums are added ascending by one thread per sum.
__global__ __launch_bounds__(kThreads) void k_relax_sum(const double* __restrict__ work, long long P, int first,
                                                        double* __restrict__ out) {
  __shared__ double part[kSums][kThreads];
  const size_t r = (size_t)first + blockIdx.x;
  const double* wk = work + r * kSums * (size_t)P;
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
    out[r * kSums + threadIdx.x] = s;
  }
}

}  // namespace admm

namespace {

using admm::k_bound_project_relaxed;
using admm::k_consensus_relaxed;
using admm::k_relax_sum;

inline long long blocks_of(long long n) { return (n + kBlockPix - 1) / kBlockPix; }

int check_n(long long n) {
  if (n < 1 || blocks_of(n) > kMaxBlocks) return fail(ADMM_E_INVALID, "n must be in [1, 1024 * (2^31 - 1)]");
  return ADMM_OK;
}

int check_alpha(double alpha) {
  if (!std::isfinite(alpha) || !(alpha > 0.0 && alpha < 2.0))
    return fail(ADMM_E_INVALID, "alpha must be finite and in the open interval (0, 2)");
  return ADMM_OK;
}

}  // namespace

extern "C" {

int admm_consensus_relaxed_work(long long n, int n_edges, long long* n_doubles) {
  if (!n_doubles) return fail(ADMM_E_INVALID, "n_doubles is null");
  if (int rc = check_n(n)) return rc;
  if (n_edges < 0) return fail(ADMM_E_INVALID, "n_edges must be >= 0");
  *n_doubles = (long long)kSums * blocks_of(n) * (long long)std::max(n_edges, 1);
  return ADMM_OK;
}

int admm_consensus_relaxed(const double* x_ext, long long n, int n_rows, double* y, double* y_b, double* z,
                           const double* w, const int32_t* edge_a, const int32_t* edge_b, int e0, int e1,
                           double alpha, double* work, double* edge_stats, void* stream) {
  if (!x_ext) return fail(ADMM_E_INVALID, "x_ext is null");
  if (!y || !z) return fail(ADMM_E_INVALID, "y or z is null");
  if (!edge_a || !edge_b) return fail(ADMM_E_INVALID, "edge_a or edge_b is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!edge_stats) return fail(ADMM_E_INVALID, "edge_stats is null");
  if ((y_b == nullptr) != (w == nullptr))
    return fail(ADMM_E_INVALID, "y_b and w come as a pair: both null (midpoint fusion) or both set (weighted)");
  if (e0 < 0 || e1 < e0) return fail(ADMM_E_INVALID, "edge slots need 0 <= e0 <= e1");
  if (int rc = check_n(n)) return rc;
  if (n_rows < 1) return fail(ADMM_E_INVALID, "n_rows must be >= 1");
  if (int rc = check_alpha(alpha)) return rc;
  if (e1 == e0) return ADMM_OK;
  hipStream_t s = (hipStream_t)stream;
  const long long P = blocks_of(n);
  const double om = 1.0 - alpha;
  for (int c0 = e0; c0 < e1; c0 += kMaxY) {  // (gridDim.y holds 65535 edges)
    const dim3 grid((unsigned)P, (unsigned)std::min(kMaxY, e1 - c0));
    if (w)
      hipLaunchKernelGGL(k_consensus_relaxed<true>, grid, dim3(kThreads), 0, s, x_ext, n_rows, y, y_b, z, w, edge_a,
                         edge_b, alpha, om, n, c0, work);
    else
      hipLaunchKernelGGL(k_consensus_relaxed<false>, grid, dim3(kThreads), 0, s, x_ext, n_rows, y, y_b, z, w, edge_a,
                         edge_b, alpha, om, n, c0, work);
    RHIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_relax_sum, dim3((unsigned)(e1 - e0)), dim3(kThreads), 0, s, (const double*)work, P, e0,
                     edge_stats);
  RHIPCHK(hipGetLastError());
  return ADMM_OK;
}

int admm_bound_project_relaxed(const double* x, long long x_stride, double* w, double* f, long long wf_stride,
                               const double* lo_map, const double* hi_map, double lo, double hi, long long n,
                               int nimg, double alpha, double* work, double* out, void* stream) {
  if (!x) return fail(ADMM_E_INVALID, "x is null");
  if (!w || !f) return fail(ADMM_E_INVALID, "w or f is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (int rc = check_n(n)) return rc;
  if (nimg < 1 || nimg > kMaxY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  if (x_stride < n || wf_stride < n) return fail(ADMM_E_INVALID, "x_stride and wf_stride must be >= n");
  if (lo != lo || hi != hi) return fail(ADMM_E_INVALID, "lo and hi must not be NaN");
  if (lo > hi) return fail(ADMM_E_INVALID, "lo > hi: the box is empty");
  if (int rc = check_alpha(alpha)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long long P = blocks_of(n);
  hipLaunchKernelGGL(k_bound_project_relaxed, dim3((unsigned)P, (unsigned)nimg), dim3(kThreads), 0, s, x, x_stride, w,
                     f, wf_stride, lo_map, hi_map, lo, hi, alpha, 1.0 - alpha, n, work);
  RHIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_relax_sum, dim3((unsigned)nimg), dim3(kThreads), 0, s, (const double*)work, P, 0, out);
  RHIPCHK(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

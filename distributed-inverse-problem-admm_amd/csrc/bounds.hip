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
// library is built without contraction).  In an over-relaxed run (scope row f9, DESIGN.md 6.10;
// the edges: relax.hip) the projection is taken around the relaxed image instead,
//
//   xh = alpha * x + om * w,   t = xh + f        (om = 1 - alpha formed once on the host)
//
// with the same w', f' and sums of the true x: admm_bound_project_relaxed, the same kernel body
// (k_bound_project<true>) and the same host path.  alpha = 1 gives the plain step bit for bit on
// finite, nonzero data.
//
// k_bound_project follows k_consensus<false> (kernels.hpp) in the launch shape of common.hpp: one
// image per blockIdx.y, 1024 pixels per block, thread t takes pixels t, t + 256, t + 512, t + 768
// of the block -- scalar 8-byte accesses, coalesced per wave, so rows of an odd pixel count (8-byte
// aligned only) need no special case.  x, f, w read and f, w written: 40 B per pixel-image; the
// maps add 16 B that every image of the batch shares (L2).  Each block's three sums go to its own
// slot of `work` (block_sums<3>); k_row_sums<3> adds an image's slots in a fixed order (both:
// common.hpp).  No atomics: an image's w, f and sums depend on its pixels alone, not on nimg, its
// place in the batch or the strides.
#include "common.hpp"

using namespace admm;

namespace {

using admm_internal::fail;

constexpr int kSums = 3;

}  // namespace

namespace admm {

static __device__ __forceinline__ double clip(double t, double l, double h) { return t < l ? l : (t > h ? h : t); }

// RELAXED: the projection around xh = alpha x + om w, om = 1 - alpha formed on the host; the plain
// instantiation never reads alpha and om.
template <bool RELAXED>
__global__ __launch_bounds__(kThreads) void k_bound_project(const double* __restrict__ x, long long x_stride,
                                                            double* __restrict__ w, double* __restrict__ f,
                                                            long long wf_stride, const double* __restrict__ lo_map,
                                                            const double* __restrict__ hi_map, double lo, double hi,
                                                            double alpha, double om, long long n,
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
      double t;
      if constexpr (RELAXED) {
        const double ax = alpha * xp, ow = om * wo;
        const double xh = ax + ow;
        t = xh + fp;
      } else {
        t = xp + fp;
      }
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

}  // namespace admm

namespace {

int check_shape(long long n, int nimg) {
  if (int rc = check_n(n)) return rc;
  if (nimg < 1 || nimg > kMaxGridY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  return ADMM_OK;
}

// the argument checks and the launch pair of both entry points (the plain one: alpha = 1, unread)
template <bool RELAXED>
int bound_project(const double* x, long long x_stride, double* w, double* f, long long wf_stride, const double* lo_map,
                  const double* hi_map, double lo, double hi, long long n, int nimg, double alpha, double* work,
                  double* out, void* stream) {
  if (!x) return fail(ADMM_E_INVALID, "x is null");
  if (!w || !f) return fail(ADMM_E_INVALID, "w or f is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (int rc = check_shape(n, nimg)) return rc;
  if (x_stride < n || wf_stride < n) return fail(ADMM_E_INVALID, "x_stride and wf_stride must be >= n");
  if (lo != lo || hi != hi) return fail(ADMM_E_INVALID, "lo and hi must not be NaN");
  if (lo > hi) return fail(ADMM_E_INVALID, "lo > hi: the box is empty");
  if (int rc = check_alpha(alpha)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long long P = blocks_of(n);
  hipLaunchKernelGGL(k_bound_project<RELAXED>, dim3((unsigned)P, (unsigned)nimg), dim3(kThreads), 0, s, x, x_stride, w,
                     f, wf_stride, lo_map, hi_map, lo, hi, alpha, 1.0 - alpha, n, work);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_row_sums<kSums>, dim3((unsigned)nimg), dim3(kThreads), 0, s, (const double*)work, P, 0, out);
  HIP_TRY(hipGetLastError());
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
  return bound_project<false>(x, x_stride, w, f, wf_stride, lo_map, hi_map, lo, hi, n, nimg, 1.0, work, out, stream);
}

int admm_bound_project_relaxed(const double* x, long long x_stride, double* w, double* f, long long wf_stride,
                               const double* lo_map, const double* hi_map, double lo, double hi, long long n,
                               int nimg, double alpha, double* work, double* out, void* stream) {
  return bound_project<true>(x, x_stride, w, f, wf_stride, lo_map, hi_map, lo, hi, n, nimg, alpha, work, out, stream);
}

}  // extern "C"

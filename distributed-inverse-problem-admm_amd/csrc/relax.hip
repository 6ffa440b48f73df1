// relax.hip -- the over-relaxed edge update (scope row f9).
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
// Every line is one IEEE float64 operation (the library is built without contraction).  alpha = 1
// gives om = 0, hz = +-0 and xha = x_a: the unrelaxed updates bit for bit on finite, nonzero data.
// The constraint slot of a bounded run is relaxed too: admm_bound_project_relaxed, bounds.hip.
//
// The kernel has the shape of k_consensus<false> (kernels.hpp) and k_bound_project, the launch
// shape of common.hpp: one edge per blockIdx.y, 1024 pixels per block, thread t takes pixels t,
// t + 256, t + 512, t + 768 -- scalar 8-byte accesses, coalesced per wave, so rows of an odd pixel
// count need no special case.  x_a, x_b, y, z read and y, z written: 48 B per pixel-edge, as the
// unrelaxed kernel (z_old, which that one reads for DZ2 alone, is the only new operand).  Each
// block's three sums go to its own slot of `work`, indexed by the edge's absolute slot
// (block_sums<3>); k_row_sums<3> adds a row's slots in a fixed order (both: common.hpp).  No
// atomics: an edge's z', y' and sums depend on its own pixels alone, not on the range [e0, e1) it
// was launched in nor on its neighbours.
#include <algorithm>

#include "common.hpp"

using namespace admm;

namespace {

using admm_internal::fail;

constexpr int kSums = 3;

}  // namespace

namespace admm {

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
  block_sums(acc, red);
  if (threadIdx.x == 0) {
    const size_t P = gridDim.x;
#pragma unroll
    for (int q = 0; q < kSums; ++q) work[(e * kSums + q) * P + blockIdx.x] = rows_ok ? acc[q] : NAN;
  }
}

}  // namespace admm

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
  for (int c0 = e0; c0 < e1; c0 += kMaxGridY) {  // (gridDim.y holds 65535 edges)
    const dim3 grid((unsigned)P, (unsigned)std::min(kMaxGridY, e1 - c0));
    if (w)
      hipLaunchKernelGGL(k_consensus_relaxed<true>, grid, dim3(kThreads), 0, s, x_ext, n_rows, y, y_b, z, w, edge_a,
                         edge_b, alpha, om, n, c0, work);
    else
      hipLaunchKernelGGL(k_consensus_relaxed<false>, grid, dim3(kThreads), 0, s, x_ext, n_rows, y, y_b, z, w, edge_a,
                         edge_b, alpha, om, n, c0, work);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_row_sums<kSums>, dim3((unsigned)(e1 - e0)), dim3(kThreads), 0, s, (const double*)work, P, e0,
                     edge_stats);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

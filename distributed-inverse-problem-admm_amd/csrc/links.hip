// links.hip -- the gated edge update of a run with unreliable links (scope row f14).
//
// At every iteration each edge slot e is up or down, up[e] != 0 or == 0 (one byte per slot, read
// from device memory: the schedule of a whole run is uploaded once and the host only moves the row
// pointer).  An up edge performs exactly the update of k_consensus<WEIGHTED> (kernels.hpp;
// RELAXED = false) or of k_consensus_relaxed<WEIGHTED> (relax.hip; RELAXED = true), operation for
// operation.  A down edge keeps y, z (and y_b) as they are -- nothing of them is written -- and
// reports its disagreement with the last agreed z:
//
//   RA2 = sum (x_a - z)^2,  RB2 = sum (x_b - z)^2,  DZ2 = +0
//
// The flag is uniform over a block (one edge per blockIdx.y), so the choice is a scalar branch.  Up:
// x_a, x_b, y, z read and y, z written, 48 B per pixel-edge as the ungated kernels; down: x_a, x_b, z
// read, 24 B.  The launch shape, the per-block sums in fixed slots of `work` (block_sums<3>) and the
// fixed-order sum per edge (k_row_sums<3>) are those of relax.hip (common.hpp).  No atomics: an edge's
// results depend on its own pixels and its own flag alone.
#include <algorithm>

#include "common.hpp"

using namespace admm;

namespace {

using admm_internal::fail;

constexpr int kSums = 3;

}  // namespace

namespace admm {

// edge slot e = e0 + blockIdx.y.  An edge whose endpoint row lies outside [0, n_rows) is left as it is
// and its sums are NaN, up or down: nothing outside x_ext is ever read.
template <bool WEIGHTED, bool RELAXED>
__global__ __launch_bounds__(kThreads) void k_consensus_gated(const double* __restrict__ xext, int n_rows,
                                                              double* __restrict__ y, double* __restrict__ yb,
                                                              double* __restrict__ z, const double* __restrict__ w,
                                                              const int* __restrict__ ea, const int* __restrict__ eb,
                                                              double alpha, double om, long long n, int e0,
                                                              const uint8_t* __restrict__ up,
                                                              double* __restrict__ work) {
  __shared__ double red[kSums][kThreads / 64];
  const size_t e = (size_t)e0 + blockIdx.y;
  const int ra = ea[e], rb = eb[e];
  const bool rows_ok = ra >= 0 && ra < n_rows && rb >= 0 && rb < n_rows;  // (uniform over the block)
  const bool is_up = up[e] != 0;                                          // (uniform over the block)
  double acc[kSums] = {0.0, 0.0, 0.0};
  if (rows_ok) {
    const size_t eo = e * (size_t)n, ra_off = (size_t)ra * (size_t)n, rb_off = (size_t)rb * (size_t)n;
    const double* xa = xext + ra_off;
    const double* xb = xext + rb_off;
    const long long base = (long long)blockIdx.x * kBlockPix;
    if (is_up) {
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const long long p = base + u * kThreads + threadIdx.x;
        if (p < n) {
          const double xav = xa[p], xbv = xb[p], yv = y[eo + p], zo = z[eo + p];
          double zn;
          if constexpr (RELAXED) {  // relax.hip, line for line
            const double hz = om * zo;
            const double xha = alpha * xav + hz;
            const double xhb = alpha * xbv + hz;
            const double aa = xha + yv;
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
          } else {  // k_consensus<WEIGHTED>, line for line
            if constexpr (WEIGHTED) {
              const double ybv = yb[eo + p];
              const double wa = w[ra_off + p], wb = w[rb_off + p];
              const double aa = xav + yv, ab = xbv + ybv;
              zn = (wa * aa + wb * ab) / (wa + wb);
              yb[eo + p] = ybv + xbv - zn;
            } else {
              const double aa = xav + yv, ab = xbv - yv;
              zn = (aa + ab) * 0.5;
            }
            y[eo + p] = yv + xav - zn;
          }
          z[eo + p] = zn;
          const double r_a = xav - zn, r_b = xbv - zn, dz = zn - zo;
          acc[0] += r_a * r_a;
          acc[1] += r_b * r_b;
          acc[2] += dz * dz;
        }
      }
    } else {  // down: the state keeps its bits; the residuals against the last agreed z
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const long long p = base + u * kThreads + threadIdx.x;
        if (p < n) {
          const double zo = z[eo + p];
          const double r_a = xa[p] - zo, r_b = xb[p] - zo;
          acc[0] += r_a * r_a;
          acc[1] += r_b * r_b;
        }
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

namespace {

template <bool WEIGHTED, bool RELAXED>
void launch_gated(dim3 grid, hipStream_t s, const double* x_ext, int n_rows, double* y, double* y_b, double* z,
                  const double* w, const int32_t* edge_a, const int32_t* edge_b, double alpha, double om,
                  long long n, int c0, const uint8_t* up, double* work) {
  hipLaunchKernelGGL((k_consensus_gated<WEIGHTED, RELAXED>), grid, dim3(kThreads), 0, s, x_ext, n_rows, y, y_b, z, w,
                     edge_a, edge_b, alpha, om, n, c0, up, work);
}

}  // namespace

extern "C" {

int admm_consensus_gated_work(long long n, int n_edges, long long* n_doubles) {
  if (!n_doubles) return fail(ADMM_E_INVALID, "n_doubles is null");
  if (int rc = check_n(n)) return rc;
  if (n_edges < 0) return fail(ADMM_E_INVALID, "n_edges must be >= 0");
  *n_doubles = (long long)kSums * blocks_of(n) * (long long)std::max(n_edges, 1);
  return ADMM_OK;
}

int admm_consensus_gated(const double* x_ext, long long n, int n_rows, double* y, double* y_b, double* z,
                         const double* w, const int32_t* edge_a, const int32_t* edge_b, int e0, int e1,
                         double alpha, const uint8_t* up, double* work, double* edge_stats, void* stream) {
  if (!x_ext) return fail(ADMM_E_INVALID, "x_ext is null");
  if (!y || !z) return fail(ADMM_E_INVALID, "y or z is null");
  if (!edge_a || !edge_b) return fail(ADMM_E_INVALID, "edge_a or edge_b is null");
  if (!up) return fail(ADMM_E_INVALID, "up is null");
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
  const bool relaxed = alpha != 1.0;
  for (int c0 = e0; c0 < e1; c0 += kMaxGridY) {  // (gridDim.y holds 65535 edges)
    const dim3 grid((unsigned)P, (unsigned)std::min(kMaxGridY, e1 - c0));
    if (w) {
      if (relaxed)
        launch_gated<true, true>(grid, s, x_ext, n_rows, y, y_b, z, w, edge_a, edge_b, alpha, om, n, c0, up, work);
      else
        launch_gated<true, false>(grid, s, x_ext, n_rows, y, y_b, z, w, edge_a, edge_b, alpha, om, n, c0, up, work);
    } else {
      if (relaxed)
        launch_gated<false, true>(grid, s, x_ext, n_rows, y, y_b, z, w, edge_a, edge_b, alpha, om, n, c0, up, work);
      else
        launch_gated<false, false>(grid, s, x_ext, n_rows, y, y_b, z, w, edge_a, edge_b, alpha, om, n, c0, up, work);
    }
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_row_sums<kSums>, dim3((unsigned)(e1 - e0)), dim3(kThreads), 0, s, (const double*)work, P, e0,
                     edge_stats);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

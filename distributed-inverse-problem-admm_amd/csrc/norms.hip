// norms.hip -- the three norms of the scale-free stop test (scope row f10).
//
// Boyd et al. (3.12) stop ADMM at  ||r|| <= sqrt(p) eps_abs + eps_rel max(||Ax||, ||Bz||)  and
// ||s|| <= sqrt(n) eps_abs + eps_rel ||A^T y||.  For the stacked constraint "x_i - z_e = 0 at both
// ends of every edge" the three norms have node-centric forms -- a node's batch stores every edge
// incident to it -- so they ride in the one-writer node statistics table.  Per image v < nimg (its
// row: x + v * x_stride) and pixel p, over the incidences q = inc_off[v] .. inc_off[v + 1] - 1 in
// ascending order:
//
//   e  = inc_edge[q]
//   yv = inc_sign[q] > 0 ? y[e][p] : (y_b ? y_b[e][p] : -y[e][p])
//   s  += yv                     (from +0)
//   zz += z[e][p] * z[e][p]      (from +0)
//
//   out[v] = { X2 = sum_p x^2,  Z2 = sum_p zz,  U2 = sum_p s * s }
//
//   ||Ax||^2 = sum_i ninc_i X2_i,   ||Bz||^2 = sum_i Z2_i,   ||A^T u||^2 = sum_i U2_i   (u: the scaled dual)
//
// Every line is one IEEE float64 operation (the library is built without contraction).  A bound
// constraint's slot (bounds.hip) is one more incidence with z row = w, y row = f and sign +1: no
// special case.  An isolated node has Z2 = U2 = +0.
//
// k_node_norms has the launch shape of k_bound_project (common.hpp): one image per blockIdx.y, 1024
// pixels per block, thread t takes pixels t, t + 256, t + 512, t + 768 of the block -- scalar 8-byte
// accesses, coalesced per wave, so rows of an odd pixel count need no special case.  The incidence
// loop is the outer one, so the four pixels' loads of an incidence are in flight together; each
// pixel's own operations keep the order above.  x and, per incidence, one y and one z row read:
// 8 (1 + 2 deg) B per pixel-node; only sums written.  Each block's three sums go to its own slot of
// `work` (block_sums<3>); k_row_sums<3> adds an image's slots in a fixed order.  No atomics: an
// image's sums depend on its pixels alone, not on nimg, its place in the batch or x_stride.
//
// The index arrays are device memory, which the host cannot check: an incidence whose slot lies
// outside [0, n_edges) -- or an incidence range that runs backwards -- is not dereferenced, and the
// node's three sums are NaN.
#include "common.hpp"

using namespace admm;

namespace {

using admm_internal::fail;

constexpr int kSums = 3;

int check_shape(long long n, int nimg) {
  if (int rc = check_n(n)) return rc;
  if (nimg < 1 || nimg > kMaxGridY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  return ADMM_OK;
}

}  // namespace

namespace admm {

__global__ __launch_bounds__(kThreads) void k_node_norms(const double* __restrict__ x, long long x_stride,
                                                         const double* __restrict__ y, const double* __restrict__ yb,
                                                         const double* __restrict__ z, long long n,
                                                         const int* __restrict__ inc_off,
                                                         const int* __restrict__ inc_edge,
                                                         const int* __restrict__ inc_sign, int n_edges,
                                                         double* __restrict__ work) {
  __shared__ double red[kSums][kThreads / 64];
  const size_t v = blockIdx.y;
  const double* xv = x + v * (size_t)x_stride;
  const int q0 = inc_off[v], q1 = inc_off[v + 1];
  const long long base = (long long)blockIdx.x * kBlockPix;
  bool ok = q0 >= 0 && q1 >= q0;  // (uniform over the node's blocks: all of them write NaN or none)
  double s[kPer] = {0.0, 0.0, 0.0, 0.0}, zz[kPer] = {0.0, 0.0, 0.0, 0.0};
  for (int q = q0; ok && q < q1; ++q) {
    const int e = inc_edge[q];
    if (e < 0 || e >= n_edges) {
      ok = false;
      break;
    }
    const bool lower = inc_sign[q] > 0;
    const size_t eo = (size_t)e * (size_t)n;
    const double* yr = (lower || !yb) ? y + eo : yb + eo;
    const bool neg = !lower && !yb;
    const double* zr = z + eo;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const long long p = base + u * kThreads + threadIdx.x;
      if (p < n) {
        const double yl = yr[p], zv = zr[p];
        const double yv = neg ? -yl : yl;
        s[u] += yv;
        zz[u] += zv * zv;
      }
    }
  }
  double acc[kSums] = {0.0, 0.0, 0.0};
  if (ok) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const long long p = base + u * kThreads + threadIdx.x;
      if (p < n) {
        const double xp = xv[p];
        acc[0] += xp * xp;
        acc[1] += zz[u];
        acc[2] += s[u] * s[u];
      }
    }
  }
  block_sums(acc, red);
  if (threadIdx.x == 0) {
    const size_t P = gridDim.x;
#pragma unroll
    for (int q = 0; q < kSums; ++q) work[(v * kSums + q) * P + blockIdx.x] = ok ? acc[q] : NAN;
  }
}

}  // namespace admm

extern "C" {

int admm_node_norms_work(long long n, int nimg, long long* n_doubles) {
  if (!n_doubles) return fail(ADMM_E_INVALID, "n_doubles is null");
  if (int rc = check_shape(n, nimg)) return rc;
  *n_doubles = (long long)kSums * blocks_of(n) * (long long)nimg;
  return ADMM_OK;
}

int admm_node_norms(const double* x, long long x_stride, const double* y, const double* y_b, const double* z,
                    long long n, int nimg, const int32_t* inc_off, const int32_t* inc_edge, const int32_t* inc_sign,
                    int n_edges, double* work, double* out, void* stream) {
  if (!x) return fail(ADMM_E_INVALID, "x is null");
  if (!inc_off) return fail(ADMM_E_INVALID, "inc_off is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (n_edges < 0) return fail(ADMM_E_INVALID, "n_edges must be >= 0");
  if (n_edges > 0 && (!y || !z)) return fail(ADMM_E_INVALID, "y or z is null with n_edges > 0");
  if (n_edges > 0 && (!inc_edge || !inc_sign))
    return fail(ADMM_E_INVALID, "inc_edge or inc_sign is null with n_edges > 0");
  if (int rc = check_shape(n, nimg)) return rc;
  if (x_stride < n) return fail(ADMM_E_INVALID, "x_stride must be >= n");
  hipStream_t s = (hipStream_t)stream;
  const long long P = blocks_of(n);
  hipLaunchKernelGGL(k_node_norms, dim3((unsigned)P, (unsigned)nimg), dim3(kThreads), 0, s, x, x_stride, y, y_b, z, n,
                     inc_off, inc_edge, inc_sign, n_edges, work);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_row_sums<kSums>, dim3((unsigned)nimg), dim3(kThreads), 0, s, (const double*)work, P, 0, out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

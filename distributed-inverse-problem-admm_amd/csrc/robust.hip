// robust.hip -- the Huber data term by reweighted rays (scope row f12).
//
// Node i minimises sum_r omega_r psi_delta((A x - b)_r) + ..., psi_delta(a) = a^2 / 2 for |a| <= delta
// and delta |a| - delta^2 / 2 beyond.  Majorise-minimise: after an x-update the residual gives
// h_r = 1 where |r_r| <= delta, else delta / |r_r|, and the next x-update is the weighted least-squares
// update with omega^eff = omega h (admm_batch_update_ray_weights).  A fixed point satisfies
// A^T (omega^eff r) = A^T (omega psi'_delta(r)): the Huber problem's stationarity.
//
// Per image v < nimg and ray p < m, T the sample type, every line one IEEE operation (the library is
// built without contraction), so a NumPy restatement is bitwise:
//
//   r     = ax - b                                   (T)
//   a     = |(double)r|
//   h64   = a <= delta ? 1.0 : delta / a
//   h     = (T)h64
//   w_out = w ? w * h (T) : h
//   psi   = a <= delta ? 0.5 * (a * a) : delta * a - hd      hd = 0.5 * (delta * delta), from the host
//
//   out[v] = { sum_p (double)w psi,  #{p : w != 0 and a > delta} }
//
// A ray with w == 0 is masked: w_out = 0, its term is +0 whatever ax and b hold (NaN included), and it
// is never counted.  A NaN residual of an unmasked ray propagates into w_out and the loss; it is not
// counted (a > delta is false).  delta = +inf: every h = 1, w_out is w (or 1) bitwise, no outlier.
//
// k_huber_weights has the launch shape of common.hpp: one image per blockIdx.y, 1024 rays per block,
// thread t takes rays t, t + 256, t + 512, t + 768 of the block -- scalar accesses of the sample type,
// coalesced per wave, so rows of an odd ray count need no special case.  2 (3 with w) sample arrays
// read, 1 written.  Each block's two sums go to its own slot of `work` (block_sums<2>);
// k_row_sums<2> adds an image's slots in a fixed order.  No atomics: an image's results depend on its
// rays alone, not on nimg or its place in the batch.
#include "common.hpp"

using namespace admm;

namespace {

using admm_internal::fail;

constexpr int kSums = 2;  // the weighted Huber value, the outlier count

int check_shape(long long m, int nimg) {
  if (int rc = check_n(m)) return rc;
  if (nimg < 1 || nimg > kMaxGridY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  return ADMM_OK;
}

}  // namespace

namespace admm {

// kDev: the image's threshold is delta_dev[v * delta_stride] and hd is formed here, by the host's expression
template <typename T, bool kDev>
__global__ __launch_bounds__(kThreads) void k_huber_weights(const T* __restrict__ ax, const T* __restrict__ b,
                                                            const T* __restrict__ w, T* __restrict__ w_out,
                                                            long long m, double delta, double hd,
                                                            const double* __restrict__ delta_dev,
                                                            long long delta_stride, double* __restrict__ work) {
  __shared__ double red[kSums][kThreads / 64];
  const size_t v = blockIdx.y;
  if (kDev) {
    delta = delta_dev[v * (size_t)delta_stride];
    hd = 0.5 * (delta * delta);
  }
  const size_t row = v * (size_t)m;
  const long long base = (long long)blockIdx.x * kBlockPix;
  double acc[kSums] = {0.0, 0.0};
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const long long p = base + u * kThreads + threadIdx.x;
    if (p < m) {
      const size_t i = row + (size_t)p;
      const T r = ax[i] - b[i];
      const double a = fabs((double)r);
      const bool inl = a <= delta;
      const double h64 = inl ? 1.0 : delta / a;
      const T h = (T)h64;
      const double psi = inl ? 0.5 * (a * a) : delta * a - hd;
      T wo = h;
      double term = psi;
      bool counted = a > delta;
      if (w) {
        const T wv = w[i];
        if (wv == (T)0) {  // masked
          wo = (T)0;
          term = 0.0;
          counted = false;
        } else {
          wo = wv * h;
          term = (double)wv * psi;
        }
      }
      w_out[i] = wo;
      acc[0] += term;
      acc[1] += counted ? 1.0 : 0.0;
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

// the checks and the two launches both entry points share; delta_dev == nullptr: the host's delta
int huber_launch(const void* ax, const void* b, const void* w, void* w_out, int dtype, long long m, int nimg,
                 double delta, const double* delta_dev, long long delta_stride, double* work, double* out,
                 void* stream) {
  if (!ax) return fail(ADMM_E_INVALID, "ax is null");
  if (!b) return fail(ADMM_E_INVALID, "b is null");
  if (!w_out) return fail(ADMM_E_INVALID, "w_out is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (w_out == ax || w_out == b || w_out == w) return fail(ADMM_E_INVALID, "w_out must be distinct from ax, b and w");
  if (dtype != ADMM_DTYPE_F32 && dtype != ADMM_DTYPE_F64)
    return fail(ADMM_E_INVALID, "dtype must be ADMM_DTYPE_F32 or ADMM_DTYPE_F64");
  if (!delta_dev && (std::isnan(delta) || !(delta > 0.0)))
    return fail(ADMM_E_INVALID, "delta must be > 0 (+inf allowed), not NaN");
  if (int rc = check_shape(m, nimg)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long long P = blocks_of(m);
  const double hd = 0.5 * (delta * delta);
  const dim3 grid((unsigned)P, (unsigned)nimg);
#define ADMM_HUBER_LAUNCH(T, DEV)                                                                             \
  hipLaunchKernelGGL((k_huber_weights<T, DEV>), grid, dim3(kThreads), 0, s, (const T*)ax, (const T*)b,        \
                     (const T*)w, (T*)w_out, m, delta, hd, delta_dev, delta_stride, work)
  if (dtype == ADMM_DTYPE_F64) {
    if (delta_dev) ADMM_HUBER_LAUNCH(double, true); else ADMM_HUBER_LAUNCH(double, false);
  } else {
    if (delta_dev) ADMM_HUBER_LAUNCH(float, true); else ADMM_HUBER_LAUNCH(float, false);
  }
#undef ADMM_HUBER_LAUNCH
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_row_sums<kSums>, dim3((unsigned)nimg), dim3(kThreads), 0, s, (const double*)work, P, 0, out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // namespace

extern "C" {

int admm_huber_weights_work(long long m, int nimg, long long* n_doubles) {
  if (!n_doubles) return fail(ADMM_E_INVALID, "n_doubles is null");
  if (int rc = check_shape(m, nimg)) return rc;
  *n_doubles = (long long)kSums * blocks_of(m) * (long long)nimg;
  return ADMM_OK;
}

int admm_huber_weights(const void* ax, const void* b, const void* w, void* w_out, int dtype, long long m, int nimg,
                       double delta, double* work, double* out, void* stream) {
  return huber_launch(ax, b, w, w_out, dtype, m, nimg, delta, nullptr, 0, work, out, stream);
}

int admm_huber_weights_dev(const void* ax, const void* b, const void* w, void* w_out, int dtype, long long m,
                           int nimg, const double* delta, long long delta_stride, double* work, double* out,
                           void* stream) {
  if (!delta) return fail(ADMM_E_INVALID, "delta is null");
  if (delta_stride < 1) return fail(ADMM_E_INVALID, "delta_stride must be >= 1");
  if (delta == out || (const void*)delta == w_out)
    return fail(ADMM_E_INVALID, "delta must be distinct from out and w_out");
  return huber_launch(ax, b, w, w_out, dtype, m, nimg, 1.0, delta, delta_stride, work, out, stream);
}

}  // extern "C"

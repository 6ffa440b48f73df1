// fbp.hip -- ramp filter of filtered back projection (setup path, DESIGN.md 6.6, scope row f5).
//
// The reference's legacy loader reserves the key `agg_fbp_recon` for an "optional FBP
// reconstruction" (block_2_test.py:11,77) and never fills it.  FBP here is
//   x = A^T q,   q[t][j] = scale * tau * sum_k sino[t][k] * h[j - k]
// with A^T the exact adjoint admm_project_adj (unchanged) and this file the filter: a direct
// convolution along the detector axis with the spatial taps of the band-limited ramp (cutoff
// 1/(2 tau)), optionally windowed.  A direct sum rather than an FFT: n_det <= 4096, the row and
// the taps fit in LDS, and a fixed ascending-k fma chain per output bin makes a row's result
// independent of the batch around it.
//
//   Ram-Lak      h[0] = 1/(4 tau^2), h[k] = -1/(pi^2 k^2 tau^2) (k odd), 0 (k even)
//   Shepp-Logan  h[k] = -2/(pi^2 tau^2 (4 k^2 - 1))
//   Hann         h[k] = rl[k]/2 + (rl[k-1] + rl[k+1])/4   (window (1 + cos 2 pi f tau)/2)
#include <cstdint>

#include "common.hpp"

namespace {

using admm_internal::fail;

constexpr int kMaxDet = 4096;  // the library's N limit: row + taps = 2 x 32 KiB of LDS
constexpr int kThreads = 256;
constexpr int kOut = 4;  // output bins per thread and pass: one broadcast row read serves 4 fmas
constexpr double kPi = 3.14159265358979323846;

// Ram-Lak tap |k| (IEEE divisions; admm_hip/fbp.py filter_taps states the same expressions)
__device__ __forceinline__ double ramlak(int k, double tau) {
  if (k == 0) return 1.0 / (4.0 * (tau * tau));
  if ((k & 1) == 0) return 0.0;
  const double kk = (double)k * (double)k;
  return -1.0 / (((kPi * kPi) * kk) * (tau * tau));
}

__device__ __forceinline__ double tap(int k, double tau, int filter) {
  if (filter == ADMM_FBP_SHEPP_LOGAN) {
    const double kk = (double)k * (double)k;
    return -2.0 / (((kPi * kPi) * (tau * tau)) * (4.0 * kk - 1.0));
  }
  if (filter == ADMM_FBP_HANN) {
    const int km = k == 0 ? 1 : k - 1;  // rl is even: rl[-1] = rl[1]
    return 0.5 * ramlak(k, tau) + 0.25 * (ramlak(km, tau) + ramlak(k + 1, tau));
  }
  return ramlak(k, tau);
}

// One block per (image, angle) row.  LDS: the row as float64 [n_det], then the taps h[0 .. n_det-1].
// Thread t owns bins t, t + 256, ...; kOut of them per pass share each broadcast read of row[k].
// The tap index |j - k| is consecutive over the lanes on either side of the diagonal, so the
// 8-byte tap reads are conflict-free (two-way for the one lane group the diagonal crosses).
template <typename T>
__global__ __launch_bounds__(kThreads) void k_fbp_filter(const T* __restrict__ sino, T* __restrict__ out, int n_det,
                                                         double tau, double gain, int filter) {
  extern __shared__ double lds[];
  double* row = lds;
  double* h = lds + n_det;
  const size_t base = (size_t)blockIdx.x * (size_t)n_det;
  for (int k = threadIdx.x; k < n_det; k += kThreads) {
    row[k] = (double)sino[base + k];
    h[k] = tap(k, tau, filter);
  }
  __syncthreads();
  for (int j0 = threadIdx.x; j0 < n_det; j0 += kOut * kThreads) {
    int j[kOut];
    double acc[kOut];
#pragma unroll
    for (int r = 0; r < kOut; ++r) {
      j[r] = min(j0 + r * kThreads, n_det - 1);  // bins past the row recompute the last one, unstored
      acc[r] = 0.0;
    }
    for (int k = 0; k < n_det; ++k) {
      const double v = row[k];
#pragma unroll
      for (int r = 0; r < kOut; ++r) acc[r] = fma(v, h[abs(j[r] - k)], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < kOut; ++r) {
      const int jr = j0 + r * kThreads;
      if (jr < n_det) out[base + jr] = (T)(gain * acc[r]);
    }
  }
}

}  // namespace

extern "C" {

int admm_fbp_filter(const void* sino, void* out, int dtype, int n_angles, int n_det, int nimg, double det_spacing,
                    double scale, int filter, void* stream) {
  if (!sino) return fail(ADMM_E_INVALID, "sino is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (out == sino) return fail(ADMM_E_INVALID, "out must not alias sino (a row is read after its bins are written)");
  if (dtype != ADMM_DTYPE_F32 && dtype != ADMM_DTYPE_F64) return fail(ADMM_E_INVALID, "dtype must be ADMM_DTYPE_F32 / _F64");
  if (filter != ADMM_FBP_RAMLAK && filter != ADMM_FBP_SHEPP_LOGAN && filter != ADMM_FBP_HANN)
    return fail(ADMM_E_INVALID, "filter must be one of ADMM_FBP_RAMLAK / _SHEPP_LOGAN / _HANN");
  if (n_det < 1 || n_det > kMaxDet) return fail(ADMM_E_INVALID, "n_det must be in [1, 4096]");
  if (n_angles < 1) return fail(ADMM_E_INVALID, "n_angles must be >= 1");
  if (nimg < 1) return fail(ADMM_E_INVALID, "nimg must be >= 1");
  const long long rows = (long long)nimg * (long long)n_angles;
  if (rows * (long long)n_det >= (1ll << 31)) return fail(ADMM_E_INVALID, "nimg * n_angles * n_det must be < 2^31");
  if (!(det_spacing > 0.0)) return fail(ADMM_E_INVALID, "det_spacing must be > 0");
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = 2 * (size_t)n_det * sizeof(double);  // <= 64 KiB
  const double gain = scale * det_spacing;
  if (dtype == ADMM_DTYPE_F64)
    hipLaunchKernelGGL((k_fbp_filter<double>), dim3((unsigned)rows), dim3(kThreads), lds, s, (const double*)sino,
                       (double*)out, n_det, det_spacing, gain, filter);
  else
    hipLaunchKernelGGL((k_fbp_filter<float>), dim3((unsigned)rows), dim3(kThreads), lds, s, (const float*)sino,
                       (float*)out, n_det, det_spacing, gain, filter);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

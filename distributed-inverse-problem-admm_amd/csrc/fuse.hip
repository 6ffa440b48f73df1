// fuse.hip -- the network-fused image and the consensus error (scope row f11).
//
// The fused image is the weighted mean over ALL graph nodes, xbar = (sum_i w_i x_i) / (sum_i w_i)
// per pixel (w_i = 1: the plain mean).  The nodes live in different device batches, streams and
// ranks, and a run must be bitwise the same however they are grouped, so the sums over nodes are
// fixed-point: exact in int64 and therefore independent of order.  fixed_sum(t) of terms t_i[p],
// over all v_total nodes and p < n, every line one IEEE float64 operation:
//
//   B = max_{i,p} |t_i[p]|                  a NaN or +-inf term: B = +inf and every output is NaN
//   B == 0: s = 0;  else B = m 2^e, 0.5 <= m < 1 (frexp),  L = bit_length(v_total - 1),  s = 61 - e - L
//   q_i[p] = llrint(ldexp(t_i[p], s))       |q| <= 2^(61 - L): v_total of them cannot overflow int64
//   S[p]   = sum_i q_i[p]                   int64: exact, associative
//   fixed_sum[p] = ldexp((double)S[p], -s)  the conversion rounds to nearest even
//
// and from it  Nn = fixed_sum(w x),  Dn = fixed_sum(w)  (v_total for w = 1),  xbar = Nn / Dn,
// spread = sqrt(fixed_sum(w ((x - xbar) (x - xbar))) / Dn),  dev2_i = sum_p (x_i[p] - xbar[p])^2.
//
// Resolution: every pixel shares the one grid 2^-s, so a sum is within v_total 2^-s <= 2 v_total^2 B
// 2^-61 of the exact sum of its terms -- relative to the largest term of the whole network, not to
// the pixel: one wild pixel coarsens every pixel's grid.  With B within a few powers of two of the
// typical values the grid is finer than double.
//
// Launch shape of k_bound_project / k_node_norms (common.hpp): 256 threads, 1024 pixels per block,
// thread t takes pixels t, t + 256, t + 512, t + 768 -- scalar 8-byte accesses, so rows of an odd n
// need no special case.  No atomics anywhere.
//
//   k_fuse_absmax      grid (ceil(n / 1024), nimg): each block's max |t| (non-finite -> +inf) to its slot
//                      of `work`; k_fuse_max folds the slots into out[0] = max(out[0], .), so calls chain.
//   k_fuse_accumulate  grid ceil(n / 1024): one thread per pixel loops over the batch's images in groups
//                      of four -- the group's loads (x and w of four images for four pixels) are issued
//                      before the dependent conversions -- and adds the group's q to acc[p] in place.
//                      It derives s from the device value of B itself: the host never reads B.
//   k_fuse_finish      one thread per pixel: ldexp, the division (and the spread's sqrt), the NaN rule.
//   k_fuse_deviation   grid (ceil(n / 1024), nimg): block sums of (x - mean)^2 to fixed slots of `work`
//                      (block_sums<1>), then k_row_sums<1>: an image's dev2 depends on its pixels alone.
#include "common.hpp"

using namespace admm;

namespace {

using admm_internal::fail;

constexpr int kModeWX = 0, kModeW = 1, kModeWD2 = 2;
constexpr int kGroup = 4;  // images whose loads one thread keeps in flight together
constexpr int kMaxVTotal = 1 << 30;

int check_shape(long long n, int nimg) {
  if (int rc = check_n(n)) return rc;
  if (nimg < 1 || nimg > kMaxGridY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  return ADMM_OK;
}

int check_terms(const double* x, long long x_stride, const double* w, long long w_stride, const double* m,
                long long n, int nimg, int mode) {
  if (mode != kModeWX && mode != kModeW && mode != kModeWD2)
    return fail(ADMM_E_INVALID, "mode must be 0 (w x), 1 (w) or 2 (w (x - m)^2)");
  if (mode != kModeW && !x) return fail(ADMM_E_INVALID, "x is null");
  if (mode == kModeWD2 && !m) return fail(ADMM_E_INVALID, "m is null with mode 2");
  if (int rc = check_shape(n, nimg)) return rc;
  if (mode != kModeW && x_stride < n) return fail(ADMM_E_INVALID, "x_stride must be >= n");
  if (w && w_stride < n) return fail(ADMM_E_INVALID, "w_stride must be >= n");
  return ADMM_OK;
}

int check_v_total(int v_total) {
  if (v_total < 1 || v_total > kMaxVTotal) return fail(ADMM_E_INVALID, "v_total must be in [1, 2^30]");
  return ADMM_OK;
}

}  // namespace

namespace admm {

// the term of one image at one pixel; xv, wv, mv are loaded values (wv = 1 without weights)
template <int MODE>
__device__ __forceinline__ double fuse_term(double xv, double wv, double mv, bool weighted) {
  if (MODE == kModeW) return wv;
  if (MODE == kModeWX) return weighted ? wv * xv : xv;
  const double d = xv - mv;
  const double dd = d * d;
  return weighted ? wv * dd : dd;
}

// s of B and v_total; false: B is not finite (every output of the sum is NaN)
__device__ __forceinline__ bool fuse_shift(double B, int v_total, int* s) {
  if (!(B < INFINITY)) return false;
  *s = 0;
  if (B != 0.0) {
    int e;
    (void)frexp(B, &e);
    const int L = v_total > 1 ? 32 - __clz(v_total - 1) : 0;
    *s = 61 - e - L;
  }
  return true;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_fuse_absmax(const double* __restrict__ x, long long x_stride,
                                                          const double* __restrict__ w, long long w_stride,
                                                          const double* __restrict__ m, long long n,
                                                          double* __restrict__ work) {
  __shared__ double red[kThreads / 64];
  const size_t v = blockIdx.y;
  const double* xv = MODE != kModeW ? x + v * (size_t)x_stride : nullptr;
  const double* wv = w ? w + v * (size_t)w_stride : nullptr;
  const long long base = (long long)blockIdx.x * kBlockPix;
  double b = 0.0;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const long long p = base + u * kThreads + threadIdx.x;
    if (p < n) {
      const double xp = MODE != kModeW ? xv[p] : 0.0;
      const double wp = wv ? wv[p] : 1.0;
      const double mp = MODE == kModeWD2 ? m[p] : 0.0;
      const double a = fabs(fuse_term<MODE>(xp, wp, mp, wv != nullptr));
      b = fmax(b, a < INFINITY ? a : INFINITY);  // (NaN -> +inf; b is never NaN)
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) b = fmax(b, __shfl_down(b, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kThreads / 64; ++k) b = fmax(b, red[k]);
    work[v * gridDim.x + blockIdx.x] = b;
  }
}

// out[0] <- max(out[0], work[0 .. cnt)); a NaN already in out[0] becomes +inf
__global__ __launch_bounds__(kThreads) void k_fuse_max(const double* __restrict__ work, long long cnt,
                                                       double* __restrict__ out) {
  __shared__ double red[kThreads / 64];
  double b = 0.0;
  for (long long t = threadIdx.x; t < cnt; t += kThreads) b = fmax(b, work[t]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) b = fmax(b, __shfl_down(b, off, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kThreads / 64; ++k) b = fmax(b, red[k]);
    const double prev = out[0];
    out[0] = prev >= 0.0 ? fmax(prev, b) : INFINITY;
  }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_fuse_accumulate(const double* __restrict__ x, long long x_stride,
                                                              const double* __restrict__ w, long long w_stride,
                                                              const double* __restrict__ m, long long n, int nimg,
                                                              const double* __restrict__ bmax, int v_total,
                                                              long long* __restrict__ acc) {
  int s;
  if (!fuse_shift(bmax[0], v_total, &s)) return;  // the finish writes NaN; acc is not read
  const long long base = (long long)blockIdx.x * kBlockPix;
  const bool weighted = w != nullptr;
  double mp[kPer] = {0.0, 0.0, 0.0, 0.0};
  if (MODE == kModeWD2) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const long long p = base + u * kThreads + threadIdx.x;
      if (p < n) mp[u] = m[p];
    }
  }
  long long S[kPer] = {0, 0, 0, 0};
  for (int v0 = 0; v0 < nimg; v0 += kGroup) {
    double xv[kGroup][kPer], wv[kGroup][kPer];
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
      const bool on = v0 + g < nimg;
      const size_t v = on ? v0 + g : 0;
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const long long p = base + u * kThreads + threadIdx.x;
        const bool in = on && p < n;
        xv[g][u] = (MODE != kModeW && in) ? x[v * (size_t)x_stride + p] : 0.0;
        wv[g][u] = (weighted && in) ? w[v * (size_t)w_stride + p] : 1.0;
      }
    }
#pragma unroll
    for (int g = 0; g < kGroup; ++g) {
      if (v0 + g < nimg) {
#pragma unroll
        for (int u = 0; u < kPer; ++u) S[u] += llrint(ldexp(fuse_term<MODE>(xv[g][u], wv[g][u], mp[u], weighted), s));
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const long long p = base + u * kThreads + threadIdx.x;
    if (p < n) acc[p] += S[u];
  }
}

// out[p] = Nn / Dn, or its square root; NaN everywhere when a B is not finite
__global__ __launch_bounds__(kThreads) void k_fuse_finish(const long long* __restrict__ acc_num,
                                                          const double* __restrict__ bmax_num,
                                                          const long long* __restrict__ acc_den,
                                                          const double* __restrict__ bmax_den, int v_total,
                                                          long long n, int root, double* __restrict__ out) {
  int sn = 0, sd = 0;
  bool ok = fuse_shift(bmax_num[0], v_total, &sn);
  if (acc_den) ok = fuse_shift(bmax_den[0], v_total, &sd) && ok;
  const long long base = (long long)blockIdx.x * kBlockPix;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const long long p = base + u * kThreads + threadIdx.x;
    if (p < n) {
      double r = NAN;
      if (ok) {
        const double num = ldexp((double)acc_num[p], -sn);
        const double den = acc_den ? ldexp((double)acc_den[p], -sd) : (double)v_total;
        r = num / den;
        if (root) r = sqrt(r);
      }
      out[p] = r;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_fuse_deviation(const double* __restrict__ x, long long x_stride,
                                                             const double* __restrict__ mean, long long n,
                                                             double* __restrict__ work) {
  __shared__ double red[1][kThreads / 64];
  const size_t v = blockIdx.y;
  const double* xv = x + v * (size_t)x_stride;
  const long long base = (long long)blockIdx.x * kBlockPix;
  double acc[1] = {0.0};
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const long long p = base + u * kThreads + threadIdx.x;
    if (p < n) {
      const double d = xv[p] - mean[p];
      acc[0] += d * d;
    }
  }
  block_sums(acc, red);
  if (threadIdx.x == 0) work[v * gridDim.x + blockIdx.x] = acc[0];
}

}  // namespace admm

namespace {

template <int MODE>
void launch_absmax(const double* x, long long x_stride, const double* w, long long w_stride, const double* m,
                   long long n, int nimg, double* work, hipStream_t s) {
  hipLaunchKernelGGL(k_fuse_absmax<MODE>, dim3((unsigned)blocks_of(n), (unsigned)nimg), dim3(kThreads), 0, s, x,
                     x_stride, w, w_stride, m, n, work);
}

template <int MODE>
void launch_accumulate(const double* x, long long x_stride, const double* w, long long w_stride, const double* m,
                       long long n, int nimg, const double* bmax, int v_total, long long* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_fuse_accumulate<MODE>, dim3((unsigned)blocks_of(n)), dim3(kThreads), 0, s, x, x_stride, w,
                     w_stride, m, n, nimg, bmax, v_total, acc);
}

}  // namespace

extern "C" {

int admm_fuse_absmax_work(long long n, int nimg, long long* n_doubles) {
  if (!n_doubles) return fail(ADMM_E_INVALID, "n_doubles is null");
  if (int rc = check_shape(n, nimg)) return rc;
  *n_doubles = blocks_of(n) * (long long)nimg;
  return ADMM_OK;
}

int admm_fuse_deviation_work(long long n, int nimg, long long* n_doubles) {
  return admm_fuse_absmax_work(n, nimg, n_doubles);
}

int admm_fuse_absmax(const double* x, long long x_stride, const double* w, long long w_stride, const double* m,
                     long long n, int nimg, int mode, double* work, double* out, void* stream) {
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (int rc = check_terms(x, x_stride, w, w_stride, m, n, nimg, mode)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (mode == kModeWX) launch_absmax<kModeWX>(x, x_stride, w, w_stride, m, n, nimg, work, s);
  if (mode == kModeW) launch_absmax<kModeW>(x, x_stride, w, w_stride, m, n, nimg, work, s);
  if (mode == kModeWD2) launch_absmax<kModeWD2>(x, x_stride, w, w_stride, m, n, nimg, work, s);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_fuse_max, dim3(1), dim3(kThreads), 0, s, (const double*)work, blocks_of(n) * (long long)nimg,
                     out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_fuse_accumulate(const double* x, long long x_stride, const double* w, long long w_stride, const double* m,
                         long long n, int nimg, int mode, const double* bmax, int v_total, int64_t* acc,
                         void* stream) {
  if (!bmax) return fail(ADMM_E_INVALID, "bmax is null");
  if (!acc) return fail(ADMM_E_INVALID, "acc is null");
  if (int rc = check_terms(x, x_stride, w, w_stride, m, n, nimg, mode)) return rc;
  if (int rc = check_v_total(v_total)) return rc;
  if (nimg > v_total) return fail(ADMM_E_INVALID, "nimg must be <= v_total");
  hipStream_t s = (hipStream_t)stream;
  long long* a = reinterpret_cast<long long*>(acc);
  if (mode == kModeWX) launch_accumulate<kModeWX>(x, x_stride, w, w_stride, m, n, nimg, bmax, v_total, a, s);
  if (mode == kModeW) launch_accumulate<kModeW>(x, x_stride, w, w_stride, m, n, nimg, bmax, v_total, a, s);
  if (mode == kModeWD2) launch_accumulate<kModeWD2>(x, x_stride, w, w_stride, m, n, nimg, bmax, v_total, a, s);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_fuse_finish(const int64_t* acc_num, const double* bmax_num, const int64_t* acc_den, const double* bmax_den,
                     int v_total, long long n, int root, double* out, void* stream) {
  if (!acc_num || !bmax_num) return fail(ADMM_E_INVALID, "acc_num or bmax_num is null");
  if ((acc_den == nullptr) != (bmax_den == nullptr))
    return fail(ADMM_E_INVALID, "acc_den and bmax_den must both be given or both be null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (int rc = check_v_total(v_total)) return rc;
  if (int rc = check_n(n)) return rc;
  hipLaunchKernelGGL(k_fuse_finish, dim3((unsigned)blocks_of(n)), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const long long*>(acc_num), bmax_num,
                     reinterpret_cast<const long long*>(acc_den), bmax_den, v_total, n, root != 0, out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

int admm_fuse_deviation(const double* x, long long x_stride, const double* mean, long long n, int nimg, double* work,
                        double* out, void* stream) {
  if (!x) return fail(ADMM_E_INVALID, "x is null");
  if (!mean) return fail(ADMM_E_INVALID, "mean is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (int rc = check_shape(n, nimg)) return rc;
  if (x_stride < n) return fail(ADMM_E_INVALID, "x_stride must be >= n");
  hipStream_t s = (hipStream_t)stream;
  const long long P = blocks_of(n);
  hipLaunchKernelGGL(k_fuse_deviation, dim3((unsigned)P, (unsigned)nimg), dim3(kThreads), 0, s, x, x_stride, mean, n,
                     work);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_row_sums<1>, dim3((unsigned)nimg), dim3(kThreads), 0, s, (const double*)work, P, 0, out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

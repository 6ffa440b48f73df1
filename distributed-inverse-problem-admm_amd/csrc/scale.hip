// scale.hip -- the self-scaling Huber threshold: an exact quantile of |ax - b| per image (scope row f13,
// DESIGN.md 6.14).
//
// The Huber threshold of robust.hip in units of the data's own residual scale: delta_v = c * a_k, a_k the
// k-th smallest |residual| of image v (q = 0.5: the lower median, c = scale * 1.4826 the Gaussian
// consistency constant).  include/admm_tomo.h states the definition line by line; every line is one IEEE
// operation (the library is built without contraction), so a NumPy restatement is bitwise.
//
// k_ray_quantile: one block of 1024 threads per image (blockIdx.x), a most-significant-first radix select
// on the bit pattern of |r| -- the sign bit cleared, non-negative IEEE values order as unsigned integers:
// +0 == -0 < denormals < normals < +inf < NaN, the order of np.sort(np.abs(r)).  Each pass streams the
// image's rays (scalar loads of the sample type, coalesced per wave; the rows stay in L2 after the first
// pass), counts the keys that match the prefix found so far into a 2048-bin uint32 LDS histogram with
// integer atomicAdd -- exact in any order --, and the block scans the bins for the one holding the
// remaining rank.  The first pass's bins add up to cnt, the unmasked rays, which fixes the rank.  An
// image's outputs depend on its rays alone.  No floating-point atomic, no scratch, one launch.
#include "common.hpp"

#include <cstdint>
#include <limits>

using namespace admm;

namespace {

using admm_internal::fail;

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kBins = 2048;      // 2 bins per thread in the scan
constexpr int kSelPer = 8;       // rays per thread in flight: one block per image is latency-bound
constexpr long long kMaxRays = 4294967295ll;  // the histogram counts are uint32

template <typename T>
struct Key;
template <>
struct Key<float> {
  using U = uint32_t;
  static constexpr int kPasses = 3;
  static constexpr int kBits = 31;
  __device__ static U of(float r) { return __float_as_uint(r) & 0x7fffffffu; }
  __device__ static double value(U k) { return (double)__uint_as_float(k); }
};
template <>
struct Key<double> {
  using U = uint64_t;
  static constexpr int kPasses = 6;
  static constexpr int kBits = 63;
  __device__ static U of(double r) { return (U)__double_as_longlong(r) & 0x7fffffffffffffffull; }
  __device__ static double value(U k) { return __longlong_as_double((long long)k); }
};

// bits of pass p of P over B key bits, most significant first: the first B % P passes take one more
__host__ __device__ constexpr int pass_bits(int B, int P, int p) { return B / P + (p < B % P ? 1 : 0); }

}  // namespace

namespace admm {

template <typename T>
__global__ __launch_bounds__(kSelThreads) void k_ray_quantile(const T* __restrict__ ax, const T* __restrict__ b,
                                                               const T* __restrict__ w, long long m, double q,
                                                               double c, double floor_, double* __restrict__ out) {
  using K = Key<T>;
  using U = typename K::U;
  __shared__ uint32_t hist[kBins];
  __shared__ uint32_t wave_tot[kSelWaves];
  __shared__ uint32_t sel[2];  // the chosen bin, the rank inside it
  const size_t v = blockIdx.x;
  const size_t row = v * (size_t)m;
  const int t = threadIdx.x;
  U prefix = 0;          // the key bits fixed so far, right-aligned
  uint32_t rank = 0;     // the rank among the keys that match the prefix
  uint32_t cnt = 0;
  int hi = K::kBits;     // key bits [hi, kBits) are fixed
#pragma unroll
  for (int pass = 0; pass < K::kPasses; ++pass) {
    const int bits = pass_bits(K::kBits, K::kPasses, pass);
    const int lo = hi - bits;
    const uint32_t mask = (1u << bits) - 1u;
    hist[2 * t] = 0;
    hist[2 * t + 1] = 0;
    __syncthreads();
    for (long long base = 0; base < m; base += (long long)kSelThreads * kSelPer) {
      // every load of the sweep is issued before the first use: a ray past the end reads the row's last
      // ray (in bounds) and is dropped afterwards, so no load waits behind a branch
      T va[kSelPer], vb[kSelPer], vw[kSelPer];
#pragma unroll
      for (int u = 0; u < kSelPer; ++u) {
        const long long p = base + (long long)u * kSelThreads + t;
        const size_t i = row + (size_t)(p < m ? p : m - 1);
        va[u] = ax[i];
        vb[u] = b[i];
        vw[u] = w ? w[i] : (T)1;
      }
      U key[kSelPer];
      bool live[kSelPer];
#pragma unroll
      for (int u = 0; u < kSelPer; ++u) {
        const long long p = base + (long long)u * kSelThreads + t;
        const T r = va[u] - vb[u];
        key[u] = K::of(r);
        live[u] = p < m && vw[u] != (T)0;
      }
#pragma unroll
      for (int u = 0; u < kSelPer; ++u) {
        // (hi == kBits: the shift leaves the cleared sign bit, 0 == prefix)
        if (live[u] && (key[u] >> hi) == prefix) atomicAdd(&hist[(uint32_t)(key[u] >> lo) & mask], 1u);
      }
    }
    __syncthreads();
    // the bin holding `rank`: thread t owns bins 2t and 2t + 1; an inclusive scan of the pair sums inside
    // each wave, then the waves before this one added
    const uint32_t c0 = hist[2 * t], c1 = hist[2 * t + 1];
    const uint32_t s = c0 + c1;
    uint32_t incl = s;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = __shfl_up(incl, off, 64);
      if ((t & 63) >= off) incl += up;
    }
    if ((t & 63) == 63) wave_tot[t >> 6] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int wv = 0; wv < kSelWaves; ++wv) {
      const uint32_t wt = wave_tot[wv];
      if (wv < (t >> 6)) before += wt;
      total += wt;
    }
    if (pass == 0) {
      cnt = total;
      if (cnt == 0) {  // (uniform over the block)
        if (t == 0) {
          out[v * 3 + 0] = std::numeric_limits<double>::infinity();
          out[v * 3 + 1] = 0.0;
          out[v * 3 + 2] = 0.0;
        }
        return;
      }
      const double kf = floor(q * (double)(cnt - 1u));
      rank = (uint32_t)(long long)kf;
    }
    const uint32_t excl = before + incl - s;
    if (rank >= excl && rank - excl < s) {  // exactly one thread: rank < total
      const uint32_t rel = rank - excl;
      sel[0] = rel < c0 ? 2 * t : 2 * t + 1;
      sel[1] = rel < c0 ? rel : rel - c0;
    }
    __syncthreads();
    prefix = (prefix << bits) | (U)sel[0];
    rank = sel[1];
    hi = lo;
    // (the next pass's zeroing of hist and its barrier come before sel is written again)
  }
  if (t == 0) {
    double ak = K::value(prefix);
    if (ak != ak) ak = std::numeric_limits<double>::quiet_NaN();
    const double th = c * ak;
    double delta = std::numeric_limits<double>::infinity();
    if (th > 0.0 && th < std::numeric_limits<double>::infinity()) delta = th >= floor_ ? th : floor_;
    out[v * 3 + 0] = delta;
    out[v * 3 + 1] = ak;
    out[v * 3 + 2] = (double)cnt;
  }
}

}  // namespace admm

extern "C" {

int admm_ray_quantile_work(long long m, int nimg, long long* n_bytes) {
  if (!n_bytes) return fail(ADMM_E_INVALID, "n_bytes is null");
  if (m < 1 || m > kMaxRays) return fail(ADMM_E_INVALID, "m must be in [1, 2^32 - 1]");
  if (nimg < 1 || nimg > kMaxGridY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  *n_bytes = 0;
  return ADMM_OK;
}

int admm_ray_quantile(const void* ax, const void* b, const void* w, int dtype, long long m, int nimg, double q,
                      double c, double floor, void* work, double* out, void* stream) {
  (void)work;
  if (!ax) return fail(ADMM_E_INVALID, "ax is null");
  if (!b) return fail(ADMM_E_INVALID, "b is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (dtype != ADMM_DTYPE_F32 && dtype != ADMM_DTYPE_F64)
    return fail(ADMM_E_INVALID, "dtype must be ADMM_DTYPE_F32 or ADMM_DTYPE_F64");
  if (!(q >= 0.0 && q <= 1.0)) return fail(ADMM_E_INVALID, "q must be in [0, 1]");
  if (!(c > 0.0)) return fail(ADMM_E_INVALID, "c must be > 0, not NaN");
  if (!(floor >= 0.0)) return fail(ADMM_E_INVALID, "floor must be >= 0 (+inf allowed), not NaN");
  if (m < 1 || m > kMaxRays) return fail(ADMM_E_INVALID, "m must be in [1, 2^32 - 1]");
  if (nimg < 1 || nimg > kMaxGridY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nimg);
  if (dtype == ADMM_DTYPE_F64)
    hipLaunchKernelGGL(k_ray_quantile<double>, grid, dim3(kSelThreads), 0, s, (const double*)ax, (const double*)b,
                       (const double*)w, m, q, c, floor, out);
  else
    hipLaunchKernelGGL(k_ray_quantile<float>, grid, dim3(kSelThreads), 0, s, (const float*)ax, (const float*)b,
                       (const float*)w, m, q, c, floor, out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

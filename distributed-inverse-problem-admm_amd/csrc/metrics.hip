// metrics.hip -- per-image squared error and SSIM sum against one reference image
// (evaluation path, DESIGN.md 6.7, scope row f6).
//
// The reference scores a run by PSNR (test_final_integration.py:41-50: mse = mean((x_hat - x_true)^2),
// 20 log10(data_range) - 10 log10(mse), data_range = x_true.max() - x_true.min(), mean over nodes).
// This file supplies the two image-domain sums that PSNR and SSIM (Wang, Bovik, Sheikh, Simoncelli
// 2004) are formed from, for a batch of float64 images that is already in HBM:
//
//   out[v][0] = sum_p (img_v[p] - ref[p])^2                                  over mask[p] != 0
//   out[v][1] = sum_c S_v(c),  c = (i, j), 5 <= i, j <= N - 6,               over mask[c] != 0
//   S = (2 mx my + c1)(2 sxy + c2) / ((mx^2 + my^2 + c1)(sx^2 + sy^2 + c2))
//
// with the moments mx, my, E[x^2], E[y^2], E[xy] taken under the 11 x 11 Gaussian window
// (sigma = 1.5, the 1-D taps normalised to sum 1, the window their outer product) and the
// population (co)variances E[.] - mu mu: the valid region only, no boundary extension.
//
// k_image_metrics: one block per 16 x 32 image tile and image.  The tile plus its 5-pixel halo of
// img_v and ref is staged once in LDS as float64; a horizontal pass forms the five row moments of
// every in-image halo row at the tile's valid centre columns, a vertical pass the window moments
// and S at the valid centres; the block's two sums (block_sums<2>) go to its own slots of `work`,
// work[(v * 2 + q) * tiles + tile].  k_row_sums<2>: one block per image adds the slots in a fixed
// order (both: common.hpp).  No atomics anywhere: every sum is a fixed fma / add chain, so an image's
// outputs depend on its pixels alone.
#include <cmath>
#include <cstdint>

#include "common.hpp"

using namespace admm;  // kThreads = 256, block_sums, k_row_sums

namespace {

using admm_internal::fail;

constexpr int kMinN = 11, kMaxN = 4096;  // one window .. the library's N limit
constexpr int kSums = 2;                 // squared error, SSIM sum
constexpr int kRad = 5, kWin = 2 * kRad + 1;
constexpr int kTH = 16, kTW = 32;                        // tile: rows x columns
constexpr int kHH = kTH + 2 * kRad, kHW = kTW + 2 * kRad;  // tile + halo: 26 x 42
constexpr int kFields = 5;  // x, y, x^2, y^2, xy
constexpr int kCG = 4;      // horizontal pass: consecutive columns per thread (one row)
constexpr int kRG = 2;      // vertical pass: consecutive rows per thread (one column): all 256 threads
constexpr int kSS = kHW + 1;  // staged row stride 43: lanes along the rows read conflict-free (43 odd)
constexpr int kMS = kTW + 1;  // row-moment row stride 33, likewise for the horizontal pass's writes
static_assert(kHH * (kTW / kCG) <= kThreads && kTW * (kTH / kRG) <= kThreads, "one work item per thread");

struct Taps {
  double w[kWin];
};

// LDS: sx, sy 2 x 26 x 43 x 8 = 17 888 B, hm 5 x 26 x 33 x 8 = 34 320 B, red 64 B: 52 272 B, three
// blocks per CU (156 816 of the CU's 163 840 B).  Both passes slide a register window so that every
// LDS value is loaded once per kCG (kRG) outputs: a horizontal-pass thread owns kCG consecutive columns of one row -- its lanes
// run along the rows, conflict-free through the odd row strides 43 and 33 -- and a vertical-pass
// thread kRG consecutive rows of one column, lanes along the columns.  Each output's sum is the
// same ascending-k fma chain whichever thread forms it.
__global__ __launch_bounds__(kThreads) void k_image_metrics(const double* __restrict__ img, long long img_stride,
                                                            const double* __restrict__ ref,
                                                            const uint8_t* __restrict__ mask, int N, Taps g, double c1,
                                                            double c2, double* __restrict__ work) {
  __shared__ double sx[kHH][kSS];
  __shared__ double sy[kHH][kSS];
  __shared__ double hm[kFields][kHH][kMS];
  __shared__ double red[kSums][kThreads / 64];
  const int tid = threadIdx.x;
  const int i0 = (int)blockIdx.y * kTH, j0 = (int)blockIdx.x * kTW;  // the tile's first pixel
  const double* x = img + (size_t)blockIdx.z * (size_t)img_stride;

  // stage: off-image slots hold 0 and are never read into a sum (the guards below).  Every global
  // load of the thread is issued before its first LDS store: one memory latency per block, not one
  // per pass of the loop.
  constexpr int kStage = (kHH * kHW + kThreads - 1) / kThreads;
  double tx[kStage], ty[kStage];
#pragma unroll
  for (int q = 0; q < kStage; ++q) {
    const int s = tid + q * kThreads;
    const int r = s / kHW, c = s - r * kHW;
    const int gi = i0 - kRad + r, gj = j0 - kRad + c;
    const bool in = s < kHH * kHW && gi >= 0 && gi < N && gj >= 0 && gj < N;
    const size_t p = in ? (size_t)gi * (size_t)N + (size_t)gj : 0;
    tx[q] = in ? x[p] : 0.0;
    ty[q] = in ? ref[p] : 0.0;
  }
  // the vertical pass's pixels (tile rows vr0 .. vr0 + kRG - 1 of column vc): their mask bytes travel
  // with the loads above
  const bool vthread = tid < kTW * (kTH / kRG);
  const int vc = tid % kTW, vr0 = (tid / kTW) * kRG;
  bool on[kRG];
#pragma unroll
  for (int q = 0; q < kRG; ++q) {
    const int gi = i0 + vr0 + q, gj = j0 + vc;
    on[q] = vthread && gi < N && gj < N;
    if (on[q] && mask) on[q] = mask[(size_t)gi * (size_t)N + (size_t)gj] != 0;
  }
#pragma unroll
  for (int q = 0; q < kStage; ++q) {
    const int s = tid + q * kThreads;
    const int r = s / kHW, c = s - r * kHW;
    if (s < kHH * kHW) {
      sx[r][c] = tx[q];
      sy[r][c] = ty[q];
    }
  }
  __syncthreads();

  // horizontal pass: row moments of halo row r at tile columns c0 .. c0 + kCG - 1 (column c's window
  // is staged columns c .. c + 10).  Summed for in-image rows and valid centre columns only; the
  // other entries of hm are set to 0 and belong to no valid centre's window.
  if (tid < kHH * (kTW / kCG)) {
    const int r = tid % kHH, c0 = (tid / kHH) * kCG;
    const int gi = i0 - kRad + r;
    const bool row_in = gi >= 0 && gi < N;
    double xv[kWin + kCG - 1], yv[kWin + kCG - 1];
#pragma unroll
    for (int e = 0; e < kWin + kCG - 1; ++e) {
      xv[e] = sx[r][c0 + e];
      yv[e] = sy[r][c0 + e];
    }
#pragma unroll
    for (int q = 0; q < kCG; ++q) {
      const int gj = j0 + c0 + q;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
      if (row_in && gj >= kRad && gj <= N - 1 - kRad) {
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
          const double w = g.w[k], xe = xv[q + k], ye = yv[q + k];
          a0 = fma(w, xe, a0);
          a1 = fma(w, ye, a1);
          a2 = fma(w, xe * xe, a2);
          a3 = fma(w, ye * ye, a3);
          a4 = fma(w, xe * ye, a4);
        }
      }
      hm[0][r][c0 + q] = a0;
      hm[1][r][c0 + q] = a1;
      hm[2][r][c0 + q] = a2;
      hm[3][r][c0 + q] = a3;
      hm[4][r][c0 + q] = a4;
    }
  }
  __syncthreads();

  // vertical pass + S at the tile's pixels; the squared error of the same pixels
  // (tile rows r0 .. r0 + kRG - 1 of column c; row r's window is hm rows r .. r + 10)
  double acc[kSums] = {0.0, 0.0};  // squared error, SSIM sum
  double &sse = acc[0], &ssum = acc[1];
  if (vthread) {
    const int c = vc, r0 = vr0;
    const int gj = j0 + c;
    bool valid[kRG];
    bool any = false;
#pragma unroll
    for (int q = 0; q < kRG; ++q) {
      const int gi = i0 + r0 + q;
      valid[q] = on[q] && gi >= kRad && gi <= N - 1 - kRad && gj >= kRad && gj <= N - 1 - kRad;
      any = any || valid[q];
      if (on[q]) {  // masked-out and off-image pixels contribute exactly 0
        const double d = sx[r0 + q + kRad][c + kRad] - sy[r0 + q + kRad][c + kRad];
        sse = fma(d, d, sse);
      }
    }
    if (any) {
      double m[kRG][kFields];
#pragma unroll
      for (int f = 0; f < kFields; ++f) {
        double col[kWin + kRG - 1];
#pragma unroll
        for (int e = 0; e < kWin + kRG - 1; ++e) col[e] = hm[f][r0 + e][c];
#pragma unroll
        for (int q = 0; q < kRG; ++q) {
          double a = 0.0;
          if (valid[q]) {  // an excluded centre's window is never summed
#pragma unroll
            for (int k = 0; k < kWin; ++k) a = fma(g.w[k], col[q + k], a);
          }
          m[q][f] = a;
        }
      }
#pragma unroll
      for (int q = 0; q < kRG; ++q) {
        const double mx = m[q][0], my = m[q][1];
        const double vx = fma(-mx, mx, m[q][2]), vy = fma(-my, my, m[q][3]), vxy = fma(-mx, my, m[q][4]);
        const double num = fma(2.0 * mx, my, c1) * fma(2.0, vxy, c2);
        const double den = fma(mx, mx, fma(my, my, c1)) * ((vx + vy) + c2);
        if (valid[q]) ssum += num / den;
      }
    }
  }
  block_sums(acc, red);
  if (tid == 0) {
    const size_t tiles = (size_t)gridDim.x * (size_t)gridDim.y;
    const size_t tile = (size_t)blockIdx.y * (size_t)gridDim.x + (size_t)blockIdx.x;
#pragma unroll
    for (int q = 0; q < kSums; ++q) work[((size_t)blockIdx.z * kSums + q) * tiles + tile] = acc[q];
  }
}

inline int tiles_x(int N) { return (N + kTW - 1) / kTW; }
inline int tiles_y(int N) { return (N + kTH - 1) / kTH; }

int check_shape(int N, int nimg) {
  if (N < kMinN || N > kMaxN) return fail(ADMM_E_INVALID, "N must be in [11, 4096] (one 11 x 11 window .. the library's limit)");
  if (nimg < 1 || nimg > kMaxGridY) return fail(ADMM_E_INVALID, "nimg must be in [1, 65535]");
  return ADMM_OK;
}

}  // namespace

extern "C" {

int admm_image_metrics_work(int N, int nimg, long long* n_doubles) {
  if (!n_doubles) return fail(ADMM_E_INVALID, "n_doubles is null");
  if (int rc = check_shape(N, nimg)) return rc;
  *n_doubles = (long long)kSums * (long long)tiles_x(N) * (long long)tiles_y(N) * (long long)nimg;
  return ADMM_OK;
}

int admm_image_metrics(const double* img, long long img_stride, const double* ref, const uint8_t* mask, int N, int nimg,
                       double c1, double c2, double* work, double* out, void* stream) {
  if (!img) return fail(ADMM_E_INVALID, "img is null");
  if (!ref) return fail(ADMM_E_INVALID, "ref is null");
  if (!work) return fail(ADMM_E_INVALID, "work is null");
  if (!out) return fail(ADMM_E_INVALID, "out is null");
  if (int rc = check_shape(N, nimg)) return rc;
  if (img_stride < (long long)N * (long long)N) return fail(ADMM_E_INVALID, "img_stride must be >= N * N");
  if (!(c1 > 0.0) || !(c2 > 0.0) || !std::isfinite(c1) || !std::isfinite(c2))
    return fail(ADMM_E_INVALID, "c1 and c2 must be finite and > 0");
  Taps g;
  double sum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    const double d = (double)(k - kRad);
    g.w[k] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += g.w[k];
  }
  for (int k = 0; k < kWin; ++k) g.w[k] /= sum;
  hipStream_t s = (hipStream_t)stream;
  const int tx = tiles_x(N), ty = tiles_y(N);
  hipLaunchKernelGGL(k_image_metrics, dim3((unsigned)tx, (unsigned)ty, (unsigned)nimg), dim3(kThreads), 0, s, img,
                     img_stride, ref, mask, N, g, c1, c2, work);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_row_sums<kSums>, dim3((unsigned)nimg), dim3(kThreads), 0, s, (const double*)work,
                     (long long)tx * ty, 0, out);
  HIP_TRY(hipGetLastError());
  return ADMM_OK;
}

}  // extern "C"

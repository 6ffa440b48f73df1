// tables.hpp -- the table records host and device share (plain C++17: no HIP header, so the
// planner that fills them, fwd_plan.hpp, builds and runs on a machine without a GPU).
// kernels.hpp includes this file; admm_tomo.hip uploads the tables.
#pragma once
#include <cstddef>

namespace admm {

constexpr int kXcds = 8;  // MI355X: 8 XCDs, workgroups dealt round-robin (id % 8)

// Per-angle forward-projector constants (host-computed in float64).
// Ray (t,k), step m:  l = A0 + k*A1 + m*dl  (interpolation coordinate).
struct FwdAngle {
  double A0, A1, dl;
  double L;   // path length per step h/|alpha|
  int caseA;  // 1: step over axis-1 index on the transposed image
  int pad;
};
// Per-angle back-projector constants: fractional bin k_f = B0 + i*Bi + j*Bj,
// weight(k) = max(0, 1 - |k-k_f|*slope) * L.
struct BackAngle {
  double B0, Bi, Bj;
  double slope, L;
};

// Compact per-angle record of the back projector's hot loop (one s_load_dwordx8):
// k_f = (i - c0) Bi + (j - c0) Bj + K with K = -det_min/hd - 1/2 the same for every
// angle; float32 weights w0 = max(0, L - f sL), w1 = max(0, (L - sL) + f sL), formed
// as one packed fma (f, f) * ws + wc with ws = (-sL, sL), wc = (L, L - sL).
#if defined(__clang__)
typedef float float2v __attribute__((ext_vector_type(2)));  // (the taps' inline assembly takes these)
#else
struct alignas(8) float2v {  // the same 8 bytes for a host compiler without vector extensions
  float x, y;
};
#endif
struct alignas(32) BackAngleC {
  double Bi, Bj;
  float2v ws, wc;
};

#ifndef ADMM_FG_SEG
#define ADMM_FG_SEG 8
#endif
#ifndef ADMM_FG_G
#define ADMM_FG_G 16
#endif
#ifndef ADMM_FG_WIN
#define ADMM_FG_WIN 256
#endif
constexpr int kFgG = ADMM_FG_G;      // max angles (waves) per block
constexpr int kFgWin = ADMM_FG_WIN;  // staged window width (pixels)
constexpr int kFgSeg = ADMM_FG_SEG;  // row segments (partial sums) per ray

// One angle group of the grouped forward projector: angles t0 .. t0+G-1 (one case).
struct FgGroup {
  int t0, G;
};
// The rays one block projects: angle t0+q of its group takes rays k0[q] .. k0[q]+nk[q]-1
// (0 <= nk <= 64, inside [0, n_det)).  Every plan is a table of these (one per (group,
// segment, chunk)); per (group, segment) the ranges of each angle partition its rays (less
// any ray a clipped plan drops because it misses the segment inside the image).  The
// 64-ray plans give angle q rays x*64 + delta_q + [0, 64), delta_q = 0 or the shift that
// makes every angle of the group cross the same pixels at the segment's centre row; the
// chunk-aligned plan starts every angle's chunk x at the same pixel of that row (a chunk
// spans 64 rays of the group's densest angle, so sparser angles use fewer lanes), which
// keeps the union window narrow far from the detector centre too.
struct FgRange {
  int k0[kFgG];
  int nk[kFgG];
};

// One entry of the grouped forward projector's block table, read by k_fwdg as an int4.
// Plan entries: {ray-range index, group, segment, G}; launch-table entries: {ray-range index,
// group, segment + kFgSeg * node chunk, 0}.
struct alignas(16) FgBlock {
  int x, y, z, w;
};

static_assert(sizeof(FwdAngle) == 40 && alignof(FwdAngle) == 8 && offsetof(FwdAngle, L) == 24 &&
                  offsetof(FwdAngle, caseA) == 32,
              "FwdAngle layout");
static_assert(sizeof(BackAngle) == 40 && alignof(BackAngle) == 8 && offsetof(BackAngle, slope) == 24, "BackAngle layout");
static_assert(sizeof(float2v) == 8 && alignof(float2v) == 8, "float2v: an 8-byte, 8-aligned float pair");
static_assert(sizeof(BackAngleC) == 32 && alignof(BackAngleC) == 32 && offsetof(BackAngleC, Bj) == 8 &&
                  offsetof(BackAngleC, ws) == 16 && offsetof(BackAngleC, wc) == 24,
              "BackAngleC layout (one 32-byte scalar load)");
static_assert(sizeof(FgGroup) == 8 && alignof(FgGroup) == 4, "FgGroup layout");
static_assert(sizeof(FgRange) == 8 * kFgG && alignof(FgRange) == 4 && offsetof(FgRange, nk) == 4 * kFgG, "FgRange layout");
static_assert(sizeof(FgBlock) == 16 && alignof(FgBlock) == 16 && offsetof(FgBlock, w) == 12, "FgBlock layout");

}  // namespace admm

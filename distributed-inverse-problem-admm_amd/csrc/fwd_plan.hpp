// fwd_plan.hpp -- host planner of the projectors (plain C++17, no HIP: it runs and is tested on
// a machine without a GPU, tests/host/plan_dump.cpp).  From an admm_geom it makes the angle
// records (geom_tables), the six angle-group plans of the grouped forward projector
// (build_fwd_plans), a plan's block table in launch order (fwd_block_order) and the choice of
// the plan a batch binds (choose_fwd_plan_index).  admm_tomo.hip uploads the results; every
// device and environment query stays there and arrives here as an argument.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/admm_tomo.h"
#include "tables.hpp"

namespace admm {

// The argument checks of admm_ctx_create, in its order: the message of the first one that
// fails (ADMM_E_INVALID), or null.
inline const char* check_geom(const admm_geom& g, int dtype, int max_images) {
  if (g.N < 2 || g.n_angles < 1 || g.n_det < 1) return "bad geometry sizes";
  if (g.N > 4096) return "N > 4096 is not supported";
  if (dtype != ADMM_DTYPE_F32 && dtype != ADMM_DTYPE_F64) return "bad dtype";
  if (max_images < 1) return "max_images < 1";
  const double h = 2.0 / g.N;
  const double hd = (g.det_max - g.det_min) / g.n_det;
  if (!(hd > 0)) return "det_max <= det_min";
  if (hd < h * (1.0 - 1e-9))
    return "detector spacing finer than the pixel size is not supported "
           "(det_width_factor must be >= 1 with n_det = N)";
  const size_t npix = (size_t)g.N * g.N, m = (size_t)g.n_angles * g.n_det;
  if ((size_t)max_images * npix * 8 >= (1ull << 31) || (size_t)max_images * m * 8 >= (1ull << 31))
    return "batch too large for 32-bit buffer offsets; split it across contexts";
  return nullptr;
}

// geometry tables, float64 (oracle/geometry.py)
struct GeomTables {
  std::vector<FwdAngle> fa;
  std::vector<BackAngle> ba;
  std::vector<BackAngleC> bc;
  double Kb = 0.0;  // angle-independent part of the back projector's k_f
  int kbias = 0;    // integer bias making every pixel's k_f positive (k_back)
  int wexp = 0;     // k_back float weights scaled by 2^-wexp (<= 1 for the fma clamp)
};

// The tables of a geometry that passed check_geom; null, or the message of ADMM_E_INVALID.
inline const char* geom_tables(const admm_geom& g, int dtype, GeomTables& T) {
  T = GeomTables{};
  const double h = 2.0 / g.N;
  const double hd = (g.det_max - g.det_min) / g.n_det;
  std::vector<FwdAngle>& fa = T.fa;
  std::vector<BackAngle>& ba = T.ba;
  std::vector<BackAngleC>& bc = T.bc;
  fa.resize(g.n_angles);
  ba.resize(g.n_angles);
  bc.resize(g.n_angles);
  T.Kb = -g.det_min / hd - 0.5;
  const double c0 = 0.5 * (g.N - 1);
  for (int t = 0; t < g.n_angles; ++t) {
    const double th = g.angle_min + (t + 0.5) * (g.angle_max - g.angle_min) / g.n_angles;
    const double cs = std::cos(th), sn = std::sin(th);
    const bool caseA = std::fabs(cs) >= std::fabs(sn);
    const double al = caseA ? cs : sn, be = caseA ? sn : cs;
    fa[t].A0 = c0 + (g.det_min / h + 0.5 * hd / h + c0 * be) / al;
    fa[t].A1 = (hd / h) / al;
    fa[t].dl = -be / al;
    fa[t].L = h / std::fabs(al);
    fa[t].caseA = caseA ? 1 : 0;
    ba[t].Bi = cs * h / hd;
    ba[t].Bj = sn * h / hd;
    ba[t].B0 = -c0 * (ba[t].Bi + ba[t].Bj) - g.det_min / hd - 0.5;
    ba[t].slope = (hd / h) / std::fabs(al);
    ba[t].L = h / std::fabs(al);
    bc[t].Bi = ba[t].Bi;
    bc[t].Bj = ba[t].Bj;
    const float sLf = (float)(ba[t].slope * ba[t].L);
    bc[t].ws = float2v{-sLf, sLf};
    bc[t].wc = float2v{(float)ba[t].L, (float)(ba[t].L - ba[t].slope * ba[t].L)};
    while (std::ldexp((double)bc[t].wc.x, -T.wexp) > 1.0) ++T.wexp;
    // smallest k_f of any pixel at this angle: Kb - c0 (|Bi| + |Bj|)
    const double kmn = T.Kb - c0 * (std::fabs(ba[t].Bi) + std::fabs(ba[t].Bj));
    T.kbias = std::max(T.kbias, (int)std::ceil(-kmn) + 2);
  }
  // the float taps' kf_split needs k_f + kbias in (0, 2^20) for every pixel and angle (the sum
  // with 2^20 must stay in [2^20, 2^21)); a detector far off the image could break that
  for (int t = 0; t < g.n_angles && dtype == ADMM_DTYPE_F32; ++t) {
    const double kmx = T.Kb + T.kbias + c0 * (std::fabs(ba[t].Bi) + std::fabs(ba[t].Bj)) + 2.0;
    if (kmx >= 1048576.0) return "detector offset puts a bin position past 2^20 (kf_split)";
  }
  // exact power-of-two scalings: 2^-wexp (N < 3: L = 2 / (N |cos|) can exceed 1) on ws and wc, and
  // 2^-32 on ws, whose float taps multiply frac(k_f) x 2^32 (kernels.hpp kf_split)
  for (int t = 0; t < g.n_angles; ++t) {
    bc[t].ws = float2v{std::ldexp(bc[t].ws.x, -T.wexp - 32), std::ldexp(bc[t].ws.y, -T.wexp - 32)};
    bc[t].wc = float2v{std::ldexp(bc[t].wc.x, -T.wexp), std::ldexp(bc[t].wc.y, -T.wexp)};
  }
  return nullptr;
}

// The group plans, chosen at bind time: 0: 64-ray chunks, 1: chunks aligned per (row segment,
// angle) at the detector centre, 2: chunks aligned per (row segment, chunk); 3-5: the same with
// every block's rays clipped to those crossing its segment inside the image (groups re-planned
// on the narrower windows)
constexpr int kFwdPlans = 6;

struct FwdPlan {
  std::vector<FgGroup> groups;  // empty: the geometry does not have this plan
  std::vector<FgRange> ranges;  // per block: its rays
  std::vector<FgBlock> blocks;  // per block: {ray-range index, group, segment, G}
  std::vector<char> caseA;      // per group: its angles read the transposed image
  double staged = 0.0;          // touched row pixels staged per node chunk (host model)
};
struct FwdPlans {
  FwdPlan plan[kFwdPlans];
  bool fits = true;  // false: no grouped kernel for this geometry (plans 0-1 are mandatory, 2-5 optional)
};

// angle groups for the grouped forward projector: consecutive angles of one case,
// G <= kFgG, whose union row window of every block fits kFgWin (float64, same formulas as
// the device; 2 pixels of margin).  Three plans, each a table of per-block ray ranges
// (FgRange): plain 64-ray chunks; 64-ray chunks aligned per (row segment, angle) at the
// detector centre (FgGroup.delta: narrower windows and larger groups, one more chunk per
// segment); chunks aligned per (row segment, chunk) -- every angle's chunk x starts at the
// same pixel of the segment's centre row, so windows stay narrow far from the detector
// centre, where the rays' spacing 1/|cos| differs between the group's angles.
// admm_batch_bind picks one (choose_fwd_plan_index).
inline FwdPlans build_fwd_plans(const admm_geom& g, const std::vector<FwdAngle>& fa) {
  FwdPlans P;
  const double cd = 0.5 * (g.n_det - 1);
  // touched row pixels of one block over its segment's rows, -1 if a row is too wide
  auto window_px = [&](int t0, int G, int mlo, int mhi, const FgRange& r) -> long {
    long px = 0;
    for (int m = mlo; m < mhi; ++m) {
      double lo = 1e300, hi = -1e300;
      for (int q = 0; q < G; ++q) {
        if (r.nk[q] == 0) continue;
        const FwdAngle& b = fa[t0 + q];
        for (int kk : {r.k0[q], r.k0[q] + r.nk[q] - 1}) {
          const double l = std::fma((double)m, b.dl, std::fma((double)kk, b.A1, b.A0));
          lo = std::min(lo, l);
          hi = std::max(hi, l);
        }
      }
      if (lo > hi) continue;
      const double w = std::floor(hi) - std::floor(lo) + 2;
      if (w > kFgWin - 2) return -1;
      px += (long)w;
    }
    return px;
  };
  // the blocks of group (t0, G) under plan pl: ray ranges rv, block entries bv
  // ({range index within rv, group index gi, segment, G}), staged pixels st
  auto plan_group = [&](int t0, int G, int pl, int gi, FgGroup& gr, std::vector<FgRange>& rv,
                        std::vector<FgBlock>& bv, double& st) -> bool {
    for (int q = 0; q < G; ++q)
      if (fa[t0 + q].caseA != fa[t0].caseA) return false;
    const int scheme = pl % 3;
    const bool clipped = pl >= 3;
    gr = FgGroup{};
    gr.t0 = t0;
    gr.G = G;
    rv.clear();
    bv.clear();
    st = 0.0;
    for (int s = 0; s < kFgSeg; ++s) {
      const int mlo = s * g.N / kFgSeg, mhi = (s + 1) * g.N / kFgSeg;
      const double mc = 0.5 * (mlo + mhi - 1);
      // only rays that cross the segment's rows inside the image get lanes: a ray whose every
      // row position l lies outside [-2, N + 1] taps zero-filled columns only, so its partial
      // for this segment is exactly 0 and its slot keeps the zero it was filled with
      // (admm_batch_bind / op_forward_chunk zero the partials when the plan changes)
      const double dlo = std::min(mlo * 1.0, mhi - 1.0), dhi = std::max(mlo * 1.0, mhi - 1.0);
      auto clip = [&](FgRange& r) {
        for (int q = 0; q < G; ++q) {
          const FwdAngle& b = fa[t0 + q];
          const double e0 = std::min(dlo * b.dl, dhi * b.dl), e1 = std::max(dlo * b.dl, dhi * b.dl);
          const double ka = (-2.0 - b.A0 - e1) / b.A1, kb = (g.N + 1.0 - b.A0 - e0) / b.A1;
          const double klo = std::ceil(std::min(ka, kb)), khi = std::floor(std::max(ka, kb));
          const int lo = (int)std::max((double)r.k0[q], klo);
          const int hi = (int)std::min((double)(r.k0[q] + r.nk[q]), khi + 1.0);
          r.nk[q] = std::max(0, hi - lo);
          r.k0[q] = std::min(std::max(lo, 0), g.n_det - 1);
        }
      };
      auto emit = [&](FgRange r) -> bool {
        if (clipped) clip(r);
        bool any = false;
        for (int q = 0; q < G; ++q) any = any || r.nk[q] > 0;
        if (!any) return true;
        const long px = window_px(t0, G, mlo, mhi, r);
        if (px < 0) return false;
        st += (double)px;
        bv.push_back(FgBlock{(int)rv.size(), gi, s, G});
        rv.push_back(r);
        return true;
      };
      if (scheme < 2) {
        const FwdAngle& r0 = fa[t0];
        const double lref = r0.A0 + cd * r0.A1 + mc * r0.dl;  // reference ray at the centre row
        int delta[kFgG] = {};  // per-angle ray offset of the 64-ray chunks (scheme 1)
        int dmin = 0, dmax = 0;
        for (int q = 0; q < G; ++q) {
          const FwdAngle& b = fa[t0 + q];
          const int d = scheme == 1 ? (int)std::lround((lref - b.A0 - cd * b.A1 - mc * b.dl) / b.A1) : 0;
          delta[q] = d;
          dmin = std::min(dmin, d);
          dmax = std::max(dmax, d);
        }
        const int kcb = (int)std::floor(-dmax / 64.0);
        const int kce = (int)std::ceil((g.n_det - dmin) / 64.0);
        for (int kc = kcb; kc < kce; ++kc) {
          FgRange r{};
          for (int q = 0; q < G; ++q) {
            const int lo = std::max(kc * 64 + delta[q], 0);
            const int hi = std::min(kc * 64 + delta[q] + 64, g.n_det);
            r.k0[q] = lo;
            r.nk[q] = std::max(0, hi - lo);
          }
          if (!emit(r)) return false;
        }
      } else {
        // position of ray k at the centre row, along the direction of increasing k:
        // u_q(k) = sgn (A0 + mc dl) + k |A1|; chunk x holds the rays with u in
        // [U0 + x S, U0 + (x + 1) S), S = 64 min|A1| (<= 64 rays of every angle)
        const double sgn = fa[t0].A1 > 0 ? 1.0 : -1.0;
        double amin = 1e300, U0 = 1e300;
        double cq[kFgG], aq[kFgG];
        for (int q = 0; q < G; ++q) {
          const FwdAngle& b = fa[t0 + q];
          if ((b.A1 > 0) != (sgn > 0)) return false;
          aq[q] = std::fabs(b.A1);
          cq[q] = sgn * (b.A0 + mc * b.dl);
          amin = std::min(amin, aq[q]);
          U0 = std::min(U0, cq[q]);
        }
        const double S = 64.0 * amin * (1.0 - 1e-9);
        auto bnd = [&](int q, long x) {
          const double v = std::ceil((U0 + (double)x * S - cq[q]) / aq[q]);
          return (int)std::min(std::max(v, 0.0), (double)g.n_det);
        };
        for (long x = 0;; ++x) {
          if (x > 4L * g.n_det + 8) return false;  // (cannot happen: every chunk spans >= 64 pixels)
          FgRange r{};
          bool done = true;
          for (int q = 0; q < G; ++q) {
            const int lo = bnd(q, x), hi = bnd(q, x + 1);
            done = done && lo >= g.n_det;
            r.k0[q] = std::min(lo, g.n_det - 1);
            r.nk[q] = hi - lo;
            if (r.nk[q] > 64) return false;
          }
          if (done) break;
          if (!emit(r)) return false;
        }
      }
    }
    return true;
  };
  // greedy: the largest G <= kFgG consecutive same-case angles whose windows fit.
  // (Balanced splits of each same-case run were measured slower: they force wide windows
  // near 45 degrees, where greedy makes small narrow groups and stages fewer pixels.)
  for (int pl = 0; pl < kFwdPlans && P.fits; ++pl) {
    FwdPlan& Q = P.plan[pl];
    for (int t0 = 0; t0 < g.n_angles;) {
      int G = std::min(kFgG, g.n_angles - t0);
      const int gi = (int)Q.groups.size();
      FgGroup gr{};
      std::vector<FgRange> rv;
      std::vector<FgBlock> bv;
      double st = 0.0;
      while (G > 1 && !plan_group(t0, G, pl, gi, gr, rv, bv, st)) --G;
      if (G == 1 && !plan_group(t0, 1, pl, gi, gr, rv, bv, st)) {
        if (pl < 2) P.fits = false;  // no grouped kernel for this geometry
        Q = FwdPlan{};               // (plans 2-5 are optional)
        break;
      }
      const int base = (int)Q.ranges.size();
      for (FgBlock b : bv) Q.blocks.push_back(FgBlock{b.x + base, b.y, b.z, b.w});
      Q.ranges.insert(Q.ranges.end(), rv.begin(), rv.end());
      Q.groups.push_back(gr);
      Q.caseA.push_back(fa[gr.t0].caseA != 0);
      Q.staged += st;
      t0 += G;
    }
  }
  if (!P.fits)
    for (FwdPlan& Q : P.plan) Q = FwdPlan{};
  return P;
}

// Block table of the grouped forward projector for nch node chunks: every live
// (ray chunk, group, segment, node chunk), sorted by group size G (waves of work), heaviest
// first.  When every block is resident at once (<= 2 per CU) the second half is reversed so
// the blocks sharing a CU pair heavy with light (dispatch fills one slot per CU, then the
// second); otherwise heaviest-first is the longest-processing-time order.
// cus: the device's compute units (<= 0: table order).  mirror_half: the plan is a mirror-mode
// context's half geometry; pair_xcds: its segments s and kFgSeg-1-s then share an XCD pair
// (ADMM_FWD_MIRROR_XCD=0 turns that off).
inline std::vector<FgBlock> fwd_block_order(const FwdPlan& plan, int nch, int cus, bool mirror_half,
                                            bool pair_xcds) {
  struct Blk {
    FgBlock b;
    int w;
  };
  std::vector<Blk> v;
  for (int c = 0; c < nch; ++c)
    for (const FgBlock& b : plan.blocks) v.push_back({FgBlock{b.x, b.y, b.z + kFgSeg * c, 0}, b.w});
  const int n = (int)v.size();
  auto by_weight = [](std::vector<Blk>& l, int slots) {
    std::stable_sort(l.begin(), l.end(), [](const Blk& a, const Blk& b) { return a.w > b.w; });
    const int m = (int)l.size();
    if (m <= 2 * slots && m > slots) std::reverse(l.begin() + slots, l.end());
  };
  if (cus > 0 && cus % kXcds == 0) {
    // XCD-aware: workgroups are dealt round-robin over the 8 XCDs (id % 8), so launch
    // position p runs on XCD p % 8.  Row segment s goes to XCD s % 8: each XCD's L2 then
    // holds one band of image rows (and of the transposed copy) instead of re-fetching the
    // whole image from the Infinity Cache (LDS-DMA staging reads ~10x the image per launch).
    // Per XCD: heaviest first, the second round reversed (heavy + light per CU pair).
    // Mirror mode (the half geometry): a case-B block of segment s stages rows of band s
    // (virtual plane 0) and of band kFgSeg-1-s (plane 1, row N-1-m), a case-A block only
    // band s of the transposed image (plane 1 mirrors the column).  Segments s and
    // kFgSeg-1-s therefore share an XCD pair: one XCD takes their case-B blocks, the other
    // their case-A blocks, so each band of either image lives in one L2 (segment-per-XCD put
    // every img band in two L2s: FETCH_SIZE 2x, profiles/r4_mirror_xcd.txt).
    const bool paired = mirror_half && pair_xcds;
    auto xcd_of = [&](const FgBlock& b) {
      const int sg = b.z % kFgSeg;
      if (!paired) return sg % kXcds;
      const int pair = std::min(sg, kFgSeg - 1 - sg);
      return (2 * pair + (plan.caseA[b.y] ? 1 : 0)) % kXcds;
    };
    std::vector<std::vector<Blk>> L(kXcds);
    for (const Blk& b : v) L[xcd_of(b.b)].push_back(b);
    for (auto& l : L) by_weight(l, cus / kXcds);
    std::vector<size_t> pos(kXcds, 0);
    v.clear();
    for (int p = 0; p < n; ++p) {
      int x = p % kXcds;
      if (pos[x] >= L[x].size()) {  // this XCD's segment is used up: the fullest list lends
        size_t best = 0;
        for (int y = 0; y < kXcds; ++y)
          if (L[y].size() - pos[y] > best) best = L[y].size() - pos[y], x = y;
      }
      v.push_back(L[x][pos[x]++]);
    }
  } else if (cus > 0) {  // cus <= 0: launch order = table order (tuning comparison)
    by_weight(v, cus);
  }
  std::vector<FgBlock> t(n);
  for (int i = 0; i < n; ++i) t[i] = v[i].b;
  return t;
}

// Forward plan for a batch of nch node chunks, by rounds of resident blocks: a launch of B
// blocks on `slots` = (blocks per CU) x CUs slots runs ceil(B / slots) rounds, and a partial
// last round costs nearly a full one (C3 mirror mode: 1024 / 992 blocks = 2 rounds, 65 us;
// 1056-1296 = 3 rounds, 74-84 us; profiles/r4_fwd_plan_rounds.txt).  Among the plans with the
// fewest rounds, the one staging the fewest row pixels (1024^2, 2048^2: the chunk-aligned plan
// with clipped rays, 107 / 870 us against 130 / 1020 for the best unclipped one) -- except in a
// single round, where the 64-ray plan's equal segment shares keep every XCD on its own row
// band (512^2, one chunk: 33 us against 35-37 for the clipped plans).
// forced (ADMM_FWD_PLAN): that plan if the geometry has it; -1: none.
// A plan with groups but no blocks (a clipped plan of a detector that misses the image: every
// ray's partial is the zero its slot was filled with) cannot be launched -- a grid of 0 blocks --
// and counts as a plan the geometry does not have, chosen or forced.
inline int choose_fwd_plan_index(const int* plan_blocks, const int* plan_n, const double* plan_staged, int nch,
                                 long slots, int forced) {
  auto has = [&](int pl) { return plan_n[pl] > 0 && plan_blocks[pl] > 0; };
  auto rounds = [&](int pl) { return ((long)plan_blocks[pl] * nch + slots - 1) / slots; };
  int pl = 0;
  for (int q = 1; q < kFwdPlans; ++q) {
    if (!has(q)) continue;
    if (rounds(q) < rounds(pl) || (rounds(q) == rounds(pl) && plan_staged[q] < plan_staged[pl])) pl = q;
  }
  if (rounds(pl) == 1 && rounds(0) == 1) pl = 0;
  if (forced >= 0 && forced < kFwdPlans && has(forced)) pl = forced;
  return pl;
}

}  // namespace admm

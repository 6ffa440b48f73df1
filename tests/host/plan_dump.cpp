// plan_dump -- the host planner (csrc/fwd_plan.hpp) on a machine without a GPU: prints the
// geometry's angle records, forward plans, block orders and plan choices as one JSON object.
//
//   plan_dump N n_angles n_det angle_min angle_max det_min det_max dtype what
//
// The four doubles are read by strtod (hex floats keep every bit); dtype is 0 (float32) or 1
// (float64); what is "tables" or "orders" (the tables plus fwd_block_order of every plan for
// 1-3 node chunks, 0 / 256 / 250 compute units, XCD pairing off and on).
// tests/test_fwd_plan_cpu.py builds this file with g++ and with clang++ under the address and
// undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../distributed-inverse-problem-admm_amd/csrc/fwd_plan.hpp"
#include "../../distributed-inverse-problem-admm_amd/csrc/tables.hpp"
#include "../../include/admm_tomo.h"

using namespace admm;

static void print_blocks(const std::vector<FgBlock>& v) {
  std::printf("[");
  for (size_t i = 0; i < v.size(); ++i)
    std::printf("%s[%d,%d,%d,%d]", i ? "," : "", v[i].x, v[i].y, v[i].z, v[i].w);
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc != 10) {
    std::fprintf(stderr, "usage: plan_dump N n_angles n_det angle_min angle_max det_min det_max dtype tables|orders\n");
    return 2;
  }
  admm_geom g{};
  g.N = std::atoi(argv[1]);
  g.n_angles = std::atoi(argv[2]);
  g.n_det = std::atoi(argv[3]);
  g.angle_min = std::strtod(argv[4], nullptr);
  g.angle_max = std::strtod(argv[5], nullptr);
  g.det_min = std::strtod(argv[6], nullptr);
  g.det_max = std::strtod(argv[7], nullptr);
  const int dtype = std::atoi(argv[8]);
  const bool orders = std::strcmp(argv[9], "orders") == 0;

  GeomTables T;
  const char* err = check_geom(g, dtype, 1);
  if (!err) err = geom_tables(g, dtype, T);
  if (err) {
    std::printf("{\"error\": \"%s\"}\n", err);
    return 0;
  }
  const FwdPlans P = build_fwd_plans(g, T.fa);

  std::printf("{\"error\": null, \"kFgG\": %d, \"kFgSeg\": %d, \"kFgWin\": %d, \"kXcds\": %d, \"fits\": %s,\n", kFgG,
              kFgSeg, kFgWin, kXcds, P.fits ? "true" : "false");
  std::printf(" \"Kb\": %.17g, \"kbias\": %d, \"wexp\": %d,\n \"fa\": [", T.Kb, T.kbias, T.wexp);
  for (size_t t = 0; t < T.fa.size(); ++t)
    std::printf("%s[%.17g,%.17g,%.17g,%d]", t ? "," : "", T.fa[t].A0, T.fa[t].A1, T.fa[t].dl, T.fa[t].caseA);
  std::printf("],\n \"plans\": [");
  int plan_n[kFwdPlans], plan_blocks[kFwdPlans];
  double plan_staged[kFwdPlans];
  bool first = true;
  for (int pl = 0; pl < kFwdPlans; ++pl) {
    const FwdPlan& Q = P.plan[pl];
    plan_n[pl] = (int)Q.groups.size();
    plan_blocks[pl] = (int)Q.blocks.size();
    plan_staged[pl] = Q.staged;
    if (Q.groups.empty()) continue;
    std::printf("%s\n  {\"plan\": %d, \"staged_px\": %.17g, \"groups\": [", first ? "" : ",", pl, Q.staged);
    first = false;
    for (size_t i = 0; i < Q.groups.size(); ++i)
      std::printf("%s[%d,%d,%d]", i ? "," : "", Q.groups[i].t0, Q.groups[i].G, (int)Q.caseA[i]);
    std::printf("],\n   \"ranges\": [");
    for (size_t i = 0; i < Q.ranges.size(); ++i) {
      std::printf("%s[[", i ? "," : "");
      for (int q = 0; q < kFgG; ++q) std::printf("%s%d", q ? "," : "", Q.ranges[i].k0[q]);
      std::printf("],[");
      for (int q = 0; q < kFgG; ++q) std::printf("%s%d", q ? "," : "", Q.ranges[i].nk[q]);
      std::printf("]]");
    }
    std::printf("],\n   \"blocks\": ");
    print_blocks(Q.blocks);
    if (orders) {
      std::printf(",\n   \"orders\": [");
      bool fo = true;
      for (int nch = 1; nch <= 3; ++nch)
        for (int cus : {0, 256, 250})
          for (int paired = 0; paired < 2; ++paired) {
            std::printf("%s\n    {\"nch\": %d, \"cus\": %d, \"paired\": %d, \"table\": ", fo ? "" : ",", nch, cus, paired);
            fo = false;
            print_blocks(fwd_block_order(Q, nch, cus, paired != 0, paired != 0));
            std::printf("}");
          }
      std::printf("]");
    }
    std::printf("}");
  }
  std::printf("],\n");
  // plan choices: every plan in one round (more slots than any table), a realistic slot count for
  // 1-4 chunks, and each forced plan
  const long many = 1L << 40;
  std::printf(" \"choice\": {\"one_round\": %d, \"slots512\": [",
              choose_fwd_plan_index(plan_blocks, plan_n, plan_staged, 1, many, -1));
  for (int nch = 1; nch <= 4; ++nch)
    std::printf("%s%d", nch > 1 ? "," : "", choose_fwd_plan_index(plan_blocks, plan_n, plan_staged, nch, 512, -1));
  std::printf("], \"forced\": [");
  for (int f = -1; f <= kFwdPlans; ++f)
    std::printf("%s%d", f >= 0 ? "," : "", choose_fwd_plan_index(plan_blocks, plan_n, plan_staged, 2, 512, f));
  std::printf("]}}\n");
  return 0;
}

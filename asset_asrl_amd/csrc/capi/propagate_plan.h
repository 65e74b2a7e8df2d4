// Launch plan of the batched propagation kernels (csrc/propagate_kernels.h): a pure function of the sizes -- no HIP call, no
// allocation, no environment -- so that it can be tested without a device (asset_hip_propagate_plan), like capi/kkt_map.h.
//
// Without the state-transition matrix (stm = 0) a lane is one initial-value problem: `lanes` = integ_lanes(n) problems per one-wave
// workgroup, the 13 stage vectors of every lane in LDS.
//
// With it (stm = 1) a lane is one (problem, sensitivity column) pair.  The C = n + uv + pv columns of a problem are served by a group
// of G lanes, G the power of two that holds C, at most 64; problems_per_wg = lanes / G groups share the wave.  LDS holds the state's
// 13 stage vectors ONCE per group and the column's per lane:
//     lds_bytes = 13 n 8 (problems_per_wg + lanes)  <=  PROP_LDS_BUDGET.
// While that does not fit, the workgroup runs half as many active lanes; once lanes < G the group is the whole workgroup (G = lanes)
// and a lane walks the columns c, c + G, .. in `passes` = ceil(C / G) integrations of the same problem (the state is integrated again
// in every pass: the same instructions on the same data, so the same steps).  (problem i, column c) is lane
// (i % problems_per_wg) * G + c % G of workgroup i / problems_per_wg in pass c / G: every pair exactly once.
#pragma once
#include <cstddef>

namespace asset_hip {

constexpr std::size_t PROP_LDS_BUDGET = 48 * 1024;   // static + dynamic LDS of one workgroup (integ_kernels.h: integ_lanes uses the same)
constexpr int PROP_STAGES = 13;                      // rk_tables.h: RK_STAGES

struct PropPlan {
  int group;             // G: lanes that serve one problem (1 without the STM)
  int lanes;             // active lanes of the 64-thread workgroup
  int passes;            // columns a lane walks
  int problems_per_wg;
  long long lds_bytes;
  long long grid;        // workgroups
  int columns;           // C (0 without the STM)
};

constexpr PropPlan propagate_plan(int n, int uv, int pv, long long m, int stm) {
  PropPlan p{1, 64, 1, 64, 0, 0, 0};
  if (n < 1 || uv < 0 || pv < 0 || m < 1) return PropPlan{0, 0, 0, 0, 0, 0, 0};
  const std::size_t stage = std::size_t(PROP_STAGES) * std::size_t(n) * sizeof(double);
  if (!stm) {
    while (p.lanes > 1 && stage * std::size_t(p.lanes) > PROP_LDS_BUDGET) p.lanes >>= 1;
    p.problems_per_wg = p.lanes;
    p.lds_bytes = (long long)(stage * std::size_t(p.lanes));
  } else {
    p.columns = n + uv + pv;
    int g = 1;
    while (g < p.columns && g < 64) g <<= 1;
    auto bytes = [&](int lanes) {
      const int gg = g < lanes ? g : lanes;
      return stage * std::size_t(lanes / gg + lanes);
    };
    while (p.lanes > 1 && bytes(p.lanes) > PROP_LDS_BUDGET) p.lanes >>= 1;
    p.group = g < p.lanes ? g : p.lanes;
    p.problems_per_wg = p.lanes / p.group;
    p.passes = (p.columns + p.group - 1) / p.group;
    p.lds_bytes = (long long)bytes(p.lanes);
  }
  p.grid = (m + p.problems_per_wg - 1) / p.problems_per_wg;
  return p;
}

}  // namespace asset_hip

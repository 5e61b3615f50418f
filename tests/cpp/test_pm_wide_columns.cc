// pm_host::PlanWideColumns (colmap_amd/csrc/pm_host_plan.h) without a GPU: the step behind PlanRunShape that turns an
// automatic two-column run shape into three columns per wave where the GPU is full. Every case states the shape
// PlanRunShape gives first (that function is not changed: tests/cpp/test_pm_host_plan.cc), then what the new step
// makes of it.
//   g++ -std=c++17 -I include -I colmap_amd/csrc tests/cpp/test_pm_wide_columns.cc
#include "pm_host_plan.h"

#include <cstdio>
#include <vector>

namespace {

using pm_host::HandleColumns;
using pm_host::RunShape;

int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      ++g_fail;                                                            \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

struct Case {
  std::vector<HandleColumns> cols;  // the run's problems
  int ntaps, S;
  bool geom;
  int W, H, live, ncu, cols_switch, help_switch, wide_switch;
  bool fits3;
  int base_C, base_help;  // PlanRunShape
  int C, help;            // after PlanWideColumns
};

RunShape Both(const Case& c, RunShape* base) {
  *base = pm_host::PlanRunShape(c.cols.data(), (int)c.cols.size(), c.ntaps, c.W, c.H, c.live, c.ncu, c.cols_switch,
                                c.help_switch);
  return pm_host::PlanWideColumns(*base, c.cols.data(), (int)c.cols.size(), c.ntaps, c.S, c.geom, c.W, c.H, c.live, c.ncu,
                                  c.cols_switch, c.help_switch, c.wide_switch, c.fits3);
}

std::vector<HandleColumns> Auto(int n, int C = 2) { return std::vector<HandleColumns>((size_t)n, HandleColumns{C, false}); }

}  // namespace

int main() {
  const std::vector<HandleColumns> requested2 = {{2, true}, {2, true}, {2, true}, {2, true}, {2, true}, {2, true}, {2, true}, {2, true}};
  std::vector<HandleColumns> one_requested = Auto(8);
  one_requested[5].requested = true;
  const std::vector<Case> cases = {
      // the benchmark's launch: a sub-batch of 8 of the 16 images alive, 2560 x 1920, S = 20, 256 CUs:
      // 16 x 640 = 10 240 waves at three columns for 4 096 slots
      {Auto(8), 121, 20, false, 2560, 1920, 16, 256, 0, 0, 1, true, 2, 1, 3, 1},
      // ... all 16 in one launch (COLMAP_AMD_PM_BATCH_SPLIT=0)
      {Auto(16), 121, 20, false, 2560, 1920, 16, 256, 0, 0, 1, true, 2, 1, 3, 1},
      // one or two problems alive: one column per wave, with and without the helper, stays
      {Auto(1), 121, 20, false, 2560, 1920, 1, 256, 0, 0, 1, true, 1, 2, 1, 2},
      {Auto(1), 121, 20, false, 2560, 1920, 2, 256, 0, 0, 1, true, 1, 1, 1, 1},
      {Auto(1), 121, 20, false, 2560, 1920, 1, 256, 0, 0, 2, true, 1, 2, 1, 2},   // forced: still not a two-column shape
      // small images: launch latency either way, two columns
      {Auto(16), 121, 20, false, 320, 240, 16, 256, 0, 0, 1, true, 2, 1, 2, 1},
      {Auto(1), 121, 3, false, 64, 48, 1, 256, 0, 0, 1, true, 2, 1, 2, 1},
      // ... unless the switch forces the shape (tests)
      {Auto(1), 121, 3, false, 64, 48, 1, 256, 0, 0, 2, true, 2, 1, 3, 1},
      // the switch off: the shape of PlanRunShape
      {Auto(8), 121, 20, false, 2560, 1920, 16, 256, 0, 0, 0, true, 2, 1, 2, 1},
      // a handle that requested its columns (all of them, one of them): untouched, also when forced
      {requested2, 121, 20, false, 2560, 1920, 16, 256, 0, 0, 1, true, 2, 1, 2, 1},
      {one_requested, 121, 20, false, 2560, 1920, 16, 256, 0, 0, 1, true, 2, 1, 2, 1},
      {one_requested, 121, 20, false, 2560, 1920, 16, 256, 0, 0, 2, true, 2, 1, 2, 1},
      // COLMAP_AMD_PM_COLS = 2 and COLMAP_AMD_PM_HELP = 1 / 2: untouched
      {Auto(8), 121, 20, false, 2560, 1920, 16, 256, 2, 0, 1, true, 2, 1, 2, 1},
      {Auto(8), 121, 20, false, 2560, 1920, 16, 256, 0, 1, 1, true, 2, 1, 2, 1},
      {Auto(8), 121, 20, false, 2560, 1920, 16, 256, 0, 2, 1, true, 1, 2, 1, 2},
      // geometric pass: two columns (its block of three columns does not fit; the rule does not even ask)
      {Auto(8), 121, 20, true, 2560, 1920, 16, 256, 0, 0, 1, false, 2, 1, 2, 1},
      {Auto(8), 121, 20, true, 2560, 1920, 16, 256, 0, 0, 2, true, 2, 1, 2, 1},
      // S = 32: 96 (column, view) items are two passes; S = 21 (63 lanes) is the last single pass, S = 22 not
      {Auto(8), 121, 32, false, 2560, 1920, 16, 256, 0, 0, 1, true, 2, 1, 2, 1},
      {Auto(8), 121, 21, false, 2560, 1920, 16, 256, 0, 0, 1, true, 2, 1, 3, 1},
      {Auto(8), 121, 22, false, 2560, 1920, 16, 256, 0, 0, 1, true, 2, 1, 2, 1},
      // a shape the wave kernels do not hold at three columns keeps two (never the generic family through this rule)
      {Auto(8), 121, 20, false, 2560, 1920, 16, 256, 0, 0, 1, false, 2, 1, 2, 1},
      {Auto(8), 121, 20, false, 2560, 1920, 16, 256, 0, 0, 2, false, 2, 1, 2, 1},
      // many sources: pm_pick_columns gave the handles one column; not a two-column shape
      {Auto(8, 1), 121, 20, false, 2560, 1920, 16, 256, 0, 0, 1, true, 1, 1, 1, 1},
      // another window: the generic family's four columns, untouched
      {Auto(8, 4), 49, 20, false, 2560, 1920, 16, 256, 0, 0, 1, true, 4, 1, 4, 1},
      {Auto(8, 2), 49, 20, false, 2560, 1920, 16, 256, 0, 0, 2, true, 2, 1, 2, 1},
      // the threshold, 2 x 16 x 256 = 8 192 waves at three columns: 16 x ceil(1534 / 3) = 8 192, 16 x ceil(1533 / 3) = 8 176
      {Auto(8), 121, 20, false, 2560, 1534, 16, 256, 0, 0, 1, true, 2, 1, 3, 1},
      {Auto(8), 121, 20, false, 2560, 1533, 16, 256, 0, 0, 1, true, 2, 1, 2, 1},
      // ... counted over everything alive on the device (a launch of 8 with 8 alive: 5 120 waves) and on the shorter side
      {Auto(8), 121, 20, false, 2560, 1920, 8, 256, 0, 0, 1, true, 2, 1, 2, 1},
      {Auto(8), 121, 20, false, 1533, 2560, 16, 256, 0, 0, 1, true, 2, 1, 2, 1},
      // ... and against the device's own slots: 64 CUs, 4 x 512 = 2 048 = 2 x 1 024; 4 x 511 below
      {Auto(4), 121, 20, false, 1536, 1536, 4, 64, 0, 0, 1, true, 2, 1, 3, 1},
      {Auto(4), 121, 20, false, 1533, 1536, 4, 64, 0, 0, 1, true, 2, 1, 2, 1},
  };
  for (const Case& c : cases) {
    RunShape base;
    const RunShape s = Both(c, &base);
    const int at = (int)(&c - cases.data());
    if (base.C != c.base_C || base.help != c.base_help)
      std::fprintf(stderr, "case %d: PlanRunShape gave C = %d, help = %d\n", at, base.C, base.help);
    CHECK(base.C == c.base_C && base.help == c.base_help);
    if (s.C != c.C || s.help != c.help) std::fprintf(stderr, "case %d: got C = %d, help = %d\n", at, s.C, s.help);
    CHECK(s.C == c.C && s.help == c.help);
  }
  // the step never lowers a shape and never produces anything but {3, 1} or its input
  for (int C = 1; C <= 8; ++C)
    for (int help = 1; help <= 2; ++help)
      for (int wide = 0; wide <= 2; ++wide) {
        const std::vector<HandleColumns> cols = Auto(8, C);
        const RunShape s = pm_host::PlanWideColumns({C, help}, cols.data(), 8, 121, 20, false, 2560, 1920, 16, 256, 0, 0, wide, true);
        const bool raised = C == 2 && help == 1 && wide != 0;
        CHECK(s.C == (raised ? 3 : C) && s.help == help);
      }
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("pm wide columns checks OK (%d cases)\n", (int)cases.size());
  return 0;
}

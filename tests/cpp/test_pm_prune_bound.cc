// The bound behind the prune of the 11 x 11 sweep kernels (pm_kernels.hip: sweep_wave_body, P4 in two stages) without a
// GPU, by brute force: a cost sum is accumulated in draw order in float, every term is >= +0, and the sum with an
// arbitrary subset of its terms replaced by +0 -- the evaluations that wait for stage 2 -- must never exceed the finished
// sum in the same arithmetic. From that the decision follows: a hypothesis whose bound is strictly above the finished
// sum of hypothesis 0 fails pick_best's `ci <= min_cost` with its bound exactly as with its finished sum, also when that
// sum is a NaN. Random terms of the kernel's shape (costs in [0, 2], geom_reg x a capped geometric cost) and of every
// magnitude down to denormals, with and without the geometric term, a million trials.
//   g++ -std=c++17 -ffp-contract=off tests/cpp/test_pm_prune_bound.cc
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (++g_fail < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                      \
  } while (0)

constexpr int kMaxDraws = 15;

// cost_sums (pm_kernels.hip): acc += cost; with the geometric pass acc += geom_reg * geo; draw order
float Sum(const float* cost, const float* geo, const bool* waits, int M, bool geom, float geom_reg) {
  float acc = 0.0f;
  for (int m = 0; m < M; ++m) {
    acc += waits[m] ? 0.0f : cost[m];
    if (geom) acc += geom_reg * (waits[m] ? 0.0f : geo[m]);
  }
  return acc;
}

// pick_best's test of one hypothesis against the running minimum
bool Wins(float ci, float min_cost) { return ci <= min_cost; }

float FromBits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}

}  // namespace

int main() {
  std::mt19937 rng(20240607);
  std::uniform_real_distribution<float> unit(0.0f, 1.0f);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const bool none[kMaxDraws] = {};
  long pruned = 0, trials = 0;
  for (int trial = 0; trial < 1000000; ++trial, ++trials) {
    const int M = 1 + (int)(rng() % kMaxDraws);
    const bool geom = (rng() & 1u) != 0;
    const float geom_reg = geom ? 0.3f * (float)(rng() % 8) : 0.0f;
    const int kind = (int)(rng() % 4);
    float cost[kMaxDraws], geo[kMaxDraws];
    bool waits[kMaxDraws];
    for (int m = 0; m < M; ++m) {
      if (kind == 0) {  // the kernel's terms: max(0, min(2, 1 - ncc)), a capped geometric cost
        cost[m] = std::fmax(0.0f, std::fmin(2.0f, 2.5f * unit(rng) - 0.25f));
        geo[m] = std::fmin(3.0f, 4.0f * unit(rng));
      } else if (kind == 1) {  // any non-negative finite bit pattern, denormals and +0 included
        cost[m] = FromBits(rng() % 0x7f800000u);
        geo[m] = FromBits(rng() % 0x7f800000u);
      } else if (kind == 2) {  // ties: every term the same value (a flat patch: 2.0)
        cost[m] = 2.0f;
        geo[m] = 3.0f;
      } else {  // magnitudes that round differently with and without their neighbours
        cost[m] = std::ldexp(1.0f + unit(rng), (int)(rng() % 48) - 24);
        geo[m] = std::ldexp(1.0f + unit(rng), (int)(rng() % 48) - 24);
      }
      waits[m] = (rng() & 1u) != 0;
    }
    const float full = Sum(cost, geo, none, M, geom, geom_reg);
    const float bound = Sum(cost, geo, waits, M, geom, geom_reg);
    EXPECT(bound <= full);
    // the decision: pruned means "cannot win"; the reference value is hypothesis 0's finished sum, near the two sums
    const unsigned pick = rng() % 8u;
    const float ref = pick == 0 ? bound : pick == 1 ? full : (pick & 1u ? bound : full) * (0.5f + unit(rng));
    if (bound > ref) {
      ++pruned;
      EXPECT(!Wins(full, ref));
      EXPECT(!Wins(bound, ref));
      // a waiting evaluation that would have made the finished sum a NaN changes nothing either
      EXPECT(!Wins(full + nan, ref));
    }
    EXPECT(!(bound > nan));  // against a NaN sum of hypothesis 0 nothing is pruned
    if (kind == 2 && !geom) EXPECT(!(bound > 2.0f * (float)M));  // ties at the bound prune nothing
  }
  EXPECT(pruned > trials / 20);  // the decision branch was exercised
  if (g_fail != 0) {
    std::printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  std::printf("pm prune bound checks OK (%ld trials, %ld pruned)\n", trials, pruned);
  return 0;
}

// regions_segments_sanitize -- the segment planner of the multi-region slabs
// (csrc/regions.cpp: rt_regions_plan_segments, plan_segments, segment_tables) under
// AddressSanitizer + UBSan: seeded random layouts (regions of 16 U(1, 40) cells, 1 to 5
// regions, targets 16 to 256, some with an edge or N off the 16-cell grid or an empty region),
// every output on an exactly-sized buffer and checked against the cutting rule, and the
// kernel's mirrored tables cell by cell.  Host code only.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer \
//       -I include -I radiative-transfer_amd/csrc tools/regions_segments_sanitize.cpp \
//       radiative-transfer_amd/csrc/regions.cpp radiative-transfer_amd/csrc/prm.cpp -o /tmp/regions_segments_sanitize
//   /tmp/regions_segments_sanitize
#include <cstdio>
#include <random>
#include <vector>

#include "regions.hpp"
#include "rtsn.h"

namespace {

int failures = 0;

void expect(bool ok, const char *what, int case_id) {
  if (!ok) {
    std::printf("case %d: %s\n", case_id, what);
    ++failures;
  }
}

void run_layout(int id, std::mt19937 &rng) {
  const int R = 1 + static_cast<int>(rng() % 5);
  std::vector<rt_region> regs(R);
  for (rt_region &r : regs) {
    r = rt_region{};
    r.cells = 16 * (1 + static_cast<int>(rng() % 40));
    r.width = 0.25 + (rng() % 100) / 50.0;
    r.rho = r.kappa_grey = r.T = 1.0;
  }
  const unsigned kind = rng() % 8;
  if (kind == 0) regs[rng() % R].cells += 1 + static_cast<int>(rng() % 15);  // an edge (or N) off the grid
  if (kind == 1) regs[rng() % R].cells = -static_cast<int>(rng() % 3);       // an empty region
  const int target = kind == 2 ? -5 + static_cast<int>(rng() % 21) : 16 + static_cast<int>(rng() % 241);
  std::vector<int> fc;
  const bool valid = rtamd::regions::first_cells(regs.data(), R, fc);
  int Sg = -1;
  rt_status st = rt_regions_plan_segments(regs.data(), R, target, &Sg, nullptr, nullptr);
  if (!valid || !rtamd::regions::segments_admissible(fc)) {
    expect(st == RT_ERR_PARAM && Sg == 0, "an inadmissible layout is RT_ERR_PARAM", id);
    expect(kind == 0 || kind == 1, "an admissible layout refused", id);
    return;
  }
  expect(st == RT_OK && Sg >= R, "an admissible layout plans", id);
  if (st != RT_OK) return;
  const int N = fc.back();
  std::vector<int> first(Sg + 1, -1), reg(Sg, -1);  // exactly sized
  int again = -1;
  st = rt_regions_plan_segments(regs.data(), R, target, &again, first.data(), reg.data());
  expect(st == RT_OK && again == Sg, "the second call agrees", id);
  // the rule, restated: k = ceil(n / t) segments per region, n / 16 units dealt out, longer first
  const int t = target < 16 ? 16 : (target + 15) / 16 * 16;
  expect(rtamd::regions::segment_target(target) == t, "the rounded target", id);
  int s = 0, at = 0;
  for (int r = 0; r < R; ++r) {
    const int n = regs[r].cells, k = (n + t - 1) / t, units = n / 16;
    for (int j = 0; j < k; ++j, ++s) {
      if (s >= Sg) break;
      const int len = 16 * (units / k + (j < units % k ? 1 : 0));
      expect(first[s] == at && reg[s] == r && len <= t && len > 0, "a segment of the rule", id);
      at += len;
    }
    expect(at == fc[r + 1], "a region's segments tile it", id);
  }
  expect(s == Sg && first[Sg] == N, "segments tile [0, N)", id);
  // the kernel's tables: both halves in upwind numbering, the mu < 0 half mirrored
  std::vector<int> sf(first), sr(reg);
  const std::vector<int> tab = rtamd::regions::segment_tables(sf, sr);
  expect(static_cast<int>(tab.size()) == 4 * Sg + 2, "table size", id);
  if (static_cast<int>(tab.size()) != 4 * Sg + 2) return;
  const std::vector<int> cell = rtamd::regions::cell_table(fc);
  const int *f0 = tab.data(), *f1 = f0 + Sg + 1, *r0 = f1 + Sg + 1, *r1 = r0 + Sg;
  expect(f0[0] == 0 && f1[0] == 0 && f0[Sg] == N && f1[Sg] == N, "table ends", id);
  for (int q = 0; q < Sg; ++q) {
    expect(f0[q] < f0[q + 1] && f1[q] < f1[q + 1] && f0[q] % 16 == 0 && f1[q] % 16 == 0, "table order", id);
    for (int k = f1[q]; k < f1[q + 1]; ++k) expect(cell[k] == r1[q], "mu > 0 segment region", id);
    for (int k = f0[q]; k < f0[q + 1]; ++k) expect(cell[N - 1 - k] == r0[q], "mu < 0 segment region (mirrored)", id);
  }
}

}  // namespace

int main() {
  std::mt19937 rng(20261020u);
  for (int id = 0; id < 400; ++id) run_layout(id, rng);
  int n = -1;
  expect(rt_regions_plan_segments(nullptr, 1, 64, &n, nullptr, nullptr) == RT_ERR_ARG, "NULL regions", 1000);
  rt_region one{};
  one.cells = 272;
  one.width = one.rho = one.kappa_grey = one.T = 1.0;
  int first[6], reg[5];
  expect(rt_regions_plan_segments(&one, 1, 64, &n, first, reg) == RT_OK && n == 5, "272 cells at 64", 1001);
  const int want[6] = {0, 64, 128, 176, 224, 272};
  for (int k = 0; k < 6; ++k) expect(first[k] == want[k], "272 cells at 64: 64, 64, 48, 48, 48", 1001);
  expect(rt_regions_plan_segments(&one, 1, 64, nullptr, nullptr, nullptr) == RT_OK, "every output NULL", 1002);
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}

// regions.cpp -- see regions.hpp.  Host code only (no HIP): built into librtsn with the host
// objects, so rt_regions_plan / rt_regions_load work without a GPU.
#include "regions.hpp"

#include <cstdlib>
#include <cstring>
#include <string>

#include "prm.hpp"
#include "wave_cost.hpp"

namespace rtamd::regions {

bool first_cells(const rt_region *r, int R, std::vector<int> &first_cell) {
  first_cell.clear();
  if (!r || R < 1) return false;
  long long at = 0;
  first_cell.push_back(0);
  for (int k = 0; k < R; ++k) {
    if (r[k].cells <= 0 || !(r[k].width > 0.0)) return false;
    at += r[k].cells;
    if (at > 2147483647LL) return false;
    first_cell.push_back(static_cast<int>(at));
  }
  return true;
}

unsigned admissible_mask(const std::vector<int> &first_cell) {
  unsigned mask = 0;
  for (int ci = 0; ci < 4; ++ci) {
    bool ok = true;
    for (int f : first_cell) ok = ok && f % (1 << ci) == 0;
    if (ok) mask |= 1u << ci;
  }
  return mask;
}

Plan plan(const std::vector<int> &first_cell, bool reflective, int max_waves, int want_C, long long nsteps,
          int max_C) {
  max_waves = max_waves < 1 ? 1 : (max_waves > kWaveCostWaves ? kWaveCostWaves : max_waves);
  if (first_cell.size() < 2 || first_cell.back() < 1) return Plan{};
  const int N = first_cell.back();
  const unsigned mask = admissible_mask(first_cell);
  Plan best{};
  double best_cost = 0.0;
  for (int ci = 0; ci < 4; ++ci) {
    if (!(mask >> ci & 1u)) continue;
    const int C = 1 << ci, Lw = N / C;
    if (C > max_C) continue;
    const int used = reflective ? 2 * Lw : Lw, waves = (used + 63) / 64;
    if (waves > max_waves) continue;
    if (C == want_C) return Plan{C, waves, Lw};
    const double cost =
        (static_cast<double>(nsteps) + used - 1) * (reflective ? kTickReflective : kTickVacuum)[ci][waves - 1];
    if (!best.C || cost < best_cost) {
      best = Plan{C, waves, Lw};
      best_cost = cost;
    }
  }
  return best;
}

std::vector<int> cell_table(const std::vector<int> &first_cell) {
  std::vector<int> out(first_cell.empty() ? 0 : first_cell.back());
  for (size_t k = 0; k + 1 < first_cell.size(); ++k)
    for (int c = first_cell[k]; c < first_cell[k + 1]; ++c) out[c] = static_cast<int>(k);
  return out;
}

std::vector<int> lane_table(const std::vector<int> &first_cell, int C) {
  const std::vector<int> cell = cell_table(first_cell);
  const int N = static_cast<int>(cell.size()), Lw = N / C;
  std::vector<int> out(static_cast<size_t>(2) * Lw);
  for (int j = 0; j < Lw; ++j) {
    out[j] = cell[N - 1 - j * C];  // mu < 0: upwind cell k is physical cell N - 1 - k
    out[Lw + j] = cell[j * C];
  }
  return out;
}

bool segments_admissible(const std::vector<int> &first_cell) {
  if (first_cell.size() < 2 || first_cell.back() < 1) return false;
  for (int f : first_cell)
    if (f % kSegmentUnit) return false;
  return true;
}

int segment_target(long long target_cells) {
  if (target_cells < kSegmentUnit) return kSegmentUnit;
  if (target_cells > 2147483647LL - kSegmentUnit) target_cells = 2147483647LL - kSegmentUnit;
  return static_cast<int>((target_cells + kSegmentUnit - 1) / kSegmentUnit * kSegmentUnit);
}

int plan_segments(const std::vector<int> &first_cell, long long target_cells, std::vector<int> &seg_first,
                  std::vector<int> &seg_region) {
  seg_first.clear();
  seg_region.clear();
  if (!segments_admissible(first_cell)) return 0;
  const int target = segment_target(target_cells);
  seg_first.push_back(0);
  for (size_t r = 0; r + 1 < first_cell.size(); ++r) {
    const int n = first_cell[r + 1] - first_cell[r], units = n / kSegmentUnit;
    const int k = (n - 1) / target + 1;  // ceil(n / target) <= units
    const int base = units / k, longer = units % k;
    int at = first_cell[r];
    for (int j = 0; j < k; ++j) {
      at += (base + (j < longer ? 1 : 0)) * kSegmentUnit;
      seg_first.push_back(at);
      seg_region.push_back(static_cast<int>(r));
    }
  }
  return static_cast<int>(seg_region.size());
}

std::vector<int> segment_tables(const std::vector<int> &seg_first, const std::vector<int> &seg_region) {
  const size_t Sg = seg_region.size();
  std::vector<int> out(2 * (Sg + 1) + 2 * Sg);
  if (!Sg || seg_first.size() != Sg + 1) return std::vector<int>();
  const int N = seg_first.back();
  int *first0 = out.data(), *first1 = first0 + Sg + 1, *reg0 = first1 + Sg + 1, *reg1 = reg0 + Sg;
  for (size_t s = 0; s <= Sg; ++s) {
    first0[s] = N - seg_first[Sg - s];
    first1[s] = seg_first[s];
  }
  for (size_t s = 0; s < Sg; ++s) {
    reg0[s] = seg_region[Sg - 1 - s];
    reg1[s] = seg_region[s];
  }
  return out;
}

}  // namespace rtamd::regions

// ---------------------------------------------------------------------------
// C ABI (include/rtsn.h "multi-region slabs", the host-only part)
// ---------------------------------------------------------------------------
// rtsn_api.hip: the text rt_last_error(NULL) returns (weak: this unit also builds alone, under
// the host sanitizer, tools/regions_sanitize.cpp)
namespace rtsn_detail {
__attribute__((weak)) void set_last_error(const char *msg);
}

namespace {
rt_status rfail(rt_status st, const std::string &msg) {
  if (rtsn_detail::set_last_error) rtsn_detail::set_last_error(msg.c_str());
  return st;
}
}  // namespace

extern "C" rt_status rt_regions_plan(const rt_region *r, int nregions, int reflective, int max_waves,
                                     int *cells_per_lane, int *waves, int *lanes) {
  return rt_regions_plan_steps(r, nregions, reflective, max_waves, 1000, cells_per_lane, waves, lanes);
}

extern "C" rt_status rt_regions_plan_steps(const rt_region *r, int nregions, int reflective, int max_waves,
                                           long long nsteps, int *cells_per_lane, int *waves, int *lanes) {
  if (!r || nregions < 1) return rfail(RT_ERR_ARG, "rt_regions_plan: NULL regions or nregions < 1");
  if (max_waves < 1 || max_waves > rtamd::kWaveCostWaves) return rfail(RT_ERR_ARG, "rt_regions_plan: 1..8 waves");
  if (nsteps < 1) return rfail(RT_ERR_ARG, "rt_regions_plan_steps: nsteps < 1");
  std::vector<int> fc;
  if (!rtamd::regions::first_cells(r, nregions, fc))
    return rfail(RT_ERR_PARAM, "regions: every region needs cells > 0 and width > 0");
  const rtamd::regions::Plan p = rtamd::regions::plan(fc, reflective != 0, max_waves, 0, nsteps);
  if (cells_per_lane) *cells_per_lane = p.C;
  if (waves) *waves = p.waves;
  if (lanes) *lanes = p.lanes;
  if (!p.C)
    return rfail(RT_ERR_PARAM, "regions: no chain of 1, 2, 4 or 8 cells per lane both divides every region edge "
                               "and fits the waves (N <= 512 at C = 1, 256 reflective; edges on multiples of 8 "
                               "allow 4096, 2048 reflective)");
  return RT_OK;
}

extern "C" rt_status rt_regions_plan_segments(const rt_region *r, int nregions, int target_cells, int *segments,
                                              int *first_cell, int *segment_region) {
  if (!r || nregions < 1) return rfail(RT_ERR_ARG, "rt_regions_plan_segments: NULL regions or nregions < 1");
  if (segments) *segments = 0;
  std::vector<int> fc, sf, sr;
  if (!rtamd::regions::first_cells(r, nregions, fc))
    return rfail(RT_ERR_PARAM, "regions: every region needs cells > 0 and width > 0");
  const int Sg = rtamd::regions::plan_segments(fc, target_cells, sf, sr);
  if (!Sg)
    return rfail(RT_ERR_PARAM, "regions: segments need N and every region's first cell on multiples of 16");
  if (segments) *segments = Sg;
  if (first_cell) std::memcpy(first_cell, sf.data(), sizeof(int) * sf.size());
  if (segment_region) std::memcpy(segment_region, sr.data(), sizeof(int) * sr.size());
  return RT_OK;
}

// one block: the regions, then (with the .prm's opacity table) the G opacities they share
extern "C" rt_status rt_regions_load(const char *prm_path, const char *table_dir, rt_region **out, int *nregions) {
  if (!prm_path || !out || !nregions) return rfail(RT_ERR_ARG, "rt_regions_load: NULL argument");
  *out = nullptr;
  *nregions = 0;
  rtamd::ParameterHandler ph(prm_path, table_dir ? table_dir : "");
  if (ph.status() != RT_OK) return rfail(ph.status(), ph.error());
  if (!ph.get_have_regions()) return RT_OK;
  const int R = ph.get_num_regions(), G = ph.get_G();
  const bool kap = ph.get_have_group_absorption_opacities();
  const size_t bytes = sizeof(rt_region) * R + (kap ? sizeof(double) * G : 0);
  char *block = static_cast<char *>(std::malloc(bytes));
  if (!block) return rfail(RT_ERR_NOMEM, "rt_regions_load: out of memory");
  rt_region *r = reinterpret_cast<rt_region *>(block);
  double *kappa = nullptr;
  if (kap) {
    kappa = reinterpret_cast<double *>(block + sizeof(rt_region) * R);
    std::memcpy(kappa, ph.group_kappa().data(), sizeof(double) * G);
  }
  const std::vector<double> &t = ph.regions();
  for (int k = 0; k < R; ++k) {
    r[k].cells = static_cast<int>(t[5 * k]);
    r[k].width = t[5 * k + 1];
    r[k].rho = t[5 * k + 2];
    r[k].kappa_grey = t[5 * k + 3];
    r[k].T = t[5 * k + 4];
    r[k].group_kappa = kappa;
  }
  *out = r;
  *nregions = R;
  return RT_OK;
}

extern "C" void rt_regions_free(rt_region *r) { std::free(r); }

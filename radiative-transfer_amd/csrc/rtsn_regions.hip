// rtsn_regions.hip -- the device side of a region handle (include/rtsn.h "multi-region
// slabs"; the host logic is regions.cpp): per-region group tables, the lane -> region and
// cell -> region tables the kernels index, the initial state, the region getters, and the
// change between chain mode and segment mode (the segment plan's tables).
// rt_create_regions itself sits with the other constructors in rtsn_api.hip; the per-region
// cell maps are built in rtsn_lines.hip (region_maps_s).

#include "rtsn_internal.hpp"

using namespace rtamd;
using namespace rtsn_detail;

// Before the handle's own group table is used: one table per region by the routine every
// handle uses (phys::build_group_table), with that region's rho, kappa and T.
rt_status rtsn_detail::setup_regions(rt_solver *s, const rt_region *r, int nregions) {
  if (!regions::first_cells(r, nregions, s->first_cell))
    return fail(s, RT_ERR_PARAM, "regions: every region needs cells > 0 and width > 0");
  s->regions.resize(nregions);
  for (int k = 0; k < nregions; ++k) {
    rt_solver::Region &g = s->regions[k];
    g.p = s->p;
    g.p.rho = r[k].rho;
    g.p.kappa_grey = r[k].kappa_grey;
    g.p.T = r[k].T;
    if (r[k].group_kappa) g.kappa.assign(r[k].group_kappa, r[k].group_kappa + s->p.G);
    g.p.group_kappa = g.kappa.empty() ? nullptr : g.kappa.data();
    g.dx = r[k].width / r[k].cells;
    if (rt_status st = phys::build_group_table(g.p, g.gt))
      return fail(s, st, "group table: group edges must increase");
  }
  s->wave = 2;  // the wavefront where a chain fits
  if (!region_wave_plan(s, s->wave_max).C) {
    if (!regions::segments_admissible(s->first_cell))
      return fail(s, RT_ERR_PARAM, "regions: no chain of 1, 2, 4 or 8 cells per lane both divides every region edge "
                                   "and fits 8 waves, and the region edges are not multiples of 16 (segments)");
    s->seg_mode = true;  // long lines: the pipelined segment pass (create plans the segments)
    s->wave = 0;
    s->pipe = 2;
  }
  return RT_OK;
}

// Chain mode -> segment mode: the caller has checked the layout, that nothing is queued and
// that no material coupling is on.  The stored state is exact and every position at the same
// time; the segments are planned for the current time block (resegment).
rt_status rtsn_detail::enter_segment_mode(rt_solver *s) {
  if (s->seg_mode) return RT_OK;
  const int T0 = s->T;
  if (!region_block(s->T)) s->T = default_time_block(s->scheme);
  s->seg_mode = true;
  s->Sg = 0;  // no plan yet: resegment allocates for the planner's segments and uploads the tables
  s->seg_T = 0;
  if (rt_status st = resegment(s)) {
    s->seg_mode = false;
    s->T = T0;
    s->seg_T = 0;  // (the uniform segmentation is never used by the chain)
    s->Sg = 1;
    return st;
  }
  s->wave = 0;
  s->pipe = 2;
  return RT_OK;
}

void rtsn_detail::leave_segment_mode(rt_solver *s) {  // drained (complete) by the caller
  s->seg_mode = false;
  s->pipe = 1;
  s->pipe_set = false;
}

rt_status rtsn_detail::upload_segment_tables(rt_solver *s) {
  const std::vector<int> t = regions::segment_tables(s->seg_first, s->seg_region);
  if (t.empty() || static_cast<int>(s->seg_region.size()) != s->Sg)
    return fail(s, RT_ERR_STATE, "regions: no segment plan");
  if (!s->seg_tab.p) {
    const size_t most = static_cast<size_t>(s->p.N) / regions::kSegmentUnit;
    if (dalloc(s->seg_tab, sizeof(int) * (4 * most + 2)) != hipSuccess)
      return fail(s, RT_ERR_NOMEM, "device allocation: segment tables");
  }
  return upload(s, s->seg_tab, t.data(), sizeof(int) * t.size());
}

WavePlan rtsn_detail::region_wave_plan(const rt_solver *s, int wave_max) {
  // a coupled handle only ever launches one step: the chain is planned for that (regions.hpp);
  // with the opacity law or table on, among the law form's 1, 2 and 4 cells per lane -- by the tick
  // costs measured for the map form (nobody has measured a law tick: DESIGN.md §9)
  const regions::Plan p = regions::plan(s->first_cell, s->p.bc_left_indicator == 2, wave_max, s->wave_cells,
                                        s->material ? 1 : 1000, (s->law || s->table) ? kLawChainCells : 8);
  return WavePlan{p.C, p.waves, p.lanes};
}

rt_status rtsn_detail::upload_regions(rt_solver *s) {
  const int R = static_cast<int>(s->regions.size()), N = s->p.N, Gl = s->Gl, M = s->p.M;
  // the chains' lane tables, one per admissible C
  std::vector<int> lanes;
  const unsigned mask = regions::admissible_mask(s->first_cell);
  for (int ci = 0; ci < 4; ++ci) {
    s->lane_off[ci] = -1;
    if (!(mask >> ci & 1u)) continue;
    const std::vector<int> t = regions::lane_table(s->first_cell, 1 << ci);
    s->lane_off[ci] = static_cast<long long>(lanes.size());
    lanes.insert(lanes.end(), t.begin(), t.end());
  }
  const std::vector<int> cells = regions::cell_table(s->first_cell);
  // per region: rho kappa_g and compute_balance's emission term (solver.cpp:262-272) of the
  // handle's groups, then dx
  std::vector<double> med(static_cast<size_t>(2) * R * Gl + R);
  const double ac = phys::kRadA * phys::kLight;
  for (int k = 0; k < R; ++k) {
    const rt_solver::Region &g = s->regions[k];
    for (int gl = 0; gl < Gl; ++gl) {
      const double rk = g.gt.rho[s->g_lo + gl] * g.gt.kappa[s->g_lo + gl];
      med[static_cast<size_t>(k) * Gl + gl] = rk;
      med[static_cast<size_t>(R + k) * Gl + gl] = rk * ac * std::pow(g.p.T, 4) * g.dx;
    }
    med[static_cast<size_t>(2) * R * Gl + k] = g.dx;
  }
  hipError_t e = dalloc(s->lane_region, sizeof(int) * lanes.size());
  if (!e) e = dalloc(s->cell_region, sizeof(int) * cells.size());
  if (!e) e = dalloc(s->rmedium, sizeof(double) * med.size());
  if (e) return fail(s, RT_ERR_NOMEM, std::string("device allocation: ") + hipGetErrorString(e));
  rt_status st;
  if ((st = upload(s, s->lane_region, lanes.data(), sizeof(int) * lanes.size()))) return st;
  if ((st = upload(s, s->cell_region, cells.data(), sizeof(int) * cells.size()))) return st;
  if ((st = upload(s, s->rmedium, med.data(), sizeof(double) * med.size()))) return st;
  // psi = B_g (solver.cpp:165-181) generalised: every cell at its own region's B_g, through
  // the ends path (ends (M, Gl, N, 2): i + M (g + Gl (c + N node)))
  std::vector<double> ends(static_cast<size_t>(2) * M * Gl * N);
  for (int node = 0; node < 2; ++node)
    for (int c = 0; c < N; ++c) {
      const phys::GroupTable &gt = s->regions[cells[c]].gt;
      for (int gl = 0; gl < Gl; ++gl) {
        double *dst = ends.data() + static_cast<size_t>(M) * (gl + static_cast<size_t>(Gl) * (c + static_cast<size_t>(N) * node));
        for (int i = 0; i < M; ++i) dst[i] = gt.B[s->g_lo + gl];
      }
    }
  return rt_set_ends(s, ends.data());
}

extern "C" rt_status rt_get_regions(rt_solver *s, int *nregions, int *first_cell) {
  if (!s) return fail(nullptr, RT_ERR_ARG, "rt_get_regions: NULL handle");
  if (nregions) *nregions = regional(s) ? static_cast<int>(s->regions.size()) : 1;
  if (first_cell) {
    if (regional(s)) {
      std::copy(s->first_cell.begin(), s->first_cell.end(), first_cell);
    } else {
      first_cell[0] = 0;
      first_cell[1] = s->p.N;
    }
  }
  return RT_OK;
}

extern "C" rt_status rt_get_region_data(rt_solver *s, int region, double *B, double *dBdT, double *kappa, double *dx) {
  if (!s) return fail(nullptr, RT_ERR_ARG, "rt_get_region_data: NULL handle");
  const int R = regional(s) ? static_cast<int>(s->regions.size()) : 1;
  if (region < 0 || region >= R) return fail(s, RT_ERR_ARG, "rt_get_region_data: no such region");
  const phys::GroupTable &gt = regional(s) ? s->regions[region].gt : s->gt;
  if (B) std::copy(gt.B.begin(), gt.B.end(), B);
  if (dBdT) std::copy(gt.dBdT.begin(), gt.dBdT.end(), dBdT);
  if (kappa) std::copy(gt.kappa.begin(), gt.kappa.end(), kappa);
  if (dx) *dx = regional(s) ? s->regions[region].dx : s->p.X / s->p.N;
  return RT_OK;
}

// rtsn_material.hip -- material-temperature coupling (include/rtsn.h "material"):
// per-cell Planck emission and its T derivative, the coupled sweep with fused angular sums,
// the T update implicit in the material's own emission and the owed emission it implies; on a
// coupled region handle in segment mode, the temperature-dependent opacity (the opacity law).

#include "rtsn_internal.hpp"

using namespace rtamd;
using namespace rtsn_detail;

// ---------------------------------------------------------------------------
// material-temperature coupling (include/rtsn.h)
// ---------------------------------------------------------------------------

template <int S>
static rt_status unit_maps_s(rt_solver *s) {
  return line_maps_s<S>(s, true, s->map_unit, s->hmap_unit);
}

// the kernels' f argument of the temperature-dependent opacity in force: the law's f(x) [N]
// (stride 0), the table's f_g(x) from the handle's first group on (stride G), or none
static const double *opacity_f(const rt_solver *s) {
  if (s->table) return static_cast<const double *>(s->ftab.p) + s->g_lo;
  return s->law ? static_cast<const double *>(s->fscale.p) : nullptr;
}
static int opacity_fstride(const rt_solver *s) { return s->table ? s->p.G : 0; }

static rt_status material_planck(rt_solver *s) {
  HIP_TRY(s, launch_planck_cells(s->pc, static_cast<const double *>(s->Tcell.p), static_cast<double *>(s->Bcell.p),
                                 s->stream));
  return RT_OK;
}

// dt W sum_g rho kappa_g dB_g/dT(T_max) / rho_cv over all G groups (rt_material_stability): the
// emission's stiffness at the hottest cell, 1 / (1 + number) the Fleck factor there
// (gt, rho_cv: the handle's own medium, or one region's; fg: nullptr, or the opacity table's f_g
// of every group there)
static double material_stability_number(const rt_solver *s, const phys::GroupTable &gt, double rho_cv, double T_max,
                                        const double *fg = nullptr) {
  const int G = s->p.G;
  std::vector<double> lo(s->gt.e_edge.begin(), s->gt.e_edge.begin() + G), hi(s->gt.e_edge.begin() + 1,
                                                                             s->gt.e_edge.begin() + G + 1);
  std::vector<double> B(G, 0.0), dB(G, 0.0), mu(s->M_full), wt(s->M_full);
  if (T_max > 0.0) phys::PlanckIntegrator().group_integrals(T_max, G, lo.data(), hi.data(), B.data(), dB.data());
  phys::gauss_legendre(s->M_full, phys::kFourPi, mu.data(), wt.data());
  double W = 0.0, sum = 0.0;
  for (double w : wt) W += w;
  for (int g = 0; g < G; ++g) sum += gt.rho[g] * gt.kappa[g] * (fg ? fg[g] : 1.0) * dB[g] * phys::kBoltzmannJPK;
  return s->p.dt * W * sum / rho_cv;
}

// the opacity law's scale of region k at temperature T (the device's opacity_scale, kernels.hip)
static double opacity_scale_host(const rt_solver *s, int k, double T) {
  const double n = s->law_n[k];
  const double v = T > 0.0 && std::isfinite(T) ? std::pow(T / s->law_Tref[k], -n)
                                               : (n > 0.0 ? s->law_max : (n < 0.0 ? s->law_min : 1.0));
  return std::min(std::max(v, s->law_min), s->law_max);
}

// the opacity table's f_g of region k at temperature T, every group (the device's
// opacity_table_kernel, kernels.hip: the same bracket, t and fma)
static void opacity_table_host(const rt_solver *s, int k, double T, double *f) {
  const int nT = s->tab_nT, G = s->p.G;
  int j = 0;
  double t = 0.0;
  if (T > 0.0 && std::isfinite(T) && T >= s->tab_T[0]) {
    if (T >= s->tab_T[nT - 1]) {
      j = nT - 1;
    } else {
      while (j + 2 < nT && T >= s->tab_T[j + 1]) ++j;
      t = std::log(T / s->tab_T[j]) * s->tab_r[j];
    }
  }
  const double *l0 = s->tab_lnf.data() + (static_cast<size_t>(k) * nT + j) * G;
  const double *l1 = j + 1 < nT ? l0 + G : l0;
  for (int g = 0; g < G; ++g) f[g] = std::exp(std::fma(t, l1[g] - l0[g], l0[g]));
}

// the energy table's c_v of region k at temperature T (the device's material_energy, kernels.hip:
// the same bracket, t and fma); rho_cv in rt_material_stability's number with the table on
static double heat_capacity_host(const rt_solver *s, int k, double T) {
  const int nT = s->eos_nT, R = regional(s) ? static_cast<int>(s->regions.size()) : 1;
  const double *Tg = s->eos_tab.data(), *r = Tg + nT, *lne = r + (nT - 1) + static_cast<size_t>(k) * nT;
  const double *sk = r + (nT - 1) + static_cast<size_t>(R) * nT + static_cast<size_t>(k) * (nT - 1);
  const double *c0 = r + (nT - 1) + static_cast<size_t>(R) * (2 * nT - 1);
  if (!(T >= Tg[0])) return c0[k];
  int j = 0;
  while (j + 2 < nT && T >= Tg[j + 1]) ++j;
  const double t = std::log(T / Tg[j]) * r[j];
  return sk[j] * std::exp(std::fma(t, lne[j + 1] - lne[j], lne[j])) / T;
}

extern "C" rt_status rt_material_stability(rt_solver *s, double *number) {
  if (!s || !number) return fail(s, RT_ERR_ARG, "rt_material_stability: bad argument");
  if (!s->material) return fail(s, RT_ERR_STATE, "rt_material_stability: material coupling is off");
  HIP_TRY(s, hipSetDevice(s->device));
  std::vector<double> T(s->p.N);
  HIP_TRY(s, hipMemcpyAsync(T.data(), s->Tcell.p, sizeof(double) * T.size(), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  if (regional(s)) {  // the stiffest region, each at its own hottest cell
    double worst = 0.0;
    for (size_t k = 0; k < s->regions.size(); ++k) {
      double T_max = 0.0;
      for (int c = s->first_cell[k]; c < s->first_cell[k + 1]; ++c)
        if (std::isfinite(T[c])) T_max = std::max(T_max, T[c]);
      std::vector<double> fg;
      if (s->table) {  // the table's f_g there, inside the sum
        fg.resize(s->p.G);
        opacity_table_host(s, static_cast<int>(k), T_max, fg.data());
      }
      const double cv = s->eos ? heat_capacity_host(s, static_cast<int>(k), T_max) : s->rho_cv_r[k];
      double number = material_stability_number(s, s->regions[k].gt, cv, T_max, s->table ? fg.data() : nullptr);
      if (s->law) number *= opacity_scale_host(s, static_cast<int>(k), T_max);  // the opacity there
      worst = std::max(worst, number);
    }
    *number = worst;
    return RT_OK;
  }
  double T_max = 0.0;
  for (double t : T)
    if (std::isfinite(t)) T_max = std::max(T_max, t);
  *number = material_stability_number(s, s->gt, s->eos ? heat_capacity_host(s, 0, T_max) : s->rho_cv, T_max);
  return RT_OK;
}

// The Planck kernels' arguments that do not depend on the medium, and the quadrature's weight sums.
static void material_common(rt_solver *s) {
  PlanckCells &pc = s->pc;
  phys::PlanckIntegrator().nodes(pc.node, pc.weight);
  pc.e_edge = static_cast<const double *>(s->edges.p);
  pc.G = s->p.G;
  pc.g_lo = s->g_lo;
  pc.Gl = s->Gl;
  pc.N = s->p.N;
  pc.a_c = phys::rad_a_long() * phys::kLight;
  pc.kcon = phys::kBoltzmannJPK;
  pc.accuracy = std::numeric_limits<double>::epsilon();
  pc.sigma = static_cast<const double *>(s->sigma.p);
  pc.dTlast = static_cast<const double *>(s->dTlast.p);
  pc.owed = static_cast<double *>(s->owed.p);
  pc.dB = static_cast<double *>(s->dBcell.p);
  pc.Beff = static_cast<double *>(s->Beff.p);
  pc.bpart = static_cast<double *>(s->bpart.p);
  pc.b_scale = s->d_lo == 0 ? 1.0 : 0.0;  // direction shards: every one holds all groups, count b once
  pc.sigma_all = static_cast<const double *>(s->sigma_all.p);
  pc.Bcell = static_cast<const double *>(s->Bcell.p);
  s->wsum = 0.0;
  for (double w : s->wt) s->wsum += w;
  std::vector<double> mu_all(s->M_full), wt_all(s->M_full);
  phys::gauss_legendre(s->M_full, phys::kFourPi, mu_all.data(), wt_all.data());
  s->wsum_all = 0.0;
  for (double w : wt_all) s->wsum_all += w;
}

// the energy table off: the update's forms with the constant rho_cv the handle was enabled with
static void energy_table_off(rt_solver *s) {
  s->eos = false;
  s->pc.eos_T = s->pc.eos_r = s->pc.eos_lne = s->pc.eos_s = s->pc.eos_c0 = nullptr;
  s->pc.eos_nT = 0;
}

// Coupling on a slab of regions: the coupled step is the REG && CB wavefront chain (chain mode)
// or the line walk (segment mode, sweep_walk_kernel) on unit-B maps (one set per region), the
// material kernels take each cell's own sigma_g(x) and rho_cv(x).  No fused sums or correction
// tables: phi comes from the moments kernels after each step.

// the argument checks rt_material_enable_regions and rt_material_enable_segments share (s not NULL)
static rt_status region_coupling_args(rt_solver *s, const char *fn, const double *rho_cv, int nregions) {
  if (!rho_cv) return fail(s, RT_ERR_ARG, std::string(fn) + ": NULL rho_cv");
  const int R = regional(s) ? static_cast<int>(s->regions.size()) : 1;
  if (nregions != R)
    return fail(s, RT_ERR_ARG, std::string(fn) + ": nregions must be the handle's " + std::to_string(R));
  for (int k = 0; k < R; ++k)
    if (!(rho_cv[k] > 0.0) || !std::isfinite(rho_cv[k]))
      return fail(s, RT_ERR_ARG, std::string(fn) + ": every rho_cv must be > 0");
  return RT_OK;
}

// ... and their body, on a region handle in either mode: the buffers, the unit-B maps, T0, the
// region tables and the first emission
static rt_status enable_region_coupling(rt_solver *s, const double *rho_cv, const double *T_cells) {
  const int R = static_cast<int>(s->regions.size());
  if (s->p.use_correction && s->p.V != 0.0)
    return fail(s, RT_ERR_PARAM, "material coupling needs the v/c correction off (V = 0 or use_correction = 0)");
  HIP_TRY(s, hipSetDevice(s->device));
  rt_status st = finalize(s);  // queued steps run on the uncoupled plan's chain first
  if (st) return st;
  const size_t N = s->p.N, NG = N * s->Gl, G = s->p.G;
  if (!s->Tcell.p) {
    hipError_t e = dalloc(s->Tcell, sizeof(double) * N);
    if (!e) e = dalloc(s->Bcell, sizeof(double) * NG);
    if (!e) e = dalloc(s->Beff, sizeof(double) * NG);
    if (!e) e = dalloc(s->owed, sizeof(double) * NG);
    if (!e) e = dalloc(s->dBcell, sizeof(double) * NG);
    if (!e) e = dalloc(s->dTlast, sizeof(double) * N);
    if (!e) e = dalloc(s->bpart, sizeof(double) * N);
    if (!e) e = dalloc(s->qbuf, sizeof(double) * 2 * N);
    if (!e) e = dalloc(s->edges, sizeof(double) * (G + 1));
    if (!e) e = dalloc(s->rmaterial, sizeof(double) * (R + R * G));
    if (!e) e = dalloc(s->map_unit, s->map.bytes);
    if (!e) e = dalloc(s->hmap_unit, s->hmap.bytes);
    if (e) return fail(s, RT_ERR_NOMEM, std::string("material buffers: ") + hipGetErrorString(e));
  }
  s->phi_fused = false;  // a line's directions sit in different workgroups
  switch (s->scheme) {
    case SCHEME_BE: st = region_maps_s<SCHEME_BE>(s, true); break;
    case SCHEME_CN: st = region_maps_s<SCHEME_CN>(s, true); break;
    default: st = region_maps_s<SCHEME_BDF2>(s, true); break;
  }
  if (st) return st;
  std::vector<double> T0(N);
  for (int k = 0; k < R; ++k)
    std::fill(T0.begin() + s->first_cell[k], T0.begin() + s->first_cell[k + 1], s->regions[k].p.T);
  if (T_cells) std::copy(T_cells, T_cells + N, T0.begin());
  if ((st = upload(s, s->Tcell, T0.data(), N * sizeof(double)))) return st;
  HIP_TRY(s, hipMemsetAsync(s->dTlast.p, 0, sizeof(double) * N, s->stream));  // nothing owed yet
  HIP_TRY(s, hipMemsetAsync(s->owed.p, 0, sizeof(double) * NG, s->stream));
  HIP_TRY(s, hipMemsetAsync(s->dBcell.p, 0, sizeof(double) * NG, s->stream));
  if ((st = upload(s, s->edges, s->gt.e_edge.data(), (G + 1) * sizeof(double)))) return st;
  {
    std::vector<double> rm(R + R * G);
    for (int k = 0; k < R; ++k) {
      rm[k] = rho_cv[k];
      for (size_t g = 0; g < G; ++g) rm[R + k * G + g] = s->regions[k].gt.rho[g] * s->regions[k].gt.kappa[g];
    }
    if ((st = upload(s, s->rmaterial, rm.data(), rm.size() * sizeof(double)))) return st;
  }
  material_common(s);
  PlanckCells &pc = s->pc;
  pc.sigma_all = nullptr;  // (every cell reads its region's row)
  pc.cell_region = static_cast<const int *>(s->cell_region.p);
  pc.rsigma = static_cast<const double *>(s->rmedium.p);  // its first [regions][Gl] doubles: rho kappa
  pc.rho_cv_r = static_cast<const double *>(s->rmaterial.p);
  pc.rsigma_all = pc.rho_cv_r + R;
  s->rho_cv_r.assign(rho_cv, rho_cv + R);
  s->rho_cv = rho_cv[0];
  s->law = s->table = false;  // (enabled again: the opacity law and table are off until set)
  pc.fscale = nullptr;
  pc.law_n = pc.law_Tref = nullptr;
  pc.ftab = pc.gratio = nullptr;
  pc.tab_T = pc.tab_r = pc.tab_lnf = nullptr;
  pc.tab_nT = 0;
  energy_table_off(s);  // (enabled again: the energy table is off until set)
  if ((st = material_planck(s))) return st;
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // T0 dies at return
  s->material = true;  // from here the chain is the one-step plan's (region_wave_plan)
  return RT_OK;
}

extern "C" rt_status rt_material_enable_regions(rt_solver *s, const double *rho_cv, int nregions,
                                                const double *T_cells) {
  if (!s) return fail(nullptr, RT_ERR_ARG, "rt_material_enable_regions: NULL handle");
  if (rt_status st = region_coupling_args(s, "rt_material_enable_regions", rho_cv, nregions)) return st;
  if (!regional(s)) return rt_material_enable(s, rho_cv[0], T_cells);
  if (s->seg_mode)
    return fail(s, RT_ERR_STATE, "rt_material_enable_regions: the handle is in segment mode, which takes "
                                 "rt_material_enable_segments (the coupled step is the line walk there, not the "
                                 "wavefront chain)");
  return enable_region_coupling(s, rho_cv, T_cells);
}

extern "C" rt_status rt_material_enable_segments(rt_solver *s, const double *rho_cv, int nregions,
                                                 const double *T_cells) {
  if (!s) return fail(nullptr, RT_ERR_ARG, "rt_material_enable_segments: NULL handle");
  if (rt_status st = region_coupling_args(s, "rt_material_enable_segments", rho_cv, nregions)) return st;
  if (!regional(s))
    return fail(s, RT_ERR_STATE, "rt_material_enable_segments: not a region handle; a plain handle takes "
                                 "rt_material_enable");
  if (!s->seg_mode)
    return fail(s, RT_ERR_STATE, "rt_material_enable_segments: the handle is in chain mode, which takes "
                                 "rt_material_enable_regions");
  return enable_region_coupling(s, rho_cv, T_cells);
}

extern "C" rt_status rt_material_enable(rt_solver *s, double rho_cv, const double *T_cells) {
  if (!s) return fail(nullptr, RT_ERR_ARG, "rt_material_enable: NULL handle");
  if (regional(s))
    return fail(s, RT_ERR_STATE, "rt_material_enable: a region handle takes rt_material_enable_regions (one rho_cv "
                                 "per region)");
  if (!(rho_cv > 0.0) || !std::isfinite(rho_cv)) return fail(s, RT_ERR_ARG, "rt_material_enable: rho_cv must be > 0");
  if (s->p.use_correction && s->p.V != 0.0)
    return fail(s, RT_ERR_PARAM, "material coupling needs the v/c correction off (V = 0 or use_correction = 0)");
  HIP_TRY(s, hipSetDevice(s->device));
  rt_status st = finalize(s);  // the state at the requested time, exact
  if (st) return st;
  const size_t N = s->p.N, NG = N * s->Gl;
  if (!s->Tcell.p) {
    hipError_t e = dalloc(s->Tcell, sizeof(double) * N);
    if (!e) e = dalloc(s->Bcell, sizeof(double) * NG);
    if (!e) e = dalloc(s->Beff, sizeof(double) * NG);
    if (!e) e = dalloc(s->owed, sizeof(double) * NG);
    if (!e) e = dalloc(s->dBcell, sizeof(double) * NG);
    if (!e) e = dalloc(s->dTlast, sizeof(double) * N);
    if (!e) e = dalloc(s->bpart, sizeof(double) * N);
    if (!e) e = dalloc(s->qbuf, sizeof(double) * 2 * N);
    if (!e) e = dalloc(s->edges, sizeof(double) * (s->p.G + 1));
    if (!e) e = dalloc(s->sigma_all, sizeof(double) * s->p.G);
    if (!e) e = dalloc(s->map_unit, s->map.bytes);
    if (!e) e = dalloc(s->hmap_unit, s->hmap.bytes);
    s->phi_fused = 64 % s->H == 0;  // a group's lines never straddle a wave
    if (!e && s->phi_fused) e = dalloc(s->phi_part, sizeof(double) * 4 * NG);  // [half sums, corrections][half]
    if (e) return fail(s, RT_ERR_NOMEM, std::string("material buffers: ") + hipGetErrorString(e));
  }
  switch (s->scheme) {
    case SCHEME_BE: st = unit_maps_s<SCHEME_BE>(s); break;
    case SCHEME_CN: st = unit_maps_s<SCHEME_CN>(s); break;
    default: st = unit_maps_s<SCHEME_BDF2>(s); break;
  }
  if (st) return st;
  {  // coupled passes are single steps: segments for the coupled kernel's occupancy
     // (measured on SL: 16 waves per CU instead is slower for BE, even for BDF2), or the
     // caller's rt_set_segmentation
    int w = 0;
    HIP_TRY(s, coupled_occupancy(s->scheme, &w));
    if (s->seg_set && s->seg_wgs) w = s->seg_wgs;
    const int sg0 = s->Sg;
    segment_lines(s, w);
    s->seg_T = 0;  // sized for the coupled pass
    s->seg_w = 0;
    if (s->Sg != sg0) {
      if (2LL * s->Q * s->Sg >= (1LL << 31)) return fail(s, RT_ERR_PARAM, "too many segments");
      HIP_TRY(s, alloc_segments(s));
      s->tau.assign(chain_positions(s), s->target);  // every position at the same, requested time
      s->resume_lo = s->resume_hi = -1;
    }
  }
  std::vector<double> T0(N, s->p.T);
  if (T_cells) std::copy(T_cells, T_cells + N, T0.begin());
  if (s->phi_fused)  // the correction sums of segment-0 cells are never written: zero
    HIP_TRY(s, hipMemsetAsync(s->phi_part.p, 0, s->phi_part.bytes, s->stream));
  if ((st = upload(s, s->Tcell, T0.data(), N * sizeof(double)))) return st;
  HIP_TRY(s, hipMemsetAsync(s->dTlast.p, 0, sizeof(double) * N, s->stream));  // nothing owed yet
  HIP_TRY(s, hipMemsetAsync(s->owed.p, 0, sizeof(double) * NG, s->stream));
  HIP_TRY(s, hipMemsetAsync(s->dBcell.p, 0, sizeof(double) * NG, s->stream));
  if ((st = upload(s, s->edges, s->gt.e_edge.data(), (s->p.G + 1) * sizeof(double)))) return st;
  {
    std::vector<double> sig(s->p.G);
    for (int g = 0; g < s->p.G; ++g) sig[g] = s->gt.rho[g] * s->gt.kappa[g];
    if ((st = upload(s, s->sigma_all, sig.data(), sig.size() * sizeof(double)))) return st;
  }
  material_common(s);
  s->rho_cv = rho_cv;
  energy_table_off(s);  // (enabled again: the energy table is off until set)
  if ((st = material_planck(s))) return st;
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // T0 dies at return
  s->material = true;
  return RT_OK;
}

extern "C" rt_status rt_material_sweep(rt_solver *s, double *d_q) {
  if (!s) return fail(nullptr, RT_ERR_ARG, "rt_material_sweep: NULL handle");
  if (!s->material) return fail(s, RT_ERR_STATE, "rt_material_sweep: call rt_material_enable first");
  HIP_TRY(s, hipSetDevice(s->device));
  rt_status st = check_validation(s);
  if (st) return st;
  if ((st = ensure_equilibrium(s))) return st;
  double *q = d_q ? d_q : static_cast<double *>(s->qbuf.p);
  const double *B = static_cast<const double *>(s->Bcell.p), *sig = static_cast<const double *>(s->sigma.p);
  const double *bp = static_cast<const double *>(s->bpart.p);
  if (regional(s)) {  // one launch of the coupled chain (segment mode: the line walk), then phi by the moments kernels
    if ((st = finalize(s))) return st;
    if ((st = s->seg_mode ? walk_coupled_pass(s) : wave_coupled_pass(s))) return st;
    if ((st = compute_moments(s))) return st;
    HIP_TRY(s, launch_material_q(static_cast<const double *>(s->mom.p), 1, B, static_cast<const double *>(s->rmedium.p),
                                 s->wsum, bp, q, s->Gl, s->p.N, s->stream, static_cast<const int *>(s->cell_region.p),
                                 opacity_f(s), opacity_fstride(s)));
    return RT_OK;
  }
  if (s->phi_fused) {
    // one pass over the state: the pass sums w psi of its provisional cells, the
    // correction kernel adds the cross-segment correction's share (no state
    // traffic) and the stored state keeps its correction pending for the next pass
    if ((st = complete(s))) return st;
    if ((st = enqueue_pass(s, 1, true))) return st;
    if (s->pending) {
      if ((st = enqueue_fold(s, 1, false))) return st;
      SegArgs a = seg_args(s);
      a.Gl = s->Gl;
      a.H = s->H;
      a.phic = static_cast<double *>(s->phi_part.p) + 2 * static_cast<size_t>(s->p.N) * s->Gl;
      a.wt = static_cast<const double *>(s->muwt.p) + s->p.M;
      // BE, CN: closed form, lanes over cells (phi_correction_geo_kernel); rt_set_phi_correction_form
      // 1 keeps the walk for comparison
      const bool walk = s->phi_corr_form == 1;
      if (phi_correction_geo_supported(s->scheme, a) && !walk) {
        HIP_TRY(s, launch_phi_correction_geo(s->scheme, a, s->stream));
        HIP_TRY(s, launch_material_q(static_cast<const double *>(s->phi_part.p), 4, B, sig, s->wsum, bp, q, s->Gl,
                                     s->p.N, s->stream));
        return RT_OK;
      }
      // BDF2: closed form by tabulated rows (phi_correction_rows_kernel)
      if (phi_correction_rows_supported(s->scheme, a) && !walk) {
        if (!s->corr_rows.p) {
          HIP_TRY(s, dalloc(s->corr_rows, sizeof(double) * corr_rows_doubles(s->scheme, s->Lpad)));
          HIP_TRY(s, launch_corr_rows(s->scheme, static_cast<const double *>(s->map.p),
                                      static_cast<double *>(s->corr_rows.p), s->Lpad, s->stream));
        }
        HIP_TRY(s, launch_phi_correction_rows(s->scheme, a, static_cast<const double *>(s->corr_rows.p), s->stream));
        HIP_TRY(s, launch_material_q(static_cast<const double *>(s->phi_part.p), 4, B, sig, s->wsum, bp, q, s->Gl,
                                     s->p.N, s->stream));
        return RT_OK;
      }
      // the walk along a segment is a dependent chain: cut each segment into sub-segments
      // (multiples of 16 cells) until the grid holds ~8 waves per SIMD
      const long long segs = 2LL * s->Q * s->Sg;
      const int nsub = static_cast<int>(
          std::max<long long>(1, std::min<long long>((32LL * s->cus + segs - 1) / segs, s->Ls / 16)));
      const int Lsub = ((s->Ls + nsub - 1) / nsub + 15) / 16 * 16;
      if (nsub > 1 && s->corr_pow_L != Lsub) {
        if (!s->corr_pow.p) HIP_TRY(s, dalloc(s->corr_pow, sizeof(double) * 2 * tri_count(s->K) * s->Lpad));
        HIP_TRY(s, launch_correction_power(s->scheme, static_cast<const double *>(s->map.p),
                                           static_cast<double *>(s->corr_pow.p), Lsub, s->Lpad, s->stream));
        s->corr_pow_L = Lsub;
      }
      HIP_TRY(s, launch_phi_correction(s->scheme, a, nsub, Lsub, static_cast<const double *>(s->corr_pow.p),
                                       s->stream));
    }
    HIP_TRY(s, launch_material_q(static_cast<const double *>(s->phi_part.p), s->pending ? 4 : 2, B, sig, s->wsum, bp,
                                 q, s->Gl, s->p.N, s->stream));
    return RT_OK;
  }
  if ((st = finalize(s))) return st;
  if ((st = enqueue_pass(s, 1, true))) return st;
  if ((st = compute_moments(s))) return st;  // finalizes the pass
  HIP_TRY(s, launch_material_q(static_cast<const double *>(s->mom.p), 1, B, sig, s->wsum, bp, q, s->Gl, s->p.N,
                               s->stream));
  return RT_OK;
}

extern "C" rt_status rt_material_update(rt_solver *s, const double *d_q) {
  if (!s) return fail(nullptr, RT_ERR_ARG, "rt_material_update: NULL handle");
  if (!s->material) return fail(s, RT_ERR_STATE, "rt_material_update: call rt_material_enable first");
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, launch_material_update(s->pc, static_cast<double *>(s->Tcell.p),
                                    d_q ? d_q : static_cast<const double *>(s->qbuf.p),
                                    static_cast<double *>(s->dTlast.p), s->p.dt, s->rho_cv, s->wsum_all, s->p.N,
                                    s->stream));
  return material_planck(s);
}

extern "C" rt_status rt_material_step(rt_solver *s, int nsteps) {
  if (!s || nsteps < 0) return fail(s, RT_ERR_ARG, "rt_material_step: bad argument");
  if (s->g_lo != 0 || s->g_hi != s->p.G || s->d_hi > 0)
    return fail(s, RT_ERR_STATE, "rt_material_step: the handle holds a group or direction-pair shard; sum q "
                                 "over the shards (rt_material_sweep, all-reduce, rt_material_update)");
  for (int n = 0; n < nsteps; ++n) {
    rt_status st = rt_material_sweep(s, nullptr);
    if (st) return st;
    if ((st = rt_material_update(s, nullptr))) return st;
  }
  return RT_OK;
}

// which: 0 T(x), 1 B per cell, 2 the next step's emission per cell, 3 the last update's dT per cell
static rt_status material_fetch(rt_solver *s, int which, double *out, const char *what) {
  if (!s || !out) return fail(s, RT_ERR_ARG, std::string(what) + ": bad argument");
  if (!s->material) return fail(s, RT_ERR_STATE, std::string(what) + ": material coupling is off");
  HIP_TRY(s, hipSetDevice(s->device));
  const size_t count = which == 0 || which == 3 ? s->p.N : static_cast<size_t>(s->p.N) * s->Gl;
  const void *src = which == 0 ? s->Tcell.p : (which == 1 ? s->Bcell.p : (which == 2 ? s->Beff.p : s->dTlast.p));
  HIP_TRY(s, hipMemcpyAsync(out, src, sizeof(double) * count, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return RT_OK;
}

extern "C" rt_status rt_get_temperature(rt_solver *s, double *T_cells) {
  return material_fetch(s, 0, T_cells, "rt_get_temperature");
}

extern "C" rt_status rt_get_cell_planck(rt_solver *s, double *B) { return material_fetch(s, 1, B, "rt_get_cell_planck"); }

extern "C" rt_status rt_get_cell_emission(rt_solver *s, double *Beff) {
  return material_fetch(s, 2, Beff, "rt_get_cell_emission");
}

extern "C" rt_status rt_get_material_last_dt(rt_solver *s, double *dT) {
  return material_fetch(s, 3, dT, "rt_get_material_last_dt");
}

extern "C" rt_status rt_get_material_transit(rt_solver *s, double *E) {
  if (!s || !E) return fail(s, RT_ERR_ARG, "rt_get_material_transit: bad argument");
  if (!s->material) return fail(s, RT_ERR_STATE, "rt_get_material_transit: material coupling is off");
  HIP_TRY(s, hipSetDevice(s->device));
  DeviceBuf d;
  HIP_TRY(s, dalloc(d, sizeof(double) * s->p.N));
  // (a region handle: each cell's own sigma_g(x), rmedium's first [regions][Gl] doubles)
  hipError_t e = launch_material_transit(
      static_cast<const double *>(s->Bcell.p), static_cast<const double *>(s->Beff.p),
      static_cast<const double *>(s->owed.p), static_cast<const double *>(regional(s) ? s->rmedium.p : s->sigma.p),
      s->p.dt * s->wsum, static_cast<double *>(d.p), s->Gl, s->p.N, s->stream,
      regional(s) ? static_cast<const int *>(s->cell_region.p) : nullptr, opacity_f(s), opacity_fstride(s));
  if (e == hipSuccess) e = hipMemcpyAsync(E, d.p, sizeof(double) * s->p.N, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  (void)hipStreamSynchronize(s->stream);
  d.reset();
  if (e != hipSuccess) return fail(s, RT_ERR_DEVICE, std::string("rt_get_material_transit: ") + hipGetErrorString(e));
  return RT_OK;
}

// ---------------------------------------------------------------------------
// the opacity law (include/rtsn.h rt_material_set_opacity_law)
// ---------------------------------------------------------------------------
// the handle a temperature-dependent opacity needs (rt_material_set_opacity_law and
// rt_material_set_opacity_table share the preconditions, statuses and messages)
// chain: the *_chain calls (a coupled region handle in chain mode; the mode picks the call, as with
// rt_material_enable_regions / rt_material_enable_segments); seg: the segment-mode sibling's name
static rt_status opacity_handle(rt_solver *s, const char *fn, bool chain = false, const char *seg = "") {
  if (!s) return fail(nullptr, RT_ERR_ARG, std::string(fn) + ": NULL handle");
  if (chain) {
    if (!regional(s))
      return fail(s, RT_ERR_STATE, std::string(fn) + ": not a region handle; the law needs a region handle "
                                   "(rt_create_regions, rt_material_enable_regions; a uniform slab is one region)");
    if (s->seg_mode)
      return fail(s, RT_ERR_STATE, std::string(fn) + ": the handle is in segment mode, which takes " + seg);
    if (!s->material)
      return fail(s, RT_ERR_STATE, std::string(fn) + ": call rt_material_enable_regions first");
    return RT_OK;
  }
  if (!regional(s))
    return fail(s, RT_ERR_STATE, std::string(fn) + ": not a region handle; the law needs a region handle in segment "
                                 "mode (rt_create_regions, rt_set_wavefront(s, 0), rt_material_enable_segments)");
  if (!s->seg_mode)
    return fail(s, RT_ERR_STATE, std::string(fn) + ": the handle is in chain mode; the law runs on the line walk of "
                                 "segment mode (rt_set_wavefront(s, 0), then rt_material_enable_segments), or on the "
                                 "chain through " + fn + "_chain");
  if (!s->material)
    return fail(s, RT_ERR_STATE, std::string(fn) + ": call rt_material_enable_segments first");
  return RT_OK;
}

// chain mode: the law form of the chain has 1, 2 and 4 cells per lane (kLawChainCells), so one of
// them must divide the region edges and fit rt_set_wavefront_waves' waves.  Checked before anything
// changes; with a law or table already on the plan already is such a chain
static rt_status law_chain_fits(rt_solver *s, const char *fn) {
  if (s->law || s->table) return RT_OK;
  if (regions::plan(s->first_cell, s->p.bc_left_indicator == 2, s->wave_max, s->wave_cells, 1, kLawChainCells).C)
    return RT_OK;
  return fail(s, RT_ERR_PARAM, std::string(fn) + ": no chain of 1, 2 or 4 cells per lane both divides every region edge "
                               "and fits the handle's waves (rt_set_wavefront_waves); segment mode is the route for "
                               "this slab (rt_set_wavefront(s, 0), rt_material_enable_segments)");
}

static rt_status set_opacity_law(rt_solver *s, const char *fn, bool chain, const double *exponent, const double *T_ref,
                                 int nregions, double scale_min, double scale_max) {
  if (rt_status st = opacity_handle(s, fn, chain, "rt_material_set_opacity_law")) return st;
  const int R = static_cast<int>(s->regions.size());
  const bool off = !exponent && nregions == 0;
  if (!off) {
    if (!exponent || !T_ref) return fail(s, RT_ERR_ARG, std::string(fn) + ": NULL exponent or T_ref");
    if (nregions != R)
      return fail(s, RT_ERR_ARG, std::string(fn) + ": nregions must be the handle's " + std::to_string(R));
    for (int k = 0; k < R; ++k) {
      if (!std::isfinite(exponent[k])) return fail(s, RT_ERR_ARG, std::string(fn) + ": every exponent must be finite");
      if (!(T_ref[k] > 0.0) || !std::isfinite(T_ref[k]))
        return fail(s, RT_ERR_ARG, std::string(fn) + ": every T_ref must be finite and > 0");
    }
    if (!(scale_min > 0.0) || !(scale_min <= scale_max) || !std::isfinite(scale_max))
      return fail(s, RT_ERR_ARG, std::string(fn) + ": need 0 < scale_min <= scale_max < infinity");
  }
  if (off && !s->law) return RT_OK;  // (also with the table on: the law is off, the table stays)
  if (chain && !off)
    if (rt_status st = law_chain_fits(s, fn)) return st;
  HIP_TRY(s, hipSetDevice(s->device));
  const size_t N = s->p.N;
  if (!s->fscale.p) {
    hipError_t e = dalloc(s->fscale, sizeof(double) * 2 * N);  // f, then the Planck pass's f_old / f_new
    if (!e) e = dalloc(s->lawtab, sizeof(double) * 2 * R);
    if (e) return fail(s, RT_ERR_NOMEM, std::string("opacity law buffers: ") + hipGetErrorString(e));
  }
  PlanckCells &pc = s->pc;
  // what was in force: the table is replaced by the law through the same rescale, per group
  const int had_law = s->table ? kOpacityTable : (s->law ? kOpacityLaw : kOpacityNone);
  if (!off) {
    std::vector<double> tab(2 * R);
    std::copy(exponent, exponent + R, tab.begin());
    std::copy(T_ref, T_ref + R, tab.begin() + R);
    if (rt_status st = upload(s, s->lawtab, tab.data(), tab.size() * sizeof(double))) return st;
    s->law_n.assign(exponent, exponent + R);
    s->law_Tref.assign(T_ref, T_ref + R);
    s->law_min = pc.law_min = scale_min;
    s->law_max = pc.law_max = scale_max;
    pc.law_n = static_cast<const double *>(s->lawtab.p);
    pc.law_Tref = pc.law_n + R;
  } else {
    pc.law_n = pc.law_Tref = nullptr;
  }
  pc.fscale = static_cast<double *>(s->fscale.p);
  pc.fratio = pc.fscale + N;
  pc.tab_T = pc.tab_r = pc.tab_lnf = nullptr;  // (a table in force: pc.ftab still holds its f_g, the f_old)
  // f from the current T, and the emission in transit rescaled by f_old / f_new (off: f_new = 1)
  HIP_TRY(s, launch_opacity_rescale(pc, static_cast<const double *>(s->Tcell.p), had_law, s->stream));
  s->law = !off;
  s->table = false;
  pc.ftab = pc.gratio = nullptr;
  if (off) pc.fscale = nullptr;  // the kernels' forms without the law again
  return RT_OK;
}

extern "C" rt_status rt_material_set_opacity_law(rt_solver *s, const double *exponent, const double *T_ref,
                                                 int nregions, double scale_min, double scale_max) {
  return set_opacity_law(s, "rt_material_set_opacity_law", false, exponent, T_ref, nregions, scale_min, scale_max);
}

extern "C" rt_status rt_material_set_opacity_law_chain(rt_solver *s, const double *exponent, const double *T_ref,
                                                       int nregions, double scale_min, double scale_max) {
  return set_opacity_law(s, "rt_material_set_opacity_law_chain", true, exponent, T_ref, nregions, scale_min,
                         scale_max);
}

static rt_status set_opacity_table(rt_solver *s, const char *fn, bool chain, const double *T_grid, int nT,
                                   const double *scale, int nregions) {
  if (rt_status st = opacity_handle(s, fn, chain, "rt_material_set_opacity_table")) return st;
  const int R = static_cast<int>(s->regions.size());
  const size_t N = s->p.N, G = s->p.G;
  const bool off = !T_grid && nT == 0 && nregions == 0;
  if (!off) {
    if (!T_grid || !scale) return fail(s, RT_ERR_ARG, std::string(fn) + ": NULL T_grid or scale");
    if (nregions != R)
      return fail(s, RT_ERR_ARG, std::string(fn) + ": nregions must be the handle's " + std::to_string(R));
    if (nT < 2) return fail(s, RT_ERR_ARG, std::string(fn) + ": the grid needs at least 2 nodes");
    for (int j = 0; j < nT; ++j)
      if (!(T_grid[j] > 0.0) || !std::isfinite(T_grid[j]) || (j && !(T_grid[j] > T_grid[j - 1])))
        return fail(s, RT_ERR_ARG, std::string(fn) + ": T_grid must be finite, > 0 and strictly increasing");
    for (size_t i = 0; i < static_cast<size_t>(R) * nT * G; ++i)
      if (!(scale[i] > 0.0) || !std::isfinite(scale[i]))
        return fail(s, RT_ERR_ARG, std::string(fn) + ": every scale entry must be finite and > 0");
  }
  if (off && !s->table) return RT_OK;  // (also with the law on: the table is off, the law stays)
  if (chain && !off)
    if (rt_status st = law_chain_fits(s, fn)) return st;
  HIP_TRY(s, hipSetDevice(s->device));
  if (!s->ftab.p) {  // f_g(x) of every group, then the Planck pass's f_old / f_new of the handle's
    if (hipError_t e = dalloc(s->ftab, sizeof(double) * N * (G + s->Gl)))
      return fail(s, RT_ERR_NOMEM, std::string("opacity table buffers: ") + hipGetErrorString(e));
  }
  PlanckCells &pc = s->pc;
  const int had = s->table ? kOpacityTable : (s->law ? kOpacityLaw : kOpacityNone);
  if (!off) {
    // nodes, 1 / log(T_{j+1} / T_j) and ln f, formed in long double and rounded once
    const size_t count = 2 * static_cast<size_t>(nT) - 1 + static_cast<size_t>(R) * nT * G;
    std::vector<double> tab(count);
    std::copy(T_grid, T_grid + nT, tab.begin());
    for (int j = 0; j + 1 < nT; ++j)
      tab[nT + j] = static_cast<double>(1.0L / std::log(static_cast<long double>(T_grid[j + 1]) /
                                                        static_cast<long double>(T_grid[j])));
    for (size_t i = 0; i < static_cast<size_t>(R) * nT * G; ++i)
      tab[2 * nT - 1 + i] = static_cast<double>(std::log(static_cast<long double>(scale[i])));
    if (s->tabdev.bytes < count * sizeof(double)) {
      HIP_TRY(s, hipStreamSynchronize(s->stream));  // a smaller table may still be read
      s->tabdev.reset();
      if (hipError_t e = dalloc(s->tabdev, count * sizeof(double)))
        return fail(s, RT_ERR_NOMEM, std::string("opacity table: ") + hipGetErrorString(e));
    }
    if (rt_status st = upload(s, s->tabdev, tab.data(), count * sizeof(double))) return st;
    s->tab_nT = nT;
    s->tab_T.assign(tab.begin(), tab.begin() + nT);
    s->tab_r.assign(tab.begin() + nT, tab.begin() + 2 * nT - 1);
    s->tab_lnf.assign(tab.begin() + 2 * nT - 1, tab.end());
    pc.tab_T = static_cast<const double *>(s->tabdev.p);
    pc.tab_r = pc.tab_T + nT;
    pc.tab_lnf = pc.tab_r + (nT - 1);
    pc.tab_nT = nT;
  } else {
    pc.tab_T = pc.tab_r = pc.tab_lnf = nullptr;
    pc.tab_nT = 0;
  }
  pc.ftab = static_cast<double *>(s->ftab.p);
  pc.gratio = pc.ftab + N * G;
  pc.law_n = pc.law_Tref = nullptr;  // (a law in force: pc.fscale still holds its f(x), the f_old)
  // f_g from the current T, the emission in transit rescaled by f_old,g / f_new,g and paid again,
  // and bpart with or without f_g inside its sum
  HIP_TRY(s, launch_opacity_rescale(pc, static_cast<const double *>(s->Tcell.p), had, s->stream));
  s->table = !off;
  s->law = false;
  pc.fscale = pc.fratio = nullptr;
  if (off) pc.ftab = pc.gratio = nullptr;  // the kernels' forms without the table again
  return RT_OK;
}

extern "C" rt_status rt_material_set_opacity_table(rt_solver *s, const double *T_grid, int nT, const double *scale,
                                                   int nregions) {
  return set_opacity_table(s, "rt_material_set_opacity_table", false, T_grid, nT, scale, nregions);
}

extern "C" rt_status rt_material_set_opacity_table_chain(rt_solver *s, const double *T_grid, int nT,
                                                         const double *scale, int nregions) {
  return set_opacity_table(s, "rt_material_set_opacity_table_chain", true, T_grid, nT, scale, nregions);
}

extern "C" rt_status rt_get_opacity_scale_groups(rt_solver *s, double *f) {
  if (!s || !f) return fail(s, RT_ERR_ARG, "rt_get_opacity_scale_groups: bad argument");
  if (!s->material) return fail(s, RT_ERR_STATE, "rt_get_opacity_scale_groups: material coupling is off");
  const size_t N = s->p.N, G = s->p.G, Gl = s->Gl;
  if (!s->law && !s->table) {
    std::fill(f, f + N * Gl, 1.0);
    return RT_OK;
  }
  HIP_TRY(s, hipSetDevice(s->device));
  std::vector<double> h(s->table ? N * G : N);
  HIP_TRY(s, hipMemcpyAsync(h.data(), s->table ? s->ftab.p : s->fscale.p, sizeof(double) * h.size(),
                            hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  for (size_t c = 0; c < N; ++c)
    for (size_t g = 0; g < Gl; ++g) f[g + Gl * c] = s->table ? h[c * G + s->g_lo + g] : h[c];  // the law: one f per cell
  return RT_OK;
}

extern "C" rt_status rt_get_opacity_scale(rt_solver *s, double *f) {
  if (!s || !f) return fail(s, RT_ERR_ARG, "rt_get_opacity_scale: bad argument");
  if (!s->material) return fail(s, RT_ERR_STATE, "rt_get_opacity_scale: material coupling is off");
  if (s->table)
    return fail(s, RT_ERR_STATE, "rt_get_opacity_scale: the opacity table is on, one f per cell and group: "
                                 "rt_get_opacity_scale_groups reads it");
  if (!s->law) {  // no law: the table opacities
    std::fill(f, f + s->p.N, 1.0);
    return RT_OK;
  }
  HIP_TRY(s, hipSetDevice(s->device));
  HIP_TRY(s, hipMemcpyAsync(f, s->fscale.p, sizeof(double) * s->p.N, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(s, hipStreamSynchronize(s->stream));
  return RT_OK;
}

// ---------------------------------------------------------------------------
// the energy table (include/rtsn.h rt_material_set_energy_table)
// ---------------------------------------------------------------------------
extern "C" rt_status rt_material_set_energy_table(rt_solver *s, const double *T_grid, int nT, const double *energy,
                                                  int nregions) {
  const std::string fn = "rt_material_set_energy_table";
  if (!s) return fail(nullptr, RT_ERR_ARG, fn + ": NULL handle");
  if (!s->material) return fail(s, RT_ERR_STATE, fn + ": material coupling is off; call rt_material_enable first");
  const int R = regional(s) ? static_cast<int>(s->regions.size()) : 1;
  if (!T_grid && nT == 0 && nregions == 0) {  // off: the rho_cv of rt_material_enable* again; T(x) stays
    energy_table_off(s);
    return RT_OK;
  }
  if (!T_grid || !energy) return fail(s, RT_ERR_ARG, fn + ": NULL T_grid or energy");
  if (nregions != R) return fail(s, RT_ERR_ARG, fn + ": nregions must be the handle's " + std::to_string(R));
  if (nT < 2) return fail(s, RT_ERR_ARG, fn + ": the grid needs at least 2 nodes");
  for (int j = 0; j < nT; ++j)
    if (!(T_grid[j] > 0.0) || !std::isfinite(T_grid[j]) || (j && !(T_grid[j] > T_grid[j - 1])))
      return fail(s, RT_ERR_ARG, fn + ": T_grid must be finite, > 0 and strictly increasing");
  for (int k = 0; k < R; ++k)
    for (int j = 0; j < nT; ++j) {
      const double e = energy[static_cast<size_t>(k) * nT + j];
      if (!(e > 0.0) || !std::isfinite(e)) return fail(s, RT_ERR_ARG, fn + ": every energy entry must be finite and > 0");
      if (j && !(e > energy[static_cast<size_t>(k) * nT + j - 1]))
        return fail(s, RT_ERR_ARG, fn + ": every region's energy must be strictly increasing along T_grid");
    }
  HIP_TRY(s, hipSetDevice(s->device));
  // nodes, r_j = 1 / log(T_{j+1} / T_j), ln e, s_j = (ln e_{j+1} - ln e_j) r_j and c_0 = e_0 / T_0, formed in long
  // double and rounded once
  const size_t n1 = static_cast<size_t>(nT) - 1, count = nT + n1 + static_cast<size_t>(R) * (2 * nT - 1) + R;
  std::vector<double> tab(count);
  std::vector<long double> rl(n1);
  std::copy(T_grid, T_grid + nT, tab.begin());
  for (size_t j = 0; j < n1; ++j) {
    rl[j] = 1.0L / std::log(static_cast<long double>(T_grid[j + 1]) / static_cast<long double>(T_grid[j]));
    tab[nT + j] = static_cast<double>(rl[j]);
  }
  double *lne = tab.data() + nT + n1, *sk = lne + static_cast<size_t>(R) * nT, *c0 = sk + static_cast<size_t>(R) * n1;
  for (int k = 0; k < R; ++k) {
    const double *e = energy + static_cast<size_t>(k) * nT;
    for (int j = 0; j < nT; ++j) lne[static_cast<size_t>(k) * nT + j] = static_cast<double>(std::log(static_cast<long double>(e[j])));
    for (size_t j = 0; j < n1; ++j)
      sk[k * n1 + j] = static_cast<double>(
          (std::log(static_cast<long double>(e[j + 1])) - std::log(static_cast<long double>(e[j]))) * rl[j]);
    c0[k] = static_cast<double>(static_cast<long double>(e[0]) / static_cast<long double>(T_grid[0]));
  }
  for (size_t i = 0; i < static_cast<size_t>(R) * n1; ++i)
    if (!(sk[i] > 0.0) || !std::isfinite(sk[i]))
      return fail(s, RT_ERR_ARG, fn + ": every region's energy must be strictly increasing along T_grid");
  if (s->eosdev.bytes < count * sizeof(double)) {
    HIP_TRY(s, hipStreamSynchronize(s->stream));  // a smaller table may still be read
    s->eosdev.reset();
    if (hipError_t e = dalloc(s->eosdev, count * sizeof(double)))
      return fail(s, RT_ERR_NOMEM, std::string("energy table: ") + hipGetErrorString(e));
  }
  if (rt_status st = upload(s, s->eosdev, tab.data(), count * sizeof(double))) return st;
  HIP_TRY(s, hipStreamSynchronize(s->stream));  // tab dies at return
  PlanckCells &pc = s->pc;
  pc.eos_T = static_cast<const double *>(s->eosdev.p);
  pc.eos_r = pc.eos_T + nT;
  pc.eos_lne = pc.eos_r + n1;
  pc.eos_s = pc.eos_lne + static_cast<size_t>(R) * nT;
  pc.eos_c0 = pc.eos_s + static_cast<size_t>(R) * n1;
  pc.eos_nT = nT;
  s->eos_nT = nT;
  s->eos_tab = std::move(tab);
  s->eos = true;
  return RT_OK;
}

// which: 0 e(T(x)), 1 c_v(T(x)), by the update's own device function
static rt_status material_energy_fetch(rt_solver *s, int which, double *out, const char *what) {
  if (!s || !out) return fail(s, RT_ERR_ARG, std::string(what) + ": bad argument");
  if (!s->material) return fail(s, RT_ERR_STATE, std::string(what) + ": material coupling is off");
  HIP_TRY(s, hipSetDevice(s->device));
  DeviceBuf d;
  HIP_TRY(s, dalloc(d, sizeof(double) * s->p.N));
  double *dp = static_cast<double *>(d.p);
  hipError_t e = launch_material_energy(s->pc, static_cast<const double *>(s->Tcell.p), s->rho_cv,
                                        which == 0 ? dp : nullptr, which == 1 ? dp : nullptr, s->p.N, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, d.p, sizeof(double) * s->p.N, hipMemcpyDeviceToHost, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  (void)hipStreamSynchronize(s->stream);
  d.reset();
  if (e != hipSuccess) return fail(s, RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
  return RT_OK;
}

extern "C" rt_status rt_get_material_energy(rt_solver *s, double *e) {
  return material_energy_fetch(s, 0, e, "rt_get_material_energy");
}

extern "C" rt_status rt_get_heat_capacity(rt_solver *s, double *cv) {
  return material_energy_fetch(s, 1, cv, "rt_get_heat_capacity");
}

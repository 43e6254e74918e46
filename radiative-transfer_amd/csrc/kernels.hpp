// kernels.hpp -- launch interface of kernels.hip (host side of the C ABI).
#pragma once

#include <hip/hip_runtime.h>

namespace rtamd {

// Register-tiling constants (the measured best).
constexpr int kSweepCells = 16;  // cells per wave held in registers; segment lengths are multiples of this
// rows per chunk held in registers (prefetch depth) for scheme S fusing T steps:
// measured on SL, BDF2 T = 16: 4 rows 8.67, 8 rows 8.33, 16 rows 8.15 ms/step;
// T = 20: 16 rows spill to scratch, 8 rows fit 256 VGPRs + 126 AGPRs
constexpr int chunk_cells(int S, int T) {
  return S == 3 && T >= 20 ? 8 : S == 3 && T >= 12 ? 16 : (S == 3 && T >= 2 ? 8 : kSweepCells);
}
// pipelined passes whose T levels two waves can share (sweep_split_kernel):
// BDF2, where the carried states (5 per level) are what overflows 256 registers
constexpr bool level_split_supported(int S, int T) {
  return S == 3 && (T == 4 || T == 8 || T == 10 || T == 12 || T == 16 || T == 20 || T == 24 || T == 32 || T == 40);
}
// pipelined passes with a one-wave kernel: all but BDF2 beyond 20 levels (its carried
// states would spill; those run split over four waves)
constexpr bool one_wave_block(int S, int T) { return S != 3 || T <= 20; }
// time blocks of the region form of the one-wave pipelined pass (a region handle in segment mode)
constexpr bool region_block(int T) { return (T >= 1 && T <= 8) || T == 10 || T == 12 || T == 16; }
// rows per chunk of the level-split pass (16 rows with T/2 = 8 levels spill past 256 registers)
constexpr int split_chunk_cells() { return 8; }
constexpr int kXcds = 8;                                // gfx950: workgroups are dealt to 8 XCDs round-robin
constexpr int kSweepTile = 64;                          // cells are padded to whole tiles of 64 rows

constexpr int kMaxTimeBlock = 40;                       // full steps fused per pipelined pass (template range)
constexpr int kMaxAlignedBlock = 4;                     // ... per aligned pass (carries a T K correction state)

// Segment propagators of the T-level combined state (KC = T K, packed lower
// triangle of NTC = KC (KC + 1) / 2 entries each): A_T^Ls, A_T^Llast.
constexpr int prop_count(int K, int T) { return (T * K) * (T * K + 1); }

struct SegArgs {
  double2 *E;                 // [2][Nrow][Lpad] (e_in, e_out)
  const double *map;          // [2][map_count<S>][Lpad] per-line affine cell map (cell.hpp)
  const double *hmap;         // [map_count<S>][Lpad] the reflective mu > 0 head cell's map (half 1 lines)
  const double *bdry;         // [2][Lpad] inflow value per line (non-reflective)
  const double *yseg;         // [2][Sg+1][T K][Lpad] true incoming state per segment (fold_kernel)
  const double *yrefl;        // [T K][Lpad] this pass's mu < 0 line outflow state (reflective)
  double *agg_cur;            // [2][Sg][T K][Lpad] segment aggregates of this pass
  double *aggs[2];            // pipelined: aggregates of pass p in aggs[p & 1], [2][Sg][T K][Lpad]
  int N, Nrow, Lpad, Q;
  int Sg, Ls;                 // segments per line, cells per segment (multiple of 16)
  int half0;                  // first half swept by this launch (grid covers 1 or 2 halves)
  int reflective;             // bc_left == 2
  int pending;                // the stored state is provisional: apply the correction
  int pos_lo, npos, pass_lo;  // pipelined: active chain positions and the pass of the first
  int level_waves;            // pipelined: waves per segment, 1 (sweep_block_kernel) or 2, 4 (sweep_split_kernel)
  int tail_levels;            // pipelined (launch_split_tail): position pos_lo runs this many (< T) levels
  double hd;                  // dx / 2
  // material coupling (SWEEP_PASS, T = 1 only): per-cell emission B_g(T(x)),
  // [N][Gl] (g fastest), scaling the map constants stored for B = 1
  const double *bcell;        // nullptr: line-constant source (the reference's constant T)
  int Gl, H;                  // local groups, lines per half per group (line l = i' + H g)
  // ... with the angular sums fused (H divides 64): the pass writes
  // phi[half][x][g] = sum over the half's directions of w_i psi (provisional
  // state), phi_correction_kernel adds the cross-segment correction's share
  double *phi;                // nullptr: not fused (phi from moments_kernel after a finalize)
  double *phic;               // [half][x][g] the correction's share (phi_correction_kernel)
  const double *wt;           // [M] quadrature weights
  // multi-region slabs (kernels_wave.hip, the REG forms only): map is then
  // [nregions][2][map_count<S>][Lpad], and lane_region[half][lanes] the region chain lane j's
  // cells lie in (the mu < 0 half's table the mirror image of the mu > 0 one)
  const int *lane_region;     // nullptr: one medium
  // level-split pipelined pass only (kernels_split.hip): the lean maps of a handle whose source
  // has no psi term, [lean_map_rows()][Lpad]: the mu < 0 lines' packed rows, then the mu > 0
  // lines' (cell.hpp, lean_pattern)
  const double *lmap;         // nullptr: the full map
  // multi-region slabs on long lines (the REG form of the one-wave pipelined pass): every
  // segment lies in one region.  seg_first[half][Sg + 1]: first cell of segment s (and the end
  // of the last) in the half's upwind numbering; seg_region[half][Sg]: its region, the row
  // block of map ([nregions][2][map_count<S>][Lpad]) the segment's cells take.  hmap stays
  // region 0's (the reflective head cell is physical cell 0)
  const int *seg_first;       // nullptr: one medium, segments s * Ls
  const int *seg_region;
};

struct FoldArgs {
  const double *agg;          // [2][Sg][KC][Lpad]
  const double *prop;         // [2][prop_half][Lpad]: A^Ls then A^Llast (packed)
  double *y;                  // [2][Sg+1][KC][Lpad], or [KC][Lpad] when only_last
  int prop_half, Sg, Lpad, half0, nhalf, last_short, only_last;
};

struct Geometry {
  int M, Gl, N, Nrow, Lpad;
};

enum SweepMode {
  SWEEP_PASS = 0,       // one pass of T full steps, every segment at the same time level
  SWEEP_FINALIZE = 1,   // only the pending correction of a T-step pass
  SWEEP_PIPELINED = 2   // one launch of the staggered (pipelined) schedule
};
hipError_t launch_sweep(int scheme, int T, int mode, const SegArgs &a, int grid, hipStream_t st);
// the material-coupled step of a region handle in segment mode (sweep_walk_kernel): one step of
// every line, each 64-line wave walking its whole lines across the segment edges.  a: seg_args
// with the unit-B maps (one set per region), bcell, Gl, H, seg_first and seg_region; N and every
// segment edge multiples of 16; grid = 2 Q, or Q with the reflective left boundary
hipError_t launch_walk(int scheme, const SegArgs &a, int grid, hipStream_t st);
// ... with the opacity law on (sweep_walk_law_kernel): no map; each lane forms its cell's line
// constants from sigma(x) = sigma0[region][group] f(x) and runs the reference algebra (cell.hpp)
struct WalkLaw {
  const double *fscale;       // [N] the law's scale f(x) of every cell (physical cell order)
  const double *rsigma;       // [nregions][Gl] rho kappa of the handle's groups, unscaled
  const double *rdx;          // [nregions] cell width
  const double *mu;           // [M] direction cosines
  double c, tau, dt;          // speed of light, the substep (dt / 2 for BDF2), the step
  // the opacity table (rt_material_set_opacity_table): fscale is then [N][fstride] over all G
  // groups, cell-major like bcell, and a lane reads f of (cell, fgroup0 + its group).  0: the law
  int fstride, fgroup0;
};
hipError_t launch_walk_law(int scheme, const SegArgs &a, const WalkLaw &w, int grid, hipStream_t st);
// the level-split pipelined BDF2 pass (kernels_split.hip): T levels over `waves` waves
hipError_t launch_split(int T, int waves, const SegArgs &a, int grid, hipStream_t st);
hipError_t split_occupancy(int T, int waves, int *workgroups_per_cu);
// a pipelined launch whose position pos_lo runs a.tail_levels < T levels (the run's n mod T
// remainder; vacuum lines), the rest T: (T, waves) pairs split_tail_supported
bool split_tail_supported(int T, int waves);
hipError_t launch_split_tail(int T, int waves, const SegArgs &a, int grid, hipStream_t st);
// segments resident per CU (workgroups of the pass: one wave, or two with level_waves 2)
hipError_t sweep_occupancy(int scheme, int T, int level_waves, int *waves_per_cu);
hipError_t coupled_occupancy(int scheme, int *waves_per_cu);  // the material-coupled pass (T = 1)
hipError_t launch_fold(int KC, const FoldArgs &f, hipStream_t st);
// short lines (kernels_wave.hip): nsteps full steps of every line in one launch, lanes over
// cells (a.Gl, a.H set: lines ell < H Gl).  A line (reflective: a line pair) is a chain of
// `lanes` lanes per line holding C cells each, on `waves` waves of one workgroup (C = 0: too
// long for kWaveMaxWaves waves); waves > 1 hand the chain over through LDS once per tick
// and meet at a barrier every kWaveBlockTicks ticks
constexpr int kWaveMaxWaves = 8;
constexpr int kWaveBlockTicks = 8;
constexpr int kLawChainCells = 4;  // the most cells per lane of the chain's law form
struct WavePlan {
  int C, waves, lanes;
};
WavePlan wavefront_plan(int N, bool reflective, int max_waves);
// law: the opacity law or table on a coupled region chain (a.lane_region and a.bcell set, nsteps 1,
// p.C 1, 2 or 4): the law form of the chain kernels, which hold no map and form each cell's line
// constants from sigma0 f(x) as the line walk does (WalkLaw above)
hipError_t launch_wavefront(int scheme, const WavePlan &p, const SegArgs &a, int nsteps, hipStream_t st,
                            const WalkLaw *law = nullptr);
hipError_t launch_init_state(double2 *E, const double *lineB, const Geometry &g, hipStream_t st);
// reference-layout psi / ends of the cells [c0, c0 + nc) (ends: node 0 block, then node 1)
hipError_t launch_export_psi(const double2 *E, double *psi, const Geometry &g, int c0, int nc, hipStream_t st);
hipError_t launch_export_ends(const double2 *E, double *ends, const Geometry &g, int c0, int nc, hipStream_t st);
hipError_t launch_import_ends(double2 *E, const double *ends, const Geometry &g, int c0, int nc, hipStream_t st);
// form (rt_set_moments_form): 1 the producer/consumer moments_pc_kernel where M/2 is 8, 16 or
// 32, 0 the one-wave moments_kernel; bitwise-identical results
hipError_t launch_moments(const double2 *E, const double *mu, const double *wt, double *phi, double *F,
                          double *phi_plus, const Geometry &g, int form, hipStream_t st);
hipError_t launch_boundary_rows(const double2 *E, double2 *rows, const Geometry &g, hipStream_t st);
// *flag |= 1 if any node of the N real rows of either half is not finite (flag zeroed by the caller)
hipError_t launch_finite_scan(const double2 *E, int *flag, const Geometry &g, hipStream_t st);
// per group: ab = sum_c (rk phi) dx, sr = sum_c src (compute_balance), as a two-level sum
// over contiguous cell ranges; part: balance_scratch_doubles(Gl) doubles of scratch
size_t balance_scratch_doubles(int Gl);
hipError_t launch_balance_sums(const double *phi, const double *rk, const double *src, double dx, double *part,
                               double *ab, double *sr, int Gl, int N, hipStream_t st);
hipError_t launch_group_absorption(const double *phi, const double *sigma, double *out, const Geometry &g,
                                   hipStream_t st);
// the same two read-outs on a slab of regions: cell c lies in region cell_region[c], with
// rk, src, sigma [nregions][Gl] and dx [nregions] (the uniform kernels' arithmetic per cell)
hipError_t launch_balance_sums_regions(const double *phi, const double *rk, const double *src, const double *dx,
                                       const int *cell_region, double *part, double *ab, double *sr, int Gl, int N,
                                       hipStream_t st);
hipError_t launch_group_absorption_regions(const double *phi, const double *sigma, const int *cell_region,
                                           double *out, const Geometry &g, hipStream_t st,
                                           const double *fscale = nullptr,  // the opacity law's f(x)
                                           int fstride = 0);  // > 0, the opacity table: f_g(x) = fscale[x fstride + g]

// Planck group integrals per cell (material coupling): the algorithm of
// Planck.cpp:44-337 in double precision on the device.
struct PlanckCells {
  double node[12], weight[12];  // Gauss-Legendre on [-1, 1] (Planck.cpp:231-337, rounded to double)
  const double *e_edge;         // [G+1] all groups' edges (device)
  int G, g_lo, Gl, N;
  double a_c;                   // rad_a_long() * c (Constants.h:22-23)
  double kcon;                  // jk per keV (correction.cpp:25-36)
  double accuracy;              // series tolerance (Planck.h:96, DBL_EPSILON)
  // the coupling's owed emission (rtsn_material.hip): the last update's dT per cell in;
  // owed and dB (group-major [Gl][N], the kernel's own) updated; Beff = B + the paid share
  // and bpart = b_scale sum_gl sigma[gl] dB/dT out
  const double *sigma;          // [Gl] rho kappa of the handle's groups
  const double *dTlast;         // [N]
  double *owed, *dB;            // [Gl][N]
  double *Beff;                 // [N][Gl]
  double *bpart;                // [N]
  double b_scale;               // 1, or 0 on a direction shard without pair 0 (b counted once)
  const double *sigma_all;      // [G] rho kappa of every group (the update's S(T), all groups)
  const double *Bcell;          // [N][Gl] B_g(T^n) (the update's full-emission cells: owed += B(T') - B(T^n))
  // a slab of regions (rt_material_enable_regions): cell x lies in region cell_region[x] and
  // takes that region's row of the tables; then sigma, sigma_all and the launchers' scalar
  // rho_cv are unused.  nullptr: one medium (the kernels' uniform forms, untouched)
  const int *cell_region;       // [N]
  const double *rsigma;         // [nregions][Gl] rho kappa of the handle's groups
  const double *rsigma_all;     // [nregions][G] rho kappa of every group
  const double *rho_cv_r;       // [nregions] heat capacity
  // the opacity law (rt_material_set_opacity_law; region handles only): sigma_g(x) = rsigma f(x),
  // f = clamp((T / law_Tref)^(-law_n), law_min, law_max) per cell.  nullptr: off (the kernels'
  // other forms, untouched)
  double *fscale;               // [N] f(x): read as f_old, written as f_new by the Planck pass
  double *fratio;               // [N] f_old / f_new of that pass (scratch of the pass)
  const double *law_n;          // [nregions] exponent
  const double *law_Tref;       // [nregions] reference temperature
  double law_min, law_max;
  // the opacity table (rt_material_set_opacity_table; excludes the law): sigma_g(x) = rsigma
  // f_g(x), ln f linear in ln T between the nodes and constant outside.  ftab nullptr: off
  double *ftab;                 // [N][G] f_g(x) of ALL groups, cell-major (opacity_table_kernel)
  double *gratio;               // [Gl][N] f_old / f_new of the handle's groups (like owed)
  const double *tab_T;          // [tab_nT] the nodes, increasing
  const double *tab_r;          // [tab_nT - 1] 1 / log(T_{j+1} / T_j)
  const double *tab_lnf;        // [nregions][tab_nT][G] ln f at the nodes
  int tab_nT;
  // the energy table (rt_material_set_energy_table; any coupled handle, a plain one with region
  // 0's row): the material's internal energy e_k(T) in place of rho_cv T, ln e linear in ln T
  // between the nodes and above the last, e = c_0 T below the first (material_energy, kernels.hip).
  // eos_T nullptr: off (the update's forms with the constant rho_cv, untouched)
  const double *eos_T;          // [eos_nT] the nodes, increasing
  const double *eos_r;          // [eos_nT - 1] 1 / log(T_{j+1} / T_j)
  const double *eos_lne;        // [nregions][eos_nT] ln e at the nodes
  const double *eos_s;          // [nregions][eos_nT - 1] (ln e_{j+1} - ln e_j) r_j > 0, the bracket's exponent
  const double *eos_c0;         // [nregions] e_0 / T_0, the heat capacity below the first node
  int eos_nT;
};
// B[N][Gl] = B_g(T(x)) and the fields above
hipError_t launch_planck_cells(const PlanckCells &pc, const double *T, double *B, hipStream_t st);
// the correction's share of the fused angular sums (SegArgs.phi) after a
// coupled pass with segments started from X = 0 (T = 1; each segment walked as
// sub-segments, enough to fill the chip)
// nsub sub-segments of Lsub cells per segment (Lsub a multiple of 16), each started from
// pow^j applied to the segment's correction state, pow = A^Lsub (launch_correction_power)
hipError_t launch_phi_correction(int scheme, const SegArgs &a, int nsub, int Lsub, const double *pow, hipStream_t st);
// pow[half][K (K + 1) / 2][Lpad] = A^L, A the map's linear X -> X' block (lower triangular)
// BE, CN: the correction's share in closed form (lanes over cells, H <= 32 lines per group-half)
bool phi_correction_geo_supported(int scheme, const SegArgs &a);
hipError_t launch_phi_correction_geo(int scheme, const SegArgs &a, hipStream_t st);
// BDF2: the correction's share by tabulated rows b A^j (lanes over cells, H <= 32);
// launch_corr_rows fills the table (corr_rows_doubles) once per handle from the map
bool phi_correction_rows_supported(int scheme, const SegArgs &a);
size_t corr_rows_doubles(int scheme, int Lpad);
hipError_t launch_corr_rows(int scheme, const double *map, double *rows, int Lpad, hipStream_t st);
hipError_t launch_phi_correction_rows(int scheme, const SegArgs &a, const double *rows, hipStream_t st);
hipError_t launch_correction_power(int scheme, const double *map, double *pow, int L, int Lpad, hipStream_t st);
// q[x] = sum_g sigma_g (phi_g(x) - W B_g(x)) over the handle's groups, phi the
// sum of nparts [N][Gl] arrays at phi (the fused parts, or one full phi); q[N + x] = bpart[x].
// cell_region: sigma is [nregions][Gl] and cell x takes the row cell_region[x]
// fscale (region form only): the opacity law's f(x) scales both q and b of cell x
// fstride > 0 (the opacity table): f_g(x) = fscale[x fstride + g] inside the sum of q; bpart
// already holds sum sigma_g f_g dB_g/dT (the Planck pass's table form)
hipError_t launch_material_q(const double *phi, int nparts, const double *B, const double *sigma, double W,
                             const double *bpart, double *q, int Gl, int N, hipStream_t st,
                             const int *cell_region = nullptr, const double *fscale = nullptr, int fstride = 0);
// from qb = [q, b] summed over all groups: dT = dt q / (rho_cv + dt W b), T(x) += dT, dTlast = dT
// T += dt q / (rho_cv + dt W b), or the root of the full emission where dT > T / 4 (its owed
// emission added there, dT 0): rt_oracle.c orc_material_update.  pc.cell_region set: rho_cv is
// the cell's region's (pc.rho_cv_r) and the argument unused
// pc.eos_T set (the energy table): the EOS forms -- T' the root of e(T') - e(T) + dt W b (T' - T) = dt q,
// or of e(T') - e(T) = dt (A - W S(T')) where T' - T > T / 4; rho_cv and pc.rho_cv_r are then unused
hipError_t launch_material_update(const PlanckCells &pc, double *T, const double *qb, double *dTlast, double dt,
                                  double rho_cv, double W, int N, hipStream_t st);
// e[x], cv[x] = the material's internal energy and heat capacity at T[x] (rt_get_material_energy,
// rt_get_heat_capacity), by the update's own material_energy(); without the table rho_cv(x) T[x] and
// rho_cv(x) (rho_cv: the plain handle's, as for launch_material_update).  Either output may be nullptr
hipError_t launch_material_energy(const PlanckCells &pc, const double *T, double rho_cv, double *e, double *cv, int N,
                                  hipStream_t st);
// E[x] = scale sum_gl sigma[gl] ((Beff - B) + owed[gl][x]) (rt_get_material_transit);
// cell_region: as for launch_material_q
hipError_t launch_material_transit(const double *B, const double *Beff, const double *owed, const double *sigma,
                                   double scale, double *E, int Gl, int N, hipStream_t st,
                                   const int *cell_region = nullptr, const double *fscale = nullptr,
                                   int fstride = 0);  // fstride: as for launch_material_q
// the opacity law set, changed or cleared between steps: f_new from T (pc.fscale then holds it;
// pc.law_n == nullptr: 1), and the emission in transit (Beff - B) + owed of every cell and group
// times f_old / f_new, paid again as p = max(owed, -B): Beff = B + p, owed -= p.  f_old: pc.fscale,
// or 1 where had_law is 0
// had_law names what was in force: 0 nothing, 1 the law (pc.fscale), 2 the table (pc.ftab, per
// group).  What comes into force is pc's: the table where pc.tab_lnf is set (f_g from T to pc.ftab
// by opacity_table_kernel, per-group ratios), else the law where pc.law_n is set, else nothing
enum { kOpacityNone = 0, kOpacityLaw = 1, kOpacityTable = 2 };
hipError_t launch_opacity_rescale(const PlanckCells &pc, const double *T, int had_law, hipStream_t st);

}  // namespace rtamd

// wave_cost.hpp -- the measured tick costs of the short-line wavefront (kernels_wave.hip),
// shared by wavefront_plan and the host-only region plan (regions.cpp).  Plain C++.
//
// Tick costs (ns, medians) from tools/chain_plan.py on chain_kernel / wavefront_kernel
// (round 5, profiles/r05d_chain_plan.jsonl: 1000 BDF2 steps, 8 lines, every feasible C at
// N = 16 .. 2048, vacuum and reflective; * = interpolated, no length measured there; the
// reflective rows re-measured after the head cell took its own map, r05p_chain_plan_refl.jsonl:
// N = 32 .. 2048 in steps filling each wave count).  Rows C = 1, 2, 4, 8; columns 1..8 waves.
#pragma once

namespace rtamd {

constexpr int kWaveCostWaves = 8;
inline constexpr float kTickVacuum[4][kWaveCostWaves] = {
    {79, 141, 166, 185, 225, 248, 259, 272},     // C = 1
    {126, 194, 217, 238, 306, 343, 356, 368},    // C = 2 (7 waves *)
    {220, 300, 323, 341, 441, 541, 560, 579},    // C = 4 (5, 7 waves *)
    {410, 500, 532, 555, 800, 880, 910, 943}};   // C = 8 (5-8 waves *: only C = 8 fits there)
inline constexpr float kTickReflective[4][kWaveCostWaves] = {  // N a multiple of C
    {83, 156, 173, 191, 230, 255, 266, 278},     // C = 1 (round 5 before the head map: 201 .. 354)
    {131, 203, 222, 244, 321, 349, 363, 388},    // C = 2
    {227, 307, 330, 351, 515, 551, 570, 587},    // C = 4
    {421, 529, 559, 579, 927, 977, 1001, 1046}};  // C = 8 (5-8 waves: the head's redo, r05t_chain_plan_c8)

}  // namespace rtamd

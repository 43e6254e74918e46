// regions.hpp -- host logic of the multi-region slabs (include/rtsn.h rt_regions_*,
// rt_create_regions): which chain a slab of piecewise-constant regions takes, the per-lane and
// per-cell region tables the kernels index, the segments of a long line (plan_segments), and
// the .prm's region table.  Plain C++, no HIP:
// built into librtsn with the host objects and alone (tools/regions_sanitize.cpp).
//
// A chain lane of the short-line wavefront (kernels_wave.hip) holds C consecutive cells and one
// cell map, so its cells must lie in one region: C is admissible when it divides every
// region's first cell and N.  Among the admissible C whose chain fits the wave cap the plan
// takes the least (nsteps + lanes - 1) x tick cost of wave_cost.hpp: nsteps = 1000 as
// wavefront_plan does, or 1 for a material-coupled handle, whose launches are single steps.
#pragma once

#include <vector>

#include "../../include/rtsn.h"

namespace rtamd::regions {

struct Plan {
  int C = 0, waves = 0, lanes = 0;  // C = 0: no admissible chain fits
};

// first_cell[0 .. R]: region k holds the cells [first_cell[k], first_cell[k + 1]); false when a
// region is empty or the argument is NULL
bool first_cells(const rt_region *r, int R, std::vector<int> &first_cell);
// bit ci set: C = 1 << ci (1, 2, 4, 8) divides every entry of first_cell
unsigned admissible_mask(const std::vector<int> &first_cell);
// want_C: a caller's cells per lane, taken when admissible and fitting; else the cost table's
// max_C: the most cells per lane the kernel has (4 for the law form of the chain, which holds each
// cell's own line constants; want_C beyond it counts as inadmissible)
Plan plan(const std::vector<int> &first_cell, bool reflective, int max_waves, int want_C = 0,
          long long nsteps = 1000, int max_C = 8);
// cell_region[c] for c < N
std::vector<int> cell_table(const std::vector<int> &first_cell);
// lane_region[half][lanes] at C cells per lane: half 1 (mu > 0) lane j holds the physical
// cells [j C, (j + 1) C), half 0 (mu < 0) lane j the cells N - 1 - (j C + c): the mirror image
std::vector<int> lane_table(const std::vector<int> &first_cell, int C);

// Long lines (the region form of the pipelined segment pass, kernels.hip): a segment holds one
// cell map, so it must lie in one region, and its length is a multiple of the 16-cell register
// tile -- admissible when 16 divides every region's first cell and N.
constexpr int kSegmentUnit = 16;
bool segments_admissible(const std::vector<int> &first_cell);
// target_cells rounded up to a multiple of 16, at least 16
int segment_target(long long target_cells);
// The cutting rule: a region of n cells becomes k = ceil(n / target) segments, its n / 16 units
// dealt out as evenly as possible, the longer segments first.  seg_first[0 .. Sg] (physical
// cells, left to right) and seg_region[0 .. Sg - 1]; returns Sg (0: not admissible)
int plan_segments(const std::vector<int> &first_cell, long long target_cells, std::vector<int> &seg_first,
                  std::vector<int> &seg_region);
// The kernel's tables in each half's upwind numbering: [2][Sg + 1] first cells, then [2][Sg]
// regions; half 1 (mu > 0) as planned, half 0 (mu < 0) the mirror image: upwind segment s
// covers the physical cells N - seg_first[Sg - s] .. N - seg_first[Sg - 1 - s] - 1
std::vector<int> segment_tables(const std::vector<int> &seg_first, const std::vector<int> &seg_region);

}  // namespace rtamd::regions

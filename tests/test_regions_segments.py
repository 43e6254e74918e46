"""Multi-region slabs on long lines, host side (include/rtsn.h rt_regions_plan_segments;
csrc/regions.cpp): the segment planner against a restatement of its cutting rule on seeded
random layouts, its refusals, and the planner under AddressSanitizer + UBSan
(tools/regions_segments_sanitize.cpp, its own main).  No GPU: the host-only entry points load
without one.
"""
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO


def _regions(cells):
    return [dict(cells=int(c), width=1.0 + 0.5 * k, rho=1.0, kappa_grey=1.0, T=1.0) for k, c in enumerate(cells)]


def cutting_rule(cells, target):
    """target rounded up to a multiple of 16, at least 16.  A region of n cells becomes
    k = ceil(n / target) segments; its n / 16 units are dealt out so that the first
    (n / 16) mod k segments get one unit more.  Returns the segment lengths per region."""
    t = max(16, -(-int(target) // 16) * 16)
    out = []
    for n in cells:
        k, units = -(-n // t), n // 16
        out.append([16 * (units // k + (1 if j < units % k else 0)) for j in range(k)])
    return out


def test_worked_example(rtsn_mod):
    """272 cells at target 64: 64, 64, 48, 48, 48."""
    assert cutting_rule([272], 64) == [[64, 64, 48, 48, 48]]
    got = rtsn_mod.regions_plan_segments(_regions([272]), 64)
    assert got == {"segments": 5, "first_cell": [0, 64, 128, 176, 224, 272], "segment_region": [0] * 5}


@pytest.mark.parametrize("seed", range(4))
def test_planner_rule(rtsn_mod, seed):
    """50 random layouts per seed: 1 to 5 regions of 16 U(1, 40) cells, targets 16 to 256 (not
    all multiples of 16).  The planner's tables equal the rule's; every segment lies in one
    region, is a multiple of 16 cells long and no longer than the rounded target; the segments
    tile [0, N); segment_region agrees with rt_get_regions' convention (region k holds the
    cells [first_cell[k], first_cell[k + 1]) of the cumulative cell counts)."""
    rng = np.random.default_rng(5200 + seed)
    for _ in range(50):
        cells = [16 * int(rng.integers(1, 41)) for _ in range(int(rng.integers(1, 6)))]
        target = int(rng.integers(16, 257))
        got = rtsn_mod.regions_plan_segments(_regions(cells), target)
        want = cutting_rule(cells, target)
        lengths = [n for per in want for n in per]
        Sg, first, reg = got["segments"], np.array(got["first_cell"]), np.array(got["segment_region"])
        assert Sg == len(lengths) == len(reg) == len(first) - 1, (cells, target)
        assert list(np.diff(first)) == lengths, (cells, target)
        assert list(reg) == [k for k, per in enumerate(want) for _ in per], (cells, target)
        edges = np.concatenate([[0], np.cumsum(cells)])  # rt_get_regions' first_cell
        N = int(edges[-1])
        assert first[0] == 0 and first[-1] == N and (np.diff(first) > 0).all()
        assert (first % 16 == 0).all() and (np.diff(first) <= -(-target // 16) * 16).all()
        cell_region = np.repeat(np.arange(len(cells)), cells)
        for s in range(Sg):
            assert (cell_region[first[s]:first[s + 1]] == reg[s]).all(), (cells, target, s)
            assert edges[reg[s]] <= first[s] and first[s + 1] <= edges[reg[s] + 1]


def test_planner_target_rounding(rtsn_mod):
    """The target is rounded up to a multiple of 16 and is at least 16."""
    reg = _regions([160, 48])
    assert rtsn_mod.regions_plan_segments(reg, 0) == rtsn_mod.regions_plan_segments(reg, 16)
    assert rtsn_mod.regions_plan_segments(reg, -7)["segments"] == 13
    assert rtsn_mod.regions_plan_segments(reg, 49) == rtsn_mod.regions_plan_segments(reg, 64)
    assert rtsn_mod.regions_plan_segments(reg, 64)["first_cell"] == [0, 64, 112, 160, 208]
    assert rtsn_mod.regions_plan_segments(reg, 10 ** 9)["first_cell"] == [0, 160, 208]


def test_planner_refusals(rtsn_mod):
    """RT_ERR_PARAM (3): an edge or an N that is not a multiple of 16, and cells <= 0."""
    for cells in ((100, 220), (96, 100), (8, 8), (5, 508), (16, 0), (16, -16)):
        with pytest.raises(rtsn_mod.RtError) as e:
            rtsn_mod.regions_plan_segments(_regions(cells), 64)
        assert e.value.status == 3, cells
    with pytest.raises(rtsn_mod.RtError) as e:
        rtsn_mod.regions_plan_segments([dict(cells=16, width=0.0, rho=1.0, kappa_grey=1.0, T=1.0)], 64)
    assert e.value.status == 3


def test_planner_under_sanitizers(tmp_path):
    """csrc/regions.cpp built with AddressSanitizer + UBSan and run by
    tools/regions_segments_sanitize.cpp (its own main, CPU only): the planner and the kernel's
    mirrored tables on exactly-sized buffers for seeded random layouts."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    csrc = REPO / "radiative-transfer_amd" / "csrc"
    exe = tmp_path / "regions_segments_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", "-I", str(REPO / "include"), "-I", str(csrc),
                    str(REPO / "tools" / "regions_segments_sanitize.cpp"), str(csrc / "regions.cpp"),
                    str(csrc / "prm.cpp"), "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout

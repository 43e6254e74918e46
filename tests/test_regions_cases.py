"""The random multi-region cases, CPU side (tests/regions_cases.py draws them,
tests/test_regions_random_gpu.py runs them on the GPU).

* the seeds the GPU tests run reach every kernel form of the region chains -- asserted from the
  draws and the plan rule (test_regions_gpu.region_plan, regions_material_ref.plan_rule), a
  condition on the generator;
* the references' PER-REGION tables are pinned to the C oracle before the GPU is compared with
  them: one medium written three ways (table kappa_g with rho, table 2 kappa_g with rho / 2,
  None with kappa_grey) must give RegionReference = OracleSolver on the uniform slab (1e-12
  per group) and RegionMaterialReference = OracleSolver.material_* (test_material_gpu.compare);
* RegionMaterialReference = OracleSolver.material_* at 40 and 70 groups (past one 32-group tile
  and one round of 64 lanes of the region kernels), with cells on the full-emission path.
"""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

import regions_cases as rc
from parity import per_group_rel
from regions_material_ref import RegionMaterialReference, plan_rule
from test_material import params, t_profile
from test_material_gpu import compare
from test_regions_gpu import TICK_REFLECTIVE, TICK_VACUUM, RegionReference, region_plan
from test_regions_material import _pin


def material_plan(cells, reflective, want):
    """(C, waves) of a coupled region handle with `want` cells per lane set (admissible by the draw)."""
    ok = rc.admissible(cells, reflective)
    if want in ok:
        return want, ok[want]
    return plan_rule(cells, reflective, 8, 1, TICK_VACUUM, TICK_REFLECTIVE)[:2]


def region_forms():
    """The forms the region seeds reach, each with the seeds that reach it."""
    forms = Counter()
    for seed in rc.REGION_SEEDS:
        c = rc.region_case(seed)
        p, cells, R = c["p"], c["cells"], len(c["cells"])
        refl = p["bc_left"] == 2
        C, w = region_plan(cells, refl, c["wave_cap"] or 8, c["want"])
        assert C in (1, 2, 4, 8) and 1 <= w <= (c["wave_cap"] or 8), (seed, C, w)
        assert all(n % c["C0"] == 0 for n in cells) and sum(cells) == p["N"]
        assert p["N"] * c["steps"] * (4 if p["ts_method"] == 3 else 1) <= rc.WORK_CAP or p["N"] == c["C0"]
        found = [f"C={C}", "1 wave" if w == 1 else ("2-4 waves" if w <= 4 else "5-8 waves"), f"ts={p['ts_method']}"]
        found += [f"opacity {k}" for k in set(c["kinds"])]
        if refl and C == 8 and w >= 5:
            found.append("reflective C=8 on >= 5 waves")
        if refl and C in (2, 4):
            found.append("reflective C in {2,4}")
        if refl and C == 1 and w >= 2:
            found.append("reflective C=1 on >= 2 waves")
        if R >= 2:
            found.append(f"bc {(p['bc_left'], p['bc_right'])} with R >= 2")
        if len(set(c["kinds"])) > 1:
            found.append("mixed opacity kinds")
        if R in (1, 6):
            found.append(f"R={R}")
        if R >= 2 and min(cells) == c["C0"]:
            found.append("a region of C0 cells")
        edges = set(int(e) // C for e in np.cumsum(cells)[:-1])
        if edges & set(rc.wave_edge_units(p["N"] // C, refl)):
            found.append("an edge on a wave edge")
        if p["N"] == c["C0"]:
            found.append("N = C0")
        if c["chunks"]:
            found.append("chunked")
        if c["ends_factor"] is not None:
            found.append("random initial state")
        if p["use_correction"] and p["V"] == 5.994:
            found.append("correction V=5.994")
        forms.update(found)
    return forms


REGION_FORMS = {f"C={C}": 1 for C in (1, 2, 4, 8)}
REGION_FORMS.update({"1 wave": 1, "2-4 waves": 1, "5-8 waves": 1, "reflective C=8 on >= 5 waves": 3,
                     "reflective C in {2,4}": 3, "reflective C=1 on >= 2 waves": 1, "ts=1": 1, "ts=2": 1, "ts=3": 1,
                     "mixed opacity kinds": 1, "R=1": 1, "R=6": 1, "a region of C0 cells": 1,
                     "an edge on a wave edge": 1, "N = C0": 1, "chunked": 1, "random initial state": 1,
                     "correction V=5.994": 1})
REGION_FORMS.update({f"bc {bc} with R >= 2": 1 for bc in rc.BC_PAIRS})
REGION_FORMS.update({f"opacity {k}": 1 for k in rc.OPACITY_KINDS})


def test_region_cases_cover_the_kernel_forms():
    forms = region_forms()
    print({k: forms[k] for k in REGION_FORMS})
    missing = {k: (forms[k], n) for k, n in REGION_FORMS.items() if forms[k] < n}
    assert not missing, missing
    mat = Counter()
    for seed in rc.MATERIAL_SEEDS:
        c = rc.region_material_case(seed)
        C, w = material_plan(c["cells"], c["p"]["bc_left"] == 2, c["want"])
        assert C == c["want"] and 1 <= w <= 8 and sum(c["cells"]) == c["p"]["N"] <= 600
        mat.update([f"ts={c['p']['ts_method']}", f"C={C}"] + [f"opacity {k}" for k in set(c["kinds"])])
        mat.update(["shard"] if c["shard"] != (0, 0) else [])
        mat.update(["per-cell profile"] if c["T_cells"] is not None else [])
    print(dict(mat))
    for k in ("ts=1", "ts=2", "ts=3", "shard", "opacity own_table", "opacity grey", "per-cell profile"):
        assert mat[k] > 0, k


def test_material_cases_stay_physical(oracle_mod):
    """A condition on the generator's stream, as the coverage is: the reference's T stays finite
    and above zero on every material seed (CN and BDF2 can ring phi, and with it T, below zero
    from a state far from equilibrium; such a draw has no physical state to compare)."""
    for seed in rc.MATERIAL_SEEDS:
        c = rc.region_material_case(seed)
        ref = RegionMaterialReference(oracle_mod, c["p"], c["regions"], c["rho_cv"], c["T_cells"], *c["shard"])
        ref.material_step(c["steps"])
        T = ref.temperature()
        assert np.isfinite(T).all() and (T > 0).all() and np.isfinite(ref.ends()).all(), seed


def test_cases_are_reproducible():
    a, b = rc.region_case(3), rc.region_case(3)
    assert a["cells"] == b["cells"] and np.array_equal(a["p"]["psi_source"], b["p"]["psi_source"])
    assert all(np.array_equal(x["group_kappa"], y["group_kappa"]) for x, y in zip(a["regions"], b["regions"]))
    own = [r["group_kappa"] for s in rc.REGION_SEEDS for c in [rc.region_case(s)]
           for r, k in zip(c["regions"], c["kinds"]) if k == "own_table"]
    assert all(not np.array_equal(x, y) for x, y in zip(own[:-1], own[1:]))  # a different array per region


@pytest.mark.parametrize("ts", [1, 2, 3])
@pytest.mark.parametrize("bc", [(0, 0), (2, 1)])
def test_region_reference_uses_each_regions_own_opacity(oracle_mod, ts, bc):
    """The three regions are one medium (rho kappa_g bitwise equal, V = 0): RegionReference on
    them against OracleSolver on the uniform slab, 1e-12 per group after 5 steps from a random
    state; a reference that read region 0's table or kappa_grey for every region would differ in
    the first digit."""
    lo, hi = 40, 50
    p, regions = rc.three_ways(ts, bc)
    sig = [r["rho"] * (r["group_kappa"] if r["group_kappa"] is not None else np.full(p["G"], r["kappa_grey"]))
           for r in regions]
    assert np.array_equal(sig[0], sig[1]) and np.array_equal(sig[0], sig[2])
    ref = RegionReference(oracle_mod, p, regions, g_lo=lo, g_hi=hi)
    for t in ref.tables:
        assert np.array_equal(t["sigma"], ref.tables[0]["sigma"])
    orc = oracle_mod.OracleSolver(dict(p, max_timesteps=5), g_lo=lo, g_hi=hi)
    B = orc.groups()["B"][lo:hi]
    ends0 = B[None, :, None, None] * np.random.default_rng(7 + ts).uniform(0.5, 1.5, size=(p["M"], hi - lo, p["N"], 2))
    ref.set_ends(ends0)
    orc.set_ends(ends0)
    for _ in range(5):
        ref.step()
    orc.solve()
    err = {"ends": per_group_rel(ref.ends(), orc.ends(), 1), "moved": per_group_rel(ends0, orc.ends(), 1)}
    print(err)
    assert err["ends"] <= 1e-12 and err["moved"] > 1e-3


@pytest.mark.parametrize("ts,dt", [(1, 1e-3), (3, 1e-4)])
def test_region_material_reference_uses_each_regions_own_opacity(oracle_mod, ts, dt):
    """The same three regions coupled: RegionMaterialReference against OracleSolver.material_*
    on the uniform slab through test_material_gpu.compare (T 1e-12, fields 1e-10)."""
    p, regions = rc.three_ways_material(ts, (2, 1), dt)
    T0 = t_profile(p["N"])
    orc = oracle_mod.OracleSolver(p)
    orc.material_enable(5.0, T0)
    ref = RegionMaterialReference(oracle_mod, p, regions, [5.0] * 3, T0)
    for _ in range(4):
        orc.material_step(1)
        ref.material_step(1)
    print(compare(ref, orc))


@pytest.mark.parametrize("ts,dt", [(1, 1e-3), (3, 1e-4)])
@pytest.mark.parametrize("G", [40, 70])
def test_material_reference_equals_oracle_past_64_groups(oracle_mod, G, ts, dt):
    """test_regions_material._pin at 40 and 70 groups on N = 64 with a cold block of 8 cells, so
    a few cells solve the full emission over all G groups."""
    p = params(oracle_mod, ts=ts, dt=dt, M=6, G=G, N=64, bc_left=2, bc_right=1)
    p["psi_source"] = np.linspace(0.5, 2.0, p["M"] * G).reshape(p["M"], G)
    T0 = t_profile(64)
    T0[12:20] = 0.05
    ref, _ = _pin(oracle_mod, p, 0.5, T0, 3, cuts=(24, 8, 32))
    assert ref.newton_cells > 0

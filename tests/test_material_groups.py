"""Material coupling at 31-128 groups per handle, CPU side: every case of
tests/test_material_groups_gpu.py on two fp64 CPU evaluations -- the C oracle (orc_material_*)
and the numpy restatement tests/regions_material_ref.py with one region -- under the GPU test's
own metric, to a QUARTER of its tolerances.  This is the check that the cases' inputs are well
conditioned and that the reference side alone stays inside the bounds: a case that misses gets
different inputs, never a wider bound.

Also pinned here, because the metric of part B rests on it: the grey remainder group
B_{G-1} = a c T^4 - (groups 0..G-2 as one integral) moves by up to 64 eps a c T^4 when T moves by
one ulp (the cancellation's rounding, whatever the remainder's size).  On the benchmark's grid
(1e-3..30 keV) the remainder is < 1e-8 of a c T^4 at the coupled legs' temperatures, so one ulp of
T is ~1e-8..1e-7 of the group -- far above compare's 1e-10 between ANY two evaluations; on the
coupling tests' grid (0.1..10 keV) it is >= 1e-6 and the group is measured like every other.
"""
from __future__ import annotations

import numpy as np
import pytest

import material_group_cases as mc
from test_material_gpu import compare, grey

TOL_T, TOL_FIELD = 0.25 * 1e-12, 0.25 * 1e-10  # a quarter of compare's


def _slow(c):  # the numpy reference's bisection over 128 groups per cell, or 4128-cell lines
    return c["start"] == "newton" or c["N"] > 1000


def _param(c):
    return pytest.param(c, id=c["id"], marks=[pytest.mark.slow] if _slow(c) else [])


def _within_quarter(err):
    assert err["T"] <= TOL_T, err
    for k in ("psi", "ends", "phi", "B", "Beff", "transit"):
        assert err[k] <= TOL_FIELD, err


@pytest.mark.parametrize("c", [_param(c) for c in mc.CASES])
def test_cpu_pair_agrees(oracle_mod, c):
    p, rho_cv, T0 = mc.build(oracle_mod, c)
    orcs = mc.oracle_run(oracle_mod, c)
    mc.check_start_premise(oracle_mod, c)  # (from the run's first update)
    refs = [mc.make_reference(oracle_mod, p, rho_cv, T0, lo, hi) for lo, hi in c["shards"]]
    mc.step_coupled(refs, c["steps"])
    for r, o in zip(refs, orcs):
        err = compare(r, o, field_floor=c["floor"])
        print(c["part"], c["id"], err)
        _within_quarter(err)
    if c["start"] == "newton":  # every cell solved the full emission in the first update
        assert all(r.newton_cells >= p["N"] for r in refs), [r.newton_cells for r in refs]
    if c["floor"]:
        mc.check_floor_conditions(orcs)
        mc.check_floor_conditions(refs)
    else:  # grid A, no floor: the remainder group's field is no rounding remainder of a c T^4
        last = orcs[-1]
        assert last.g_lo + last.Gl == last.G
        T_all = np.concatenate([T0, last.temperature()])
        acT4 = max(grey(t) for t in T_all)
        assert np.abs(last.psi()[:, -1]).max() >= 1e-6 * acT4
        if c["start"] == "warm":  # ... and neither is its emission, at any T the case reaches
            # (a Newton start's cells sit below 0.45 keV, where the remainder above ~8.6 keV is
            # a rounding remainder; their group-127 field is the 1 keV radiation's, and B, Beff
            # are measured against planck_rel's floor as ever)
            e = last.groups()["e_edge"]
            assert T_all.min() >= 0.65  # (the share grows with T from there: test_remainder_share_on_both_grids)
            share = [oracle_mod.planck_cell(t, e, c["G"] - 1) / grey(t) for t in (T_all.min(), T_all.max())]
            assert min(share) >= 1e-6, share


@pytest.mark.parametrize("c", mc.QB_CASES, ids=[c["id"] for c in mc.QB_CASES])
def test_cpu_pair_exchange_terms(oracle_mod, c):
    """[q, b] of the first sweep, the pair within a quarter of the GPU test's bounds."""
    p, rho_cv, T0 = mc.build(oracle_mod, c)
    N = p["N"]
    orc = mc.make_oracle(oracle_mod, p, rho_cv, T0, 0, 0)
    want = orc.material_sweep()
    got = mc.make_reference(oracle_mod, p, rho_cv, T0, 0, 0).material_sweep()
    assert (want[N:] > 0).all()
    err_b = float(np.max(np.abs(got[N:] - want[N:]) / want[N:]))
    err_q = float(np.max(np.abs(got[:N] - want[:N])) / mc.q_bound(orc))
    print("A6", c["id"], {"b": err_b, "q_over_bound_scale": err_q})
    assert err_b <= 0.25 * 1e-12 and err_q <= 0.25 * 1e-10, (err_b, err_q)


@pytest.mark.parametrize("ts,bc_left", mc.REGION_CASES)
def test_cpu_pair_region_media(oracle_mod, ts, bc_left):
    """The region case's three media, each as a uniform slab with its own table, heat capacity
    and cell width: the oracle (which has no regions) against the reference the GPU test uses."""
    p, regions, rho_cv, T0 = mc.region_case(oracle_mod, ts, bc_left)
    assert [r["cells"] for r in regions] == list(mc.REGION_CELLS) and p["G"] == mc.REGION_G
    for r, rc in zip(regions, rho_cv):
        dx = r["width"] / r["cells"]
        q = dict(p, X=dx * p["N"], dx=dx, group_kappa=r["group_kappa"], have_group_kappa=1)
        orc = mc.make_oracle(oracle_mod, q, rc, T0, 0, 0)
        ref = mc.make_reference(oracle_mod, q, rc, T0, 0, 0)
        mc.step_coupled([orc], 3)
        mc.step_coupled([ref], 3)
        assert (orc.temperature() > 0).all()
        _within_quarter(compare(ref, orc))


# ---------------------------------------------------------------------------
# the reason for the field floor
# ---------------------------------------------------------------------------
def _edges(oracle_mod, grid, G):
    p, rho_cv, T0 = mc.build(oracle_mod, mc.case("edges", "-", G, 2, 4, grid=grid))
    return oracle_mod.OracleSolver(p).groups()["e_edge"]


@pytest.mark.parametrize("grid", ["A", "bench"])
def test_remainder_group_cancellation_model(oracle_mod, grid):
    """|B_{G-1}(T+) - B_{G-1}(T)| <= 64 eps a c T^4 for T+ = nextafter(T): the remainder moves by
    the rounding of a c T^4 - (rest), on either grid; what differs is the remainder's own size."""
    e = _edges(oracle_mod, grid, 128)
    eps = np.finfo(np.float64).eps
    worst_abs, worst_rel = 0.0, 0.0
    for T in np.geomspace(0.05, 1.5, 24):
        Tp = np.nextafter(T, np.inf)
        b0, b1 = oracle_mod.planck_cell(T, e, 127), oracle_mod.planck_cell(Tp, e, 127)
        d0, d1 = oracle_mod.planck_cell_dBdT(T, e, 127), oracle_mod.planck_cell_dBdT(Tp, e, 127)
        assert abs(b1 - b0) <= 64 * eps * grey(T), (T, b0, b1)
        worst_abs = max(worst_abs, abs(b1 - b0) / grey(T))
        if 0.7 <= T <= 1.3:
            worst_rel = max(worst_rel, abs(b1 - b0) / b0, abs(d1 - d0) / d0)
    print(grid, "one ulp of T: |dB| / a c T^4 <=", worst_abs, "; relative to the group at 0.7-1.3 keV <=", worst_rel)
    if grid == "A":
        assert worst_rel <= 1e-10  # far inside compare's tolerance: no floor needed


def test_remainder_share_on_both_grids(oracle_mod):
    """Benchmark grid: the remainder is < 1e-8 of a c T^4 from 0.2 keV (the Newton start after
    its first step) to 1 keV, 4.8e-9 at 1 keV; the Wien tail above 30 keV brings it to 1e-6 at the
    warm start's hottest cell, 1.3 keV (cooled to 1.05 keV after the three steps) -- three
    decades below the floor either way.  Grid A: >= 1e-6 at every group count and temperature a
    warm part A case can reach (0.65 keV and above, growing with T; below ~0.45 keV it is a rounding remainder here
    too -- the cold starts, whose group-127 field is the 1 keV radiation's)."""
    e = _edges(oracle_mod, "bench", 128)
    for T in (0.2, 0.5, 0.7, 1.0):
        assert oracle_mod.planck_cell(T, e, 127) / grey(T) < 1e-8, T
    assert oracle_mod.planck_cell(1.3, e, 127) / grey(1.3) < 2e-6
    for G in mc.EDGE_GROUPS + (mc.REGION_G,):
        e = _edges(oracle_mod, "A", G)
        for T in np.geomspace(0.65, 3.0, 30):
            assert oracle_mod.planck_cell(T, e, G - 1) / grey(T) >= 1e-6, (G, T)


# ---------------------------------------------------------------------------
# premises that need no GPU
# ---------------------------------------------------------------------------
def test_resampled_table_range():
    """bench.slab_params' resampling: G entries of the table in its order, from its first (1e6,
    the opaque low groups) down to below 0.14 -- every case runs thick and thin groups together."""
    for G in mc.EDGE_GROUPS + (mc.REGION_G,):
        k = mc.resampled_kappa(G)
        assert k.shape == (G,) and np.isin(k, mc.KAPPA_LLNL).all()
        assert k[0] == mc.KAPPA_LLNL[0] == k.max() == 1e6 and 0.0 < k.min() <= 0.14
    assert np.array_equal(mc.resampled_kappa(len(mc.KAPPA_LLNL)), mc.KAPPA_LLNL)


def test_case_list_covers_edges_schemes_shards():
    ids = [c["id"] for c in mc.CASES]
    assert len(set(ids)) == len(ids)
    assert {c["G"] for c in mc.CASES if c["part"] == "A1"} == set(mc.EDGE_GROUPS)
    a2 = [c for c in mc.CASES if c["part"] == "A2"]
    assert len(a2) == 2 * 3 * 4 * 2 * 2 and {c["M"] for c in a2} == {4, 16, 64, 6}
    assert {c["shards"] for c in mc.CASES if c["part"] == "A5"} == {((0, 64), (64, 128)), ((0, 65), (65, 128)),
                                                                    ((0, 33), (33, 97))}
    assert all(70 <= c["N"] <= 200 for c in mc.CASES if c["part"] in ("A1", "A4", "A5", "B"))


@pytest.mark.parametrize("c", [c for c in mc.CASES if c["start"] == "newton"],
                         ids=[c["id"] for c in mc.CASES if c["start"] == "newton"])
def test_newton_start_premise(oracle_mod, c):
    """From the oracle's first update alone: the linear dT exceeds T / 4 in every cell."""
    mc.check_start_premise(oracle_mod, c)

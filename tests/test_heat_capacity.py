"""The tabulated internal energy e(T) of the material coupling, on the CPU: the conditions the GPU
cases of tests/test_heat_capacity_gpu.py rest on, asserted on the fp64 restatement
tests/heat_capacity_ref.py alone, the rule of the table stated independently, and the entry
points' declarations.

For the shared table on (32, 48) and (16, 16) cells, BE / CN / BDF2, the three boundary pairs, and
the opacity law `marshak` once per scheme:

* in every step some cell takes the linear path and some cell the full emission, and some cell
  changes its piece of the table;
* over the six steps every bracket and the piece below the first node hold a cell; with BDF2,
  (1, 1) and `marshak` some cell exceeds the last node;
* BE: the energy residual with e(T) in the statement is at most 1e-12 of the total every step.

The table energy = c x T_grid equals the parent reference with rho_cv = c at compare's tolerances.
The argument checks of rt_material_set_energy_table need a coupled handle, so a device: they are in
the GPU file; here only the NULL handle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import heat_capacity_ref as hcr

# (layout, ts, bc, law): what tests/test_heat_capacity_gpu.py runs in segment mode
SEGMENT_CASES = [(lay, ts, bc, None) for lay in ("n80", "n32") for ts in (1, 2, 3) for bc in hcr.BCS]
LAW_CASES = [("n80", 1, (2, 1), "marshak"), ("n80", 2, (0, 0), "marshak"), ("n80", 3, (1, 1), "marshak")]


@pytest.mark.parametrize("layout,ts,bc,law", SEGMENT_CASES + LAW_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_case_conditions(oracle_mod, layout, ts, bc, law):
    r = hcr.reference_run(oracle_mod, layout, ts, bc, law=law)
    ref = r["ref"]
    assert np.isfinite(ref.ends()).all() and np.isfinite(ref.temperature()).all()
    Tg = hcr.energy_table(layout)[0]
    nT = len(Tg)
    held = set()
    for n, h in enumerate(ref.history):
        solved, linear = int(h["solved"].sum()), int((~h["solved"]).sum())
        crossed = int((h["before"] != h["after"]).sum())
        held |= set(h["before"].tolist()) | set(h["after"].tolist())
        print(layout, ts, bc, law, n, dict(solved=solved, linear=linear, crossed=crossed, resid=float(r["resid"][n]),
                                           Tmin=r["Tmin"][n], Tmax=r["Tmax"][n]))
        assert solved > 0 and linear > 0, (n, solved, linear)
        assert crossed > 0, n
    assert held >= set(range(-1, nT - 1)), held
    if (ts, bc, law) == (3, (1, 1), "marshak"):
        assert max(r["Tmax"]) > Tg[-1]
    if ts == 1:
        assert np.abs(r["resid"]).max() <= 1e-12, r["resid"]
        assert min(r["Tmin"]) > 0.0 and min(r["Bmin"]) >= 0.0


@pytest.mark.parametrize("ts", [1, 3])
def test_linear_table_is_the_constant_heat_capacity(oracle_mod, ts):
    """energy = c x T_grid against the parent reference enabled with rho_cv = c, T to 1e-12 and
    the rest to 1e-10 (test_material_gpu.compare's figures): equal to rounding, not bitwise -- the
    table's e goes through log and exp, and its roots through bisection."""
    from parity import per_group_rel
    p, regions, _, T0 = hcr.case(oracle_mod, "n80", ts, (2, 1))
    c = (5.0, 0.5)
    Tg = hcr.energy_table()[0]
    parent = hcr.HeatCapacityReference(oracle_mod, p, regions, c, T0)
    child = hcr.HeatCapacityReference(oracle_mod, p, regions, (1.0, 1.0), T0,
                                      energy_table=(Tg, np.outer(c, Tg)))
    parent.material_step(hcr.STEPS)
    child.material_step(hcr.STEPS)
    assert child.newton_cells > 0 and parent.newton_cells > 0
    T, Tw = child.temperature(), parent.temperature()
    err = float(np.max(np.abs(T - Tw) / np.abs(Tw)))
    print(ts, err)
    assert err <= 1e-12
    assert per_group_rel(child.ends(), parent.ends(), 1) <= 1e-10
    np.testing.assert_allclose(child.material_energy(), parent.material_energy(), rtol=1e-12)
    np.testing.assert_allclose(child.heat_capacity(), parent.heat_capacity(), rtol=1e-13)
    tr = parent.material_transit()
    assert np.abs(child.material_transit() - tr).max() <= 1e-10 * np.abs(tr).max()


def test_table_off_is_the_parent_bitwise(oracle_mod):
    from opacity_table_ref import OpacityTableReference
    p, regions, rho_cv, T0 = hcr.case(oracle_mod, "n32", 3, (2, 1))
    parent = OpacityTableReference(oracle_mod, p, regions, rho_cv, T0)
    child = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, energy_table=hcr.energy_table("n32"))
    child.set_energy_table(None, None)
    parent.material_step(3)
    child.material_step(3)
    for name in ("temperature", "ends", "cell_emission", "material_transit"):
        assert np.array_equal(getattr(child, name)(), getattr(parent, name)()), name
    assert np.array_equal(child.heat_capacity(), np.repeat(rho_cv, [16, 16]))
    assert np.array_equal(child.material_energy(), np.repeat(rho_cv, [16, 16]) * child.temperature())


# ---------------------------------------------------------------------------
# the rule of the table, stated independently in long double
# ---------------------------------------------------------------------------
def probe_temperatures(Tg):
    """Below the first node (one of them <= 0: rt_material_enable* admits any T_cells), on every
    node, one ulp to either side of the interior nodes, above the last node."""
    Tg = np.asarray(Tg, dtype=np.float64)
    inner = Tg[1:-1]
    return np.concatenate([[0.5 * Tg[0], -0.25 * Tg[0], 0.0], Tg, np.nextafter(inner, 0.0), np.nextafter(inner, np.inf),
                           [1.5 * Tg[-1], 40.0 * Tg[-1]]])


def probe_rule(Tg, en, T, cell_region):
    """(e, c_v) by the rule in long double: below the first node the line through the origin and
    the first node; from it on the log-log chord of the bracket, the last bracket's above the
    last node; c_v the chord's slope times e / T."""
    L = np.longdouble
    Tg, en = np.asarray(Tg, dtype=np.float64), np.asarray(en, dtype=np.float64)
    e, cv = np.empty(T.size), np.empty(T.size)
    for c, (t, k) in enumerate(zip(T, cell_region)):
        if t < Tg[0]:
            c0 = L(en[k, 0]) / L(Tg[0])
            e[c], cv[c] = c0 * L(t), c0
            continue
        j = min(int(np.searchsorted(Tg, t, side="right")) - 1, Tg.size - 2)
        slope = np.log(L(en[k, j + 1]) / L(en[k, j])) / np.log(L(Tg[j + 1]) / L(Tg[j]))
        val = L(en[k, j]) * np.exp(slope * np.log(L(t) / L(Tg[j])))
        e[c], cv[c] = val, slope * val / L(t)
    return e, cv


def test_interpolation_rule(oracle_mod):
    """The reference's e and c_v at the probe temperatures against the rule, 1e-14 relative (e = 0
    at T = 0 exactly), in fp64 and in np.longdouble; e increases along the sorted probes."""
    p, regions, rho_cv, _ = hcr.case(oracle_mod, "n32", 1, (0, 0))
    Tg, en = hcr.energy_table()
    probes = probe_temperatures(Tg)
    assert (probes <= 0).sum() == 2 and (probes > Tg[-1]).sum() == 2
    for shift in (0, 16):
        T0 = np.roll(np.resize(probes, p["N"]), shift)
        for dtype in (np.float64, np.longdouble):
            ref = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, dtype=dtype, energy_table=(Tg, en))
            e = np.asarray(ref.material_energy(), dtype=np.float64)
            cv = np.asarray(ref.heat_capacity(), dtype=np.float64)
            we, wc = probe_rule(Tg, en, T0, ref.cell_region)
            assert np.max(np.abs(e - we) / np.maximum(np.abs(we), 1e-300)) <= 1e-14
            assert np.max(np.abs(cv - wc) / wc) <= 1e-14
            assert (e[T0 == 0.0] == 0.0).all()
    for k in (0, 1):
        order = np.sort(probes)
        e, cv = probe_rule(Tg, en, order, np.full(order.size, k))
        assert (np.diff(e) >= 0).all() and (cv > 0).all()


def test_two_node_power_law(oracle_mod):
    """e ~ T^4 as a two-node table: c_v = 4 e / T ~ T^3 above T_0, the Su-Olson material."""
    p, regions, rho_cv, _ = hcr.case(oracle_mod, "n32", 1, (0, 0))
    Tg = np.array([0.05, 1.0])
    en = np.array([[2.0 * 0.05 ** 4, 2.0], [0.3 * 0.05 ** 4, 0.3]])
    T0 = np.geomspace(0.05, 7.0, p["N"])
    ref = hcr.HeatCapacityReference(oracle_mod, p, regions, rho_cv, T0, energy_table=(Tg, en))
    a = np.repeat([2.0, 0.3], 16)
    np.testing.assert_allclose(ref.material_energy(), a * T0 ** 4, rtol=1e-14)
    np.testing.assert_allclose(ref.heat_capacity(), 4.0 * a * T0 ** 3, rtol=1e-14)


def test_entry_points_declared_and_exported(rtsn_mod):
    names = rtsn_mod.exported_symbols()
    L = rtsn_mod.lib()
    for f in ("rt_material_set_energy_table", "rt_get_material_energy", "rt_get_heat_capacity"):
        assert f in names and hasattr(L, f)
    fn = L.rt_material_set_energy_table
    assert len(fn.argtypes) == 5 and fn.argtypes[2] is C.c_int and fn.argtypes[4] is C.c_int
    assert len(L.rt_get_material_energy.argtypes) == 2 and len(L.rt_get_heat_capacity.argtypes) == 2
    # without a handle (no GPU needed): RT_ERR_ARG; every other check needs a coupled handle
    a = (C.c_double * 4)(1.0, 2.0, 1.0, 2.0)
    assert fn(None, a, 2, a, 1) == 8
    assert L.rt_get_material_energy(None, a) == 8 and L.rt_get_heat_capacity(None, a) == 8
    for m in ("material_set_energy_table", "material_energy", "heat_capacity"):
        assert hasattr(rtsn_mod.Solver, m)

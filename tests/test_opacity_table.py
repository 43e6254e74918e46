"""Tabulated per-group opacities of the material coupling, on the CPU: the conditions the GPU cases
of tests/test_opacity_table_gpu.py rest on, asserted on the fp64 restatement
tests/opacity_table_ref.py alone, and the entry points' declarations.

For the table `edge` on every layout, BE / CN / BDF2 and the three boundary pairs:

* BE: the energy residual is at most 1e-12 of the total every step -- the per-group owed rescale
  by f_old,g / f_new,g is the whole argument;
* T > 0 and Beff >= 0 after every step;
* f at the start spans a decade over the cells and over the groups within one cell;
* some cell changes its bracket of the table during the 6 steps (a node is crossed);
* cells on the Newton path and cells on the linear path both occur, and no cell's dT / T lies
  within 1e-6 of the switch at 0.25, so the device and the reference take the same branch.

The clamped power law written as a table (`as_law`) equals OpacityLawReference with that law
after 6 steps to 1e-12 in T; the all-ones table is bitwise the parent with the law off; mid-run
transitions among nothing, the law and the table keep the energy sum.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import opacity_law_ref as olr
import opacity_table_ref as otr

CASES = [(lay, ts, bc) for lay in otr.LAYOUTS for ts in (1, 2, 3) for bc in otr.BCS]


@pytest.mark.parametrize("layout,ts,bc", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_case_conditions(oracle_mod, layout, ts, bc):
    r = otr.reference_run(oracle_mod, layout, "edge", ts, bc)
    ref = r["ref"]
    assert min(r["Tmin"]) > 0.0 and min(r["Bmin"]) >= 0.0
    assert np.isfinite(ref.ends()).all()
    f0 = r["f0"]
    assert f0.shape == (ref.N, ref.G)
    assert f0.max(axis=0).max() >= 10.0 * f0.min(axis=0).min()           # over the cells
    assert (f0.max(axis=0) / f0.min(axis=0)).max() >= 10.0               # ... of one group
    assert (f0.max(axis=1) / f0.min(axis=1)).max() >= 10.0               # over the groups within one cell
    crossed = int((np.stack(r["bracket"]) != r["bracket"][0]).any(axis=0).sum())
    assert crossed > 0
    assert not np.array_equal(r["f"][0], r["f"][-1])
    solved = sum(int(h["solved"].sum()) for h in ref.history)
    linear = sum(int((~h["solved"]).sum()) for h in ref.history)
    assert solved > 0 and linear > 0, (solved, linear)
    near = min(float(np.abs(h["ratio"] - 0.25).min()) for h in ref.history)
    assert near > 1e-6, near
    print(layout, ts, bc, dict(f=(float(f0.min()), float(f0.max())), crossed=crossed, solved=solved, near=near,
                               Tmin=min(r["Tmin"]), resid=float(np.abs(r["resid"]).max())))
    if ts == 1:
        assert np.abs(r["resid"]).max() <= 1e-12, r["resid"]


@pytest.mark.parametrize("ts", [1, 3])
def test_clamped_law_as_a_table(oracle_mod, ts):
    """`as_law` against OpacityLawReference with `clamped`: T after 6 steps to 1e-12, f to 1e-12."""
    bc = (2, 1)
    r = otr.reference_run(oracle_mod, "n80", "as_law", ts, bc)
    want = olr.reference_run(oracle_mod, "n80", "clamped", ts, bc)
    Tg, sc = otr.table_args("as_law", 5)
    assert Tg.size == 4 and sc.min() == 0.4 and sc.max() == 5.0
    assert np.max(np.abs(r["f0"] - want["f0"][:, None]) / want["f0"][:, None]) <= 1e-14
    T, Tw = r["ref"].temperature(), want["ref"].temperature()
    err = float(np.max(np.abs(T - Tw) / Tw))
    print(ts, err)
    assert err <= 1e-12
    assert np.max(np.abs(r["ref"].f - want["ref"].f[:, None]) / want["ref"].f[:, None]) <= 1e-12


@pytest.mark.parametrize("ts", [1, 2, 3])
def test_all_ones_table_is_the_parent_bitwise(oracle_mod, ts):
    p, regions, rho_cv, T0 = otr.case(oracle_mod, "n32", ts, (2, 1))
    parent = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0)
    child = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0, table=otr.table_args("ones", p["G"]))
    parent.material_step(4)
    child.material_step(4)
    assert child.newton_cells == parent.newton_cells > 0
    for name in ("temperature", "ends", "cell_planck", "cell_emission", "material_transit"):
        assert np.array_equal(getattr(child, name)(), getattr(parent, name)()), name
    assert np.array_equal(child.opacity_scale_groups(), np.ones((p["N"], p["G"])))


def test_interpolation_rule(oracle_mod):
    """The table's rule at probe temperatures: below, above, on every node, one ulp to either
    side of an interior node, T <= 0 and not finite; in fp64 and in np.longdouble."""
    p, regions, rho_cv, _ = otr.case(oracle_mod, "n32", 1, (0, 0))
    Tg, sc = otr.table_args("edge", p["G"])
    probes = probe_temperatures(Tg)
    N = p["N"]
    T0 = np.resize(probes, N)
    for dtype in (np.float64, np.longdouble):
        ref = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, dtype=dtype, table=(Tg, sc))
        f = np.asarray(ref._scale_table(T0.astype(dtype)), dtype=np.float64)
        want = probe_rule(Tg, sc, T0, ref.cell_region)
        assert np.max(np.abs(f - want) / want) <= 1e-14


def probe_temperatures(Tg):
    """Below the first node, above the last, exactly on each node, one ulp to either side of the
    interior nodes, and the law's 0+ cases."""
    inner = Tg[1:-1]
    return np.concatenate([[0.5 * Tg[0], 2.0 * Tg[-1]], Tg, np.nextafter(inner, 0.0), np.nextafter(inner, np.inf),
                           [0.0, -1.0, np.inf, np.nan]])


def probe_rule(Tg, sc, T, cell_region):
    """The rule stated independently, in long double: the node's value on and outside the grid
    ends, the log-log chord between."""
    L = np.longdouble
    out = np.empty((T.size, sc.shape[2]))
    for c, (t, k) in enumerate(zip(T, cell_region)):
        if not (t > 0 and np.isfinite(t)) or t < Tg[0]:
            out[c] = sc[k, 0]
        elif t >= Tg[-1]:
            out[c] = sc[k, -1]
        else:
            j = int(np.searchsorted(Tg, t, side="right")) - 1
            w = np.log(L(t) / L(Tg[j])) / np.log(L(Tg[j + 1]) / L(Tg[j]))
            out[c] = np.exp(np.log(sc[k, j].astype(L)) * (1 - w) + np.log(sc[k, j + 1].astype(L)) * w)
    return out


def test_transitions_in_mid_run_keep_the_energy(oracle_mod):
    """With emission in transit: the table set, changed, replaced by the law, the law replaced by
    the table, the table cleared -- the energy sum is the same before and after, to rounding, and
    every BE step between balances at 1e-12."""
    from test_material import net_outflow
    p, regions, rho_cv, T0 = otr.case(oracle_mod, "n80", 1, (2, 1))
    ref = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0)
    dx, rcv = ref.dx_cells, np.asarray(ref.rho_cv_cells)
    ref.material_step(3)
    assert np.abs(ref.material_transit()).max() > 0.0
    for call in transitions(p["G"]):
        e0 = olr.energy(ref, dx, rcv)
        call(ref)
        e1 = olr.energy(ref, dx, rcv)
        assert abs(e1 - e0) <= 1e-14 * abs(e1), (e0, e1)
        ref.material_step(1)
        e2 = olr.energy(ref, dx, rcv)
        resid = (e2 - e1) + p["dt"] * net_outflow(olr._RefView(ref), p)
        assert abs(resid) <= 1e-12 * abs(e2)
    assert ref.table is None and ref.law is None and np.array_equal(ref.f, np.ones(ref.N))


def transitions(G):
    """The mid-run transitions, as calls on a reference (set_table, set_law) -- the GPU test
    drives a solver and a reference through the same list."""
    edge, as_law = otr.table_args("edge", G), otr.table_args("as_law", G)
    return [lambda s: s.set_table(*edge), lambda s: s.set_table(*as_law), lambda s: s.set_law(*olr.law_args("marshak")),
            lambda s: s.set_table(*edge), lambda s: s.set_table(None, None)]


def test_group_shards_of_the_reference(oracle_mod):
    """Shards (0, 2) and (2, 5) with [q, b] summed: T equals the full reference's (the all-G table
    is indexed from g_lo)."""
    p, regions, rho_cv, T0 = otr.case(oracle_mod, "n32", 3, (2, 1))
    tab = otr.table_args("edge", p["G"])
    full = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0, table=tab)
    shards = [otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0, g_lo=lo, g_hi=hi, table=tab)
              for lo, hi in ((0, 2), (2, 5))]
    for _ in range(3):
        full.material_step(1)
        qb = sum(s.material_sweep() for s in shards)
        for s in shards:
            s.material_update(qb)
    for s in shards:
        np.testing.assert_allclose(s.temperature(), full.temperature(), rtol=1e-12)
        assert np.array_equal(s.opacity_scale_groups(), s.f[:, s.g_lo:s.g_lo + s.Gl])
        np.testing.assert_allclose(s.f, full.f, rtol=1e-11)


def test_entry_points_declared_and_exported(rtsn_mod):
    names = rtsn_mod.exported_symbols()
    L = rtsn_mod.lib()
    for f in ("rt_material_set_opacity_table", "rt_get_opacity_scale_groups"):
        assert f in names and hasattr(L, f)
    fn = L.rt_material_set_opacity_table
    assert len(fn.argtypes) == 5 and fn.argtypes[2] is C.c_int and fn.argtypes[4] is C.c_int
    assert len(L.rt_get_opacity_scale_groups.argtypes) == 2
    # without a handle (no GPU needed): RT_ERR_ARG
    a = (C.c_double * 4)(1.0, 2.0, 1.0, 1.0)
    assert fn(None, a, 2, a, 1) == 8
    assert L.rt_get_opacity_scale_groups(None, a) == 8
    assert hasattr(rtsn_mod.Solver, "material_set_opacity_table") and hasattr(rtsn_mod.Solver, "opacity_scale_groups")


# ---------------------------------------------------------------------------
# the regime family: the (16, 32, 16) slab of material_regime_cases.py against extended precision
# ---------------------------------------------------------------------------
REGIME_CFL = (1e-2, 1.0, 1e2)
# (scheme, c dt / dx): boundaries (2, 1), the hot start, stiffness 1
REGIME_POINTS = [(ts, cfl) for ts in (1, 2, 3) for cfl in REGIME_CFL]
_regime = {}


def table_regime_case(oracle_mod, pt):
    """test_opacity_law.law_regime_case with the table `edge` in the law's place: edge's rule on
    three regions, T_ref each region's own T, so f_g = 1 (1.7 at the kinked node's odd groups) at
    the region's radiation temperature.  (CoupledCase, the table's arguments)."""
    if pt in _regime:
        return _regime[pt]
    import material_regime_cases as mc
    import regime_cases as rc
    ts, cfl = pt
    cells, bc, state, stiff = mc.REGION_CELLS, (2, 1), "hot", 1.0
    N = int(sum(cells))
    p = rc.medium(oracle_mod, N, ts, cfl, bc, 0.0, mc.STEPS)
    widths = [c * d for c, d in zip(cells, rc.REGION_DX)]
    p["X"] = float(sum(widths))
    p["dx"] = p["X"] / N
    regions = [dict(cells=int(c), width=float(w), rho=1.0, kappa_grey=p["kappa_grey"], T=float(T),
                    group_kappa=s * np.array(rc.SIGMA_DX) / d)
               for c, w, s, d, T in zip(cells, widths, rc.REGION_SIGMA_DX, rc.REGION_DX, rc.REGION_T)]
    o = oracle_mod.OracleSolver(p)
    W, e = float(o.quad()[1].sum()), o.groups()["e_edge"]
    rho_cv = []
    for r in regions:
        b0 = sum(r["rho"] * r["group_kappa"][g] * oracle_mod.planck_cell_dBdT(3.0 * r["T"], e, g) for g in range(rc.G))
        rho_cv.append(p["dt"] * W * float(b0) / stiff)
    T0 = mc.start_T(state, np.repeat([r["T"] for r in regions], cells), N)
    table = otr.edge_table(rc.G, T_ref=tuple(r["T"] for r in regions))
    truth = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0, dtype=np.longdouble, table=table)
    stiff0 = np.asarray(p["dt"] * truth.W * truth.bpart / truth.rho_cv_cells, dtype=np.float64)
    truth.material_step(mc.STEPS)
    ref = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0, table=table)
    ref.material_step(mc.STEPS)
    same = all(np.array_equal(a["solved"], b["solved"]) for a, b in zip(ref.history, truth.history))
    tr = mc.coupled_readouts(truth)
    Tn = np.asarray(tr["T"], dtype=np.float64)
    w_sigma = p["dt"] * W * np.asarray(truth.sigma_cells, dtype=np.float64)
    case = mc.CoupledCase(p, rc.to_rt(p), regions, rho_cv, T0, mc.STEPS, tr, mc.coupled_readouts(ref),
                          {"slab": np.arange(N)}, mc.rounding_floor(Tn, e, 0, rc.G), w_sigma, truth.history, same,
                          stiff0)
    _regime[pt] = (case, table)
    return _regime[pt]


def _needs_extended():
    import regime_cases as rc
    return pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)


@_needs_extended()
@pytest.mark.parametrize("pt", REGIME_POINTS, ids=lambda pt: f"{pt[0]}-{pt[1]:g}")
def test_regime_reference_within_a_quarter_of_K(oracle_mod, pt):
    """Every point kept: the truth is finite with T > 0 after every step, the fp64 reference takes
    the truth's branches, its own T is within ORACLE_ERR_MAX, and -- measured as the device will
    be, against max(its own error, 16 eps) scaled by 4 -- it stays within K / 4."""
    import material_regime_cases as mc
    import regime_cases as rc
    from test_opacity_law import _Fp64
    case, _ = table_regime_case(oracle_mod, pt)
    assert case.branch_same
    T = np.asarray(case.truth["T"], dtype=np.float64)
    assert np.isfinite(T).all()
    for k, h in enumerate(case.history):
        assert float(np.asarray(h["T"], dtype=np.float64).min()) > 0, (pt, k + 1)
    errT = np.abs(np.asarray(case.oracle["T"], dtype=np.longdouble) - case.truth["T"]) / np.abs(case.truth["T"])
    assert float(errT.max()) <= rc.ORACLE_ERR_MAX
    ratios = mc.coupled_ratios(mc.coupled_readouts(_Fp64(case)), case)
    print(pt, {k: float(np.max(v)) for k, v in ratios.items()}, float(T.min()), float(T.max()))
    for k, v in ratios.items():
        assert (np.asarray(v) <= rc.K / 4).all(), (pt, k, float(np.max(v)))

"""The temperature-dependent opacity of the material coupling, on the CPU: the conditions the
GPU cases of tests/test_opacity_law_gpu.py rest on, asserted on the fp64 restatement
tests/opacity_law_ref.py alone, the entry points' declarations, and the regime family's cases
(law_regime_case: the truth in np.longdouble, the fp64 reference within K / 4 of it).

* BE: the energy residual is at most 1e-12 of the total every step (tests/test_material.py's
  bound) -- the owed rescale by f_old / f_new is the whole argument; without it the same run
  misses by a large fraction of the total;
* T > 0 and Beff >= 0 after every step; f spans at least a decade in every law case, one case
  hits both clamps; every case has cells on the Newton path and cells on the linear path; no
  cell's dT / T lies within 1e-6 of the switch at 0.25, so the device and the reference take the
  same branch;
* with exponent 0 the subclass is bitwise its parent.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import opacity_law_ref as olr
from regions_material_ref import RegionMaterialReference

CASES = [(lay, law, ts, bc) for lay, law in olr.PARITY for ts in (1, 2, 3) for bc in olr.BCS] + [olr.WIDE_CASE]


@pytest.mark.parametrize("layout,law,ts,bc", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_case_conditions(oracle_mod, layout, law, ts, bc):
    r = olr.reference_run(oracle_mod, layout, law, ts, bc)
    ref = r["ref"]
    assert min(r["Tmin"]) > 0.0 and min(r["Bmin"]) >= 0.0
    assert np.isfinite(ref.ends()).all()
    lo, hi = olr.LAWS[law]["bounds"]
    assert r["f0"].max() >= 10.0 * r["f0"].min(), (r["f0"].min(), r["f0"].max())  # (a heated slab may narrow it later)
    for f in r["f"]:
        if law != "clamped":
            assert lo < f.min() and f.max() < hi  # no clamp reached
    if law == "clamped":  # both clamps active
        assert r["f0"].min() == lo and r["f0"].max() == hi
        assert any(f.min() == lo for f in r["f"][1:]) and any(f.max() == hi for f in r["f"][1:])
    assert not np.array_equal(r["f"][0], r["f"][-1])  # the opacity does move with T
    solved = sum(int(h["solved"].sum()) for h in ref.history)
    linear = sum(int((~h["solved"]).sum()) for h in ref.history)
    assert solved > 0 and linear > 0, (solved, linear)
    near = min(float(np.abs(h["ratio"] - 0.25).min()) for h in ref.history)
    assert near > 1e-6, near
    if ts == 1:
        assert np.abs(r["resid"]).max() <= 1e-12, r["resid"]


def test_energy_needs_the_owed_rescale(oracle_mod):
    """The same BE run with the rescale taken out of _planck: the residual is a large fraction of
    the total (what the rule is for)."""
    from test_material import net_outflow

    class NoRescale(olr.OpacityLawReference):
        def _planck(self):
            if self.law is not None:
                self._apply(self._scale(self.T))
            RegionMaterialReference._planck(self)

    p, regions, rho_cv, T0 = olr.case(oracle_mod, "n80", 1, (2, 1))
    ref = NoRescale(oracle_mod, p, regions, rho_cv, T0, law=olr.law_args("marshak"))
    dx, rcv = ref.dx_cells, np.asarray(ref.rho_cv_cells)
    worst = 0.0
    for _ in range(olr.STEPS):
        e0 = olr.energy(ref, dx, rcv)
        ref.material_step(1)
        e1 = olr.energy(ref, dx, rcv)
        worst = max(worst, abs((e1 - e0) + p["dt"] * net_outflow(olr._RefView(ref), p)) / abs(e1))
    assert worst > 1e-6, worst


@pytest.mark.parametrize("ts", [1, 2, 3])
def test_exponent_zero_is_the_parent_bitwise(oracle_mod, ts):
    p, regions, rho_cv, T0 = olr.case(oracle_mod, "n32", ts, (2, 1))
    parent = RegionMaterialReference(oracle_mod, p, regions, rho_cv, T0)
    child = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0, law=olr.law_args("zero"))
    parent.material_step(4)
    child.material_step(4)
    assert child.newton_cells == parent.newton_cells > 0
    for name in ("temperature", "ends", "cell_planck", "cell_emission", "material_transit"):
        assert np.array_equal(getattr(child, name)(), getattr(parent, name)()), name
    assert np.array_equal(child.opacity_scale(), np.ones(p["N"]))


def test_law_in_mid_run_keeps_the_energy(oracle_mod):
    """set_law with emission in transit: the energy sum is the same before and after, to rounding."""
    p, regions, rho_cv, T0 = olr.case(oracle_mod, "n80", 1, (2, 1))
    ref = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0)
    dx, rcv = ref.dx_cells, np.asarray(ref.rho_cv_cells)
    ref.material_step(3)
    assert np.abs(ref.material_transit()).max() > 0.0
    for args in (olr.law_args("marshak"), olr.law_args("clamped"), (None, None, 1.0, 1.0)):
        e0 = olr.energy(ref, dx, rcv)
        ref.set_law(*args)
        e1 = olr.energy(ref, dx, rcv)
        assert abs(e1 - e0) <= 1e-14 * abs(e1), (args, e0, e1)
        ref.material_step(1)


def test_entry_points_declared_and_exported(rtsn_mod):
    names = rtsn_mod.exported_symbols()
    L = rtsn_mod.lib()
    for f in ("rt_material_set_opacity_law", "rt_get_opacity_scale"):
        assert f in names and hasattr(L, f)
    fn = L.rt_material_set_opacity_law
    assert len(fn.argtypes) == 6 and fn.argtypes[3] is C.c_int and fn.argtypes[4] is C.c_double
    # without a handle (no GPU needed): RT_ERR_ARG
    a = (C.c_double * 2)(1.0, 1.0)
    assert fn(None, a, a, 2, 1e-3, 1e3) == 8
    assert L.rt_get_opacity_scale(None, a) == 8
    assert hasattr(rtsn_mod.Solver, "material_set_opacity_law") and hasattr(rtsn_mod.Solver, "opacity_scale")


# ---------------------------------------------------------------------------
# the regime family: the (16, 32, 16) slab of material_regime_cases.py against extended precision
# ---------------------------------------------------------------------------
REGIME_CFL = (1e-2, 1.0, 1e2)  # beyond, fp64-formed constants are known to lose digits
REGIME_EXPONENTS = (3.0, -1.0)
REGIME_BOUNDS = (1e-2, 1e2)
# (scheme, c dt / dx, exponent): boundaries (2, 1), the hot start, stiffness 1
REGIME_POINTS = [(ts, cfl, n) for ts in (1, 2, 3) for cfl in REGIME_CFL for n in REGIME_EXPONENTS]
# Where the truth itself has T < 0 after a step -- point: {step: min T}, measured and asserted:
# BDF2 at c dt / dx = 1e2 grows the state on this slab without the law too
# (material_regime_cases.ROOT_SOLVED); with the cold-opaque law it turns T negative in 16 cells in
# the sixth step.  The point is kept and compared like every other: the device has to follow the
# reference there too (T <= 0: B = 0, the ratio T / T_ref counts as 0+).
REGIME_NEGATIVE_T = {(3, 1e2, 3.0): {6: -6.38}}
_regime = {}


def law_regime_case(oracle_mod, pt):
    """material_regime_cases.coupled_case's region branch with the law on: (CoupledCase, the law's
    arguments).  Every region takes the exponent, with T_ref its own T, so f = 1 at the region's
    radiation temperature and 3^-n at the hot start."""
    if pt in _regime:
        return _regime[pt]
    import material_regime_cases as mc
    import regime_cases as rc
    ts, cfl, n = pt
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
    law = ([n] * len(regions), [r["T"] for r in regions]) + REGIME_BOUNDS
    truth = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0, dtype=np.longdouble, law=law)
    stiff0 = np.asarray(p["dt"] * truth.W * truth.bpart / truth.rho_cv_cells, dtype=np.float64)
    truth.material_step(mc.STEPS)
    ref = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0, law=law)
    ref.material_step(mc.STEPS)
    same = all(np.array_equal(a["solved"], b["solved"]) for a, b in zip(ref.history, truth.history))
    tr = mc.coupled_readouts(truth)
    Tn = np.asarray(tr["T"], dtype=np.float64)
    w_sigma = p["dt"] * W * np.asarray(truth.sigma_cells, dtype=np.float64)
    case = mc.CoupledCase(p, rc.to_rt(p), regions, rho_cv, T0, mc.STEPS, tr, mc.coupled_readouts(ref),
                          {"slab": np.arange(N)}, mc.rounding_floor(Tn, e, 0, rc.G), w_sigma, truth.history, same,
                          stiff0)
    _regime[pt] = (case, law)
    return _regime[pt]


def _needs_extended():
    import regime_cases as rc
    return pytest.mark.skipif(not rc.HAVE_EXTENDED, reason=rc.SKIP_REASON)


@_needs_extended()
@pytest.mark.parametrize("pt", REGIME_POINTS, ids=lambda pt: f"{pt[0]}-{pt[1]:g}-n{pt[2]:g}")
def test_regime_reference_within_a_quarter_of_K(oracle_mod, pt):
    """Every point kept: the truth is finite with T > 0, the fp64 reference takes the truth's
    branches, its own T is within ORACLE_ERR_MAX, and -- measured as the device will be, against
    max(its own error, 16 eps) scaled by 4 -- it stays within K / 4."""
    import material_regime_cases as mc
    import regime_cases as rc
    case, law = law_regime_case(oracle_mod, pt)
    assert case.branch_same
    T = np.asarray(case.truth["T"], dtype=np.float64)
    assert np.isfinite(T).all() and (T != 0).all()
    for k, h in enumerate(case.history):  # T > 0 after every step but where listed
        want = REGIME_NEGATIVE_T.get(pt, {}).get(k + 1)
        Tmin = float(np.asarray(h["T"], dtype=np.float64).min())
        assert (Tmin > 0) if want is None else (Tmin == pytest.approx(want, rel=1e-3)), (pt, k + 1, Tmin)
    errT = np.abs(np.asarray(case.oracle["T"], dtype=np.longdouble) - case.truth["T"]) / np.abs(case.truth["T"])
    assert float(errT.max()) <= rc.ORACLE_ERR_MAX
    ratios = mc.coupled_ratios(mc.coupled_readouts(_Fp64(case)), case)
    for k, v in ratios.items():
        assert (np.asarray(v) <= rc.K / 4).all(), (pt, k, float(np.max(v)))


class _Fp64:
    """The fp64 reference's read-outs under a solver's accessor names (it measures 1 against itself)."""

    def __init__(self, case):
        self.o = case.oracle

    def temperature(self):
        return np.asarray(self.o["T"], dtype=np.float64)

    def cell_emission(self):
        return np.asarray(self.o["Beff"], dtype=np.float64).T

    def material_transit(self):
        return np.asarray(self.o["transit"], dtype=np.float64)

    def ends(self):
        return np.asarray(self.o["ends"], dtype=np.float64)

"""The temperature-dependent opacity in chain mode, on the CPU: the conditions the GPU cases of
tests/test_opacity_chain_gpu.py rest on, asserted on the fp64 references alone (as
tests/test_opacity_law.py::test_case_conditions does for the line walk's cases), and the entry
points' declarations.

For every (layout, law or table, scheme, boundary pair) the GPU file compares with a reference:
T > 0 and Beff >= 0 after every step; finite ends; f_0 spans a decade; no clamp reached, or for
`clamped` both clamps active at the start and again later; f moves; cells on the Newton path and on
the linear path; no dT / T within 1e-6 of the switch at 0.25; BE: the energy residual at most 1e-12
of the total every step (tests/test_material.py's bound).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import opacity_chain_cases as occ
import opacity_law_ref as olr


def _paths(ref):
    solved = sum(int(h["solved"].sum()) for h in ref.history)
    linear = sum(int((~h["solved"]).sum()) for h in ref.history)
    near = min(float(np.abs(h["ratio"] - 0.25).min()) for h in ref.history)
    return solved, linear, near


@pytest.mark.parametrize("layout,law,ts,bc", occ.LAW_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_law_case_conditions(oracle_mod, layout, law, ts, bc):
    r = occ.reference_run(oracle_mod, layout, law, ts, bc)
    ref = r["ref"]
    assert min(r["Tmin"]) > 0.0 and min(r["Bmin"]) >= 0.0
    assert np.isfinite(ref.ends()).all()
    lo, hi = olr.LAWS[law]["bounds"]
    assert r["f0"].max() >= 10.0 * r["f0"].min(), (r["f0"].min(), r["f0"].max())
    if law == "clamped":  # both clamps active, at the start and again later
        assert r["f0"].min() == lo and r["f0"].max() == hi
        assert any(f.min() == lo for f in r["f"][1:]) and any(f.max() == hi for f in r["f"][1:])
    else:
        for f in r["f"]:
            assert lo < f.min() and f.max() < hi  # no clamp reached
    assert not np.array_equal(r["f"][0], r["f"][-1])  # the opacity does move with T
    solved, linear, near = _paths(ref)
    print(layout, law, ts, bc, dict(solved=solved, linear=linear, near=near, resid=float(np.abs(r["resid"]).max())))
    assert solved > 0 and linear > 0, (solved, linear)
    assert near > 1e-6, near
    if ts == 1:
        assert np.abs(r["resid"]).max() <= 1e-12, r["resid"]


@pytest.mark.parametrize("layout,table,ts,bc", occ.TABLE_PARITY, ids=lambda v: str(v).replace(" ", ""))
def test_table_case_conditions(oracle_mod, layout, table, ts, bc):
    """opacity_table_ref's `edge` table on (20, 24) cells: tests/test_opacity_table.py's conditions
    but the bracket crossing, which that file asserts on its own layouts."""
    r = occ.reference_run(oracle_mod, layout, table, ts, bc, kind="table")
    ref = r["ref"]
    assert min(r["Tmin"]) > 0.0 and min(r["Bmin"]) >= 0.0
    assert np.isfinite(ref.ends()).all()
    f0 = r["f0"]
    assert f0.shape == (ref.N, ref.G)
    assert f0.max(axis=0).max() >= 10.0 * f0.min(axis=0).min()   # over the cells
    assert (f0.max(axis=1) / f0.min(axis=1)).max() >= 10.0       # over the groups within one cell
    assert not np.array_equal(r["f"][0], r["f"][-1])
    solved, linear, near = _paths(ref)
    print(layout, table, ts, bc, dict(solved=solved, linear=linear, near=near, resid=float(np.abs(r["resid"]).max())))
    assert solved > 0 and linear > 0, (solved, linear)
    assert near > 1e-6, near
    if ts == 1:
        assert np.abs(r["resid"]).max() <= 1e-12, r["resid"]


def test_layouts_reach_what_they_are_for(rtsn_mod):
    """The chains the GPU cases count on, from the host-only planner at one step (the coupled
    handle's rule): c12 admits one cell per lane only; c336 at one cell per lane is 6 waves (the
    wide chain), its reflective pair fits 8 waves from 2 cells per lane on; c12 and c44 admit no
    segments, n80 and c336 do."""
    def regions(layout):
        return [dict(cells=c, width=1.0, rho=1.0, kappa_grey=1.0, T=1.0) for c in occ.LAYOUTS[layout]["cells"]]

    for refl in (False, True):
        got = rtsn_mod.regions_plan(regions("c12"), reflective=refl, nsteps=1)
        assert (got["cells_per_lane"], got["waves"], got["lanes"]) == (1, 1, 12)
    for layout in ("c12", "c44"):
        with pytest.raises(rtsn_mod.RtError):
            rtsn_mod.regions_plan_segments(regions(layout), 16)
    for layout in ("n80", "c336"):
        assert rtsn_mod.regions_plan_segments(regions(layout), 16)["segments"] == sum(occ.LAYOUTS[layout]["cells"]) // 16
    assert all(c % 4 == 0 for c in occ.LAYOUTS["c44"]["cells"] + occ.LAYOUTS["c336"]["cells"])
    assert -(-336 // 64) == 6 and -(-2 * 168 // 64) == 6 and -(-84 // 64) == 2 and -(-168 // 64) == 3


def test_entry_points_declared_and_exported(rtsn_mod):
    names = rtsn_mod.exported_symbols()
    L = rtsn_mod.lib()
    for f in ("rt_material_set_opacity_law_chain", "rt_material_set_opacity_table_chain"):
        assert f in names and hasattr(L, f)
    law, tab = L.rt_material_set_opacity_law_chain, L.rt_material_set_opacity_table_chain
    dp = C.POINTER(C.c_double)
    assert list(law.argtypes) == [C.c_void_p, dp, dp, C.c_int, C.c_double, C.c_double]
    assert list(tab.argtypes) == [C.c_void_p, dp, C.c_int, dp, C.c_int]
    # without a handle (no GPU needed): RT_ERR_ARG
    a = (C.c_double * 2)(1.0, 1.0)
    assert law(None, a, a, 2, 1e-3, 1e3) == 8
    assert tab(None, a, 2, a, 1) == 8
    assert hasattr(rtsn_mod.Solver, "material_set_opacity_law_chain")
    assert hasattr(rtsn_mod.Solver, "material_set_opacity_table_chain")

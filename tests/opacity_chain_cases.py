"""The cases of the temperature-dependent opacity in chain mode (rt_material_set_opacity_law_chain,
rt_material_set_opacity_table_chain; the law form of the wavefront chain, kernels_wave.hip),
shared by tests/test_opacity_chain.py (the conditions, on the fp64 references alone) and
tests/test_opacity_chain_gpu.py.

The medium is tests/opacity_law_ref.py's (DXS, RHO, RHO_CV, T_REGION, SCHEME_DT, LAWS, STEPS, BCS),
the references are OpacityLawReference and tests/opacity_table_ref.py's OpacityTableReference; the
layouts are the chain's:

  c12       (5, 7)      edges on no multiple of 2: one cell per lane only, one wave; the reflective
                        pair is 24 lanes.  No segment plan exists for it
  c12_wide  (5, 7)      M = 8, G = 17: 68 lines per half, group index up to 16
  c44       (20, 24)    1, 2 and 4 cells per lane admissible; not admissible for segments
  n80       (32, 48)    also admissible for segments: the line walk is the yardstick
  c336      (160, 176)  one cell per lane: 336 lanes = 6 waves, the wide chain (reflective: 2 cells per
                        lane, 6 waves); 4 per lane: 84 lanes = 2 waves, reflective 168 = 3 waves.
                        Also admissible for segments
"""
from __future__ import annotations

import numpy as np

import opacity_law_ref as olr
import opacity_table_ref as otr

STEPS, BCS, SCHEME_DT = olr.STEPS, olr.BCS, olr.SCHEME_DT

LAYOUTS = {
    "c12": dict(cells=(5, 7), MG=(6, 5)),
    "c12_wide": dict(cells=(5, 7), MG=(8, 17)),
    "c44": dict(cells=(20, 24), MG=(6, 5)),
    "n80": dict(cells=(32, 48), MG=(6, 5)),
    "c336": dict(cells=(160, 176), MG=(6, 5)),
}

SCHEMES = (1, 2, 3)
# 1: parity with the law reference -- (layout, law, scheme, boundary pair)
LAW_PARITY = [(lay, law, ts, bc)
              for lay, law in (("c12", "marshak"), ("c12", "mixed"), ("c44", "marshak"), ("c44", "mixed"),
                               ("c44", "clamped"))
              for ts in SCHEMES for bc in BCS] + [("c12_wide", "marshak", 3, (2, 1))]
# 2: the chains of several waves
MULTI_WAVE = [("c336", "marshak", ts, bc) for ts in SCHEMES for bc in ((0, 0), (2, 1))]
# 4: against the line walk of a segment-mode handle (c336's cases are MULTI_WAVE's)
WALK = [("n80", "marshak", ts, bc) for ts in SCHEMES for bc in ((0, 0), (2, 1))] + MULTI_WAVE
# 7: parity with the table reference, opacity_table_ref's `edge` table
TABLE_PARITY = [("c44", "edge", ts, bc) for ts in SCHEMES for bc in BCS]
# every law case a GPU test compares with a reference run
LAW_CASES = LAW_PARITY + MULTI_WAVE + [c for c in WALK if c not in MULTI_WAVE]


def case(oracle_mod, layout, ts, bc):
    """(p, regions, rho_cv, T0) of a layout: opacity_law_ref.case over LAYOUTS, the same medium."""
    from test_material import params
    L = LAYOUTS[layout]
    M, G = L["MG"]
    cells = L["cells"]
    p = params(oracle_mod, ts=ts, dt=SCHEME_DT[ts], M=M, G=G, N=int(sum(cells)), bc_left=bc[0], bc_right=bc[1])
    p["psi_source"] = np.linspace(0.5, 2.0, M * G).reshape(M, G)
    regions = [dict(cells=int(c), width=float(c * d), rho=float(r), kappa_grey=p["kappa_grey"], T=float(t),
                    group_kappa=None) for c, d, r, t in zip(cells, olr.DXS, olr.RHO, olr.T_REGION)]
    return p, regions, olr.RHO_CV, olr.t_cells(cells)


def energy_terms(regions, rho_cv):
    """(dx, rho_cv) per cell."""
    creg = np.repeat(np.arange(len(regions)), [r["cells"] for r in regions])
    return (np.array([r["width"] / r["cells"] for r in regions])[creg], np.asarray(rho_cv, dtype=np.float64)[creg])


_runs = {}


def reference_run(oracle_mod, layout, name, ts, bc, kind="law", g_lo=0, g_hi=0):
    """One fp64 reference run of STEPS steps per case, computed once and left unchanged, as
    opacity_law_ref.reference_run / opacity_table_ref.reference_run record it: the reference after
    the last step, the f it started from ((N), or (N, G) for kind "table"), and per step f, the BE
    residual relative to the total, min T and min Beff."""
    key = (layout, name, ts, bc, kind, g_lo, g_hi)
    if key not in _runs:
        from test_material import net_outflow
        p, regions, rho_cv, T0 = case(oracle_mod, layout, ts, bc)
        if kind == "table":
            ref = otr.OpacityTableReference(oracle_mod, p, regions, rho_cv, T0, g_lo=g_lo, g_hi=g_hi,
                                            table=otr.table_args(name, p["G"]))
            f_of = lambda: ref.f.copy()  # noqa: E731
        else:
            ref = olr.OpacityLawReference(oracle_mod, p, regions, rho_cv, T0, g_lo=g_lo, g_hi=g_hi,
                                          law=olr.law_args(name))
            f_of = ref.opacity_scale
        dx, rcv = ref.dx_cells, np.asarray(ref.rho_cv_cells, dtype=np.float64)
        rec = dict(ref=ref, p=p, regions=regions, rho_cv=rho_cv, T0=T0, f0=f_of(), f=[f_of()], resid=[], Tmin=[],
                   Bmin=[])
        view = olr._RefView(ref)
        for _ in range(STEPS):
            e0 = olr.energy(ref, dx, rcv)
            ref.material_step(1)
            e1 = olr.energy(ref, dx, rcv)
            rec["resid"].append(((e1 - e0) + p["dt"] * net_outflow(view, p)) / e1)
            rec["f"].append(f_of())
            rec["Tmin"].append(float(ref.temperature().min()))
            rec["Bmin"].append(float(ref.cell_emission().min()))
        _runs[key] = rec
    return _runs[key]

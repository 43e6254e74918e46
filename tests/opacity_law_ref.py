"""Numpy restatement of the temperature-dependent opacity of the material coupling
(include/rtsn.h rt_material_set_opacity_law) -- TEST INFRASTRUCTURE ONLY.

regions_material_ref.RegionMaterialReference with, per cell x of region k,

    sigma_g(x) = sigma0_{k,g} f(x),   f = clamp((T(x) / T_ref[k])^(-exponent[k]), lo, hi),

T <= 0 or not finite counting as a ratio of 0+.  The opacity is lagged: f is formed from T^n
(when the law is set and in every _planck, which runs after an update) and everything in step n
uses it:

* the sweep builds ONE unit LineSet per cell from sigma0 f (the constants of fused_np.LineSet,
  in the reference's dtype), its constant Sc multiplied by the cell's Beff as in the parent;
* q, b, the S(T') of the root and material_transit read sigma_cells / sigma_all_cells, which
  hold sigma0 f;
* the owed emission is kept in B units (its energy is dt W sigma_g owed_g): _planck multiplies
  the finalised owed emission owed + dB dTlast by f_old / f_new before the payment
  p = max(owed, -B) is taken; set_law (the law set, changed or cleared in mid-run) does the same
  to the emission in transit (Beff - B) + owed and pays it again by the same rule.

With exponent 0 everywhere f = 1 and every operation above is the parent's, bitwise.
Works in any dtype the parent does (np.longdouble: the truth of the regime family).

The cases the CPU and the GPU tests share, and one cached reference run per case, are at the
end of the file.
"""
from __future__ import annotations

import numpy as np

from regions_material_ref import RegionMaterialReference


class _LawCellSets:
    """sets[k] for RegionReference._sweep: the unit LineSet of upwind cell k, from the cell's
    own sigma0 f, its constant scaled by the cell's emission."""

    def __init__(self, ref, half):
        self.ref, self.half = ref, half

    def __getitem__(self, k):
        import fused_np
        ref = self.ref
        x = ref.N - 1 - k if self.half == 0 else k
        I, Gi = ref.idx[self.half]
        zeros = np.zeros(len(I))
        p = ref.p
        ls = fused_np.LineSet(ref.mu[I], ref.sigma_cells[x, Gi], np.ones(len(I)), zeros, zeros, zeros, 0.0,
                              ref.dx_cells[x], p["dt"], p["ts_method"], False, dtype=ref.dtype)
        ls.Sc = ls.Sc * ref.Beff[x, Gi]
        return ls


class OpacityLawReference(RegionMaterialReference):
    def __init__(self, oracle_mod, p, regions, rho_cv, T_cells=None, g_lo=0, g_hi=0, dtype=np.float64, law=None):
        """law: None, or (exponent per region, T_ref per region, scale_min, scale_max), set
        before any step."""
        self.law = None
        super().__init__(oracle_mod, p, regions, rho_cv, T_cells, g_lo, g_hi, dtype)
        self.sigma0_cells = self.sigma_cells.copy()
        self.sigma0_all_cells = self.sigma_all_cells.copy()
        self.map_lines = dict(self.lines)  # the parent's per-region sets (the law off)
        self.f = np.ones(self.N, dtype=self.dtype)
        if law is not None:
            self.set_law(*law)

    # ---- the law ----
    def _scale(self, T):
        f = self.dtype
        n, Tref, lo, hi = self.law
        n, Tref = n[self.cell_region], Tref[self.cell_region]
        with np.errstate(all="ignore"):
            v = np.power(T / Tref, -n)
        cold = ~((T > 0) & np.isfinite(T))
        v = np.where(cold, np.where(n > 0, hi, np.where(n < 0, lo, f(1))), v)
        return np.minimum(np.maximum(v, lo), hi).astype(f)

    def _apply(self, f_new):
        self.f = f_new
        self.sigma_cells = self.sigma0_cells * f_new[:, None]
        self.sigma_all_cells = self.sigma0_all_cells * f_new[:, None]

    def set_law(self, exponent, T_ref, scale_min, scale_max):
        """The law set, changed or (exponent None) cleared: f from the current T, the emission
        in transit rescaled by f_old / f_new and paid again."""
        f = self.dtype
        if exponent is None:
            self.law = None
            f_new = np.ones(self.N, dtype=f)
        else:
            self.law = (np.asarray(exponent, dtype=np.float64).astype(f), np.asarray(T_ref, dtype=np.float64).astype(f),
                        f(scale_min), f(scale_max))
            f_new = self._scale(self.T)
        B = self.Bcell
        owed = (self.owed + (self.Beff - B)) * (self.f / f_new)[:, None]
        pay = np.where(owed > -B, owed, -B)
        self.owed, self.Beff = owed - pay, B + pay
        self._apply(f_new)
        b = np.zeros(self.N, dtype=f)
        for gl in range(self.Gl):
            b = b + self.sigma_cells[:, gl] * self.dB[:, gl]
        self.bpart = b
        for half in (0, 1):
            self.lines[half] = self.map_lines[half] if self.law is None else _LawCellSets(self, half)

    def _planck(self):
        if self.law is not None:
            f_new = self._scale(self.T)
            # the finalised owed emission, rescaled; the parent then adds dB x 0 and pays
            self.owed = (self.owed + self.dB * self.dTlast[:, None]) * (self.f / f_new)[:, None]
            self.dTlast = np.zeros_like(self.dTlast)
            self._apply(f_new)
        super()._planck()

    # ---- read-outs ----
    def opacity_scale(self):
        return self.f.copy()

    def group_absorption(self):
        return (self.sigma_cells * self.moments()[0].T).sum(axis=1)


# ---------------------------------------------------------------------------
# the shared cases
# ---------------------------------------------------------------------------
C_LIGHT = 299.79245800
SCHEME_DT = {1: 1e-3, 2: 1e-3, 3: 1e-4}   # tests/test_regions_material_gpu.py
BCS = [(0, 0), (2, 1), (1, 1)]
STEPS = 6
WIDE = (1e-3, 1e3)                        # bounds no cell of a case reaches

# name: cells, cells per segment, segments, (M, G), exponents, T_ref, (scale_min, scale_max)
LAYOUTS = {
    "n80": dict(cells=(32, 48), seg=16, segments=5, MG=(6, 5)),
    "n32": dict(cells=(16, 16), seg=16, segments=2, MG=(6, 5)),
    "n32_wide": dict(cells=(16, 16), seg=16, segments=2, MG=(8, 17)),   # 68 lines per half
}
LAWS = {
    "marshak": dict(exponent=(3.0, 1.5), T_ref=(1.0, 0.5), bounds=WIDE),
    "mixed": dict(exponent=(-1.0, 0.0), T_ref=(0.1, 0.5), bounds=WIDE),
    "clamped": dict(exponent=(3.0, 1.5), T_ref=(1.0, 0.5), bounds=(0.4, 5.0)),
    "zero": dict(exponent=(0.0, 0.0), T_ref=(1.0, 0.5), bounds=WIDE),
}
# (layout, law) pairs of the parity family; every one runs BE / CN / BDF2 x BCS
PARITY = [("n80", "marshak"), ("n80", "mixed"), ("n80", "clamped"), ("n32", "marshak"), ("n32", "mixed")]
WIDE_CASE = ("n32_wide", "marshak", 3, (2, 1))
DXS, RHO, RHO_CV = (0.016, 0.004), (0.2, 10.0), (5.0, 0.5)


T_REGION = (1.5, 0.05)


def t_cells(cells):
    """A cold start: T falls geometrically from 1.5 keV at the left to 0.05 keV at the right, so
    that f spans decades, hot cells take the linear update and cold ones solve the root."""
    return np.repeat(T_REGION, cells).astype(float)


def case(oracle_mod, layout, ts, bc):
    """(p, regions, rho_cv, T0) of a layout: test_regions_material_segments_gpu._case's medium."""
    from test_material import params
    L = LAYOUTS[layout]
    M, G = L["MG"]
    cells = L["cells"]
    p = params(oracle_mod, ts=ts, dt=SCHEME_DT[ts], M=M, G=G, N=int(sum(cells)), bc_left=bc[0], bc_right=bc[1])
    p["psi_source"] = np.linspace(0.5, 2.0, M * G).reshape(M, G)
    regions = [dict(cells=int(c), width=float(c * d), rho=float(r), kappa_grey=p["kappa_grey"], T=float(t),
                    group_kappa=None) for c, d, r, t in zip(cells, DXS, RHO, T_REGION)]
    return p, regions, RHO_CV, t_cells(cells)


def law_args(law):
    w = LAWS[law]
    return (w["exponent"], w["T_ref"]) + tuple(w["bounds"])


def energy(s, dx_cells, rho_cv_cells):
    from regions_material_ref import region_energy
    return region_energy(s, dx_cells, rho_cv_cells, C_LIGHT)


_runs = {}


def reference_run(oracle_mod, layout, law, ts, bc, g_lo=0, g_hi=0):
    """One fp64 reference run of STEPS steps per case, computed once and left unchanged: the
    reference after the last step, the f it started from, and per step f's range, the BE
    residual relative to the total, min T and min Beff."""
    key = (layout, law, ts, bc, g_lo, g_hi)
    if key not in _runs:
        from test_material import net_outflow
        p, regions, rho_cv, T0 = case(oracle_mod, layout, ts, bc)
        ref = OpacityLawReference(oracle_mod, p, regions, rho_cv, T0, g_lo=g_lo, g_hi=g_hi, law=law_args(law))
        dx, rcv = ref.dx_cells, np.asarray(ref.rho_cv_cells, dtype=np.float64)
        rec = dict(ref=ref, p=p, regions=regions, rho_cv=rho_cv, T0=T0, f0=ref.opacity_scale(), f=[ref.opacity_scale()],
                   resid=[], Tmin=[], Bmin=[])
        view = _RefView(ref)
        for _ in range(STEPS):
            e0 = energy(ref, dx, rcv)
            ref.material_step(1)
            e1 = energy(ref, dx, rcv)
            rec["resid"].append(((e1 - e0) + p["dt"] * net_outflow(view, p)) / e1)
            rec["f"].append(ref.opacity_scale())
            rec["Tmin"].append(float(ref.temperature().min()))
            rec["Bmin"].append(float(ref.cell_emission().min()))
        _runs[key] = rec
    return _runs[key]


class _RefView:
    """test_material.net_outflow's view of a reference (ends, quad, psi_source as methods)."""

    def __init__(self, ref):
        self.ref = ref

    def ends(self):
        return self.ref.ends()

    def quad(self):
        return self.ref.quad()

    def psi_source(self):
        return np.asarray(self.ref.psi_source)

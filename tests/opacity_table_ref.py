"""Numpy restatement of the tabulated per-group opacities of the material coupling
(include/rtsn.h rt_material_set_opacity_table) -- TEST INFRASTRUCTURE ONLY.

opacity_law_ref.OpacityLawReference with, per cell x of region k and group g,

    sigma_g(x) = sigma0_{k,g} f_{k,g}(T(x)),

f given at the nodes T_0 < ... < T_{nT-1} as scale[k, j, g] over ALL G groups, linear in
(ln T, ln f) between the nodes and constant outside: with j the bracket of T,

    t = log(T / T_j) r_j,   r_j = 1 / log(T_{j+1} / T_j),   f = exp(t (ln f_{j+1} - ln f_j) + ln f_j)

(the header's fma written as a product and a sum: numpy has no fma; the difference is one
rounding of t x the difference, below the bound the GPU test states).  T below the first node,
T <= 0 or T not finite: t = 0 at the first node; T at or above the last node: t = 0 at the last.
r_j and ln f_j are formed in np.longdouble and rounded once to the reference's dtype, as the
library forms them in long double on the host; everything else runs in the reference's dtype.

f is held as (N, G).  It is lagged and conserved as the law's, per group: _planck multiplies the
finalised owed emission of group g by f_old,g / f_new,g before the payment, set_table and set_law
(the table or the law set, changed, replaced by the other or cleared in mid-run) do the same to
the emission in transit and pay it again.  The table and the law exclude each other.  With an
all-ones table every operation is the parent's with the law off, bitwise.  Works with group
shards (g_lo, g_hi) and in np.longdouble.

The cases the CPU and the GPU tests share, and one cached reference run per case, are at the
end of the file.
"""
from __future__ import annotations

import numpy as np

import opacity_law_ref as olr
from opacity_law_ref import OpacityLawReference, _LawCellSets, _RefView
from regions_material_ref import RegionMaterialReference


class OpacityTableReference(OpacityLawReference):
    def __init__(self, oracle_mod, p, regions, rho_cv, T_cells=None, g_lo=0, g_hi=0, dtype=np.float64, table=None,
                 law=None):
        """table: None, or (T_grid (nT), scale (regions, nT, G)), set before any step; law: the
        parent's (not with a table)."""
        assert table is None or law is None
        self.table = None
        super().__init__(oracle_mod, p, regions, rho_cv, T_cells, g_lo, g_hi, dtype, law=law)
        if table is not None:
            self.set_table(*table)

    # ---- the table ----
    def _own(self, f):
        """f of the handle's own groups, (N, Gl) or broadcastable to it."""
        return f[:, None] if f.ndim == 1 else f[:, self.g_lo:self.g_lo + self.Gl]

    def bracket(self, T):
        """(j, inside): the node whose value or interval a cell takes, and whether it interpolates."""
        Tg = self.table[0]
        nT = len(Tg)
        with np.errstate(all="ignore"):
            ok = (T > 0) & np.isfinite(T) & (T >= Tg[0])
            top = ok & (T >= Tg[-1])
        inside = ok & ~top
        j = np.clip(np.searchsorted(Tg, np.where(inside, T, Tg[0]), side="right") - 1, 0, nT - 2)
        return np.where(top, nT - 1, np.where(inside, j, 0)), inside

    def _scale_table(self, T):
        f = self.dtype
        Tg, r, lnf = self.table
        nT = len(Tg)
        j, inside = self.bracket(T)
        jr = np.minimum(j, nT - 2)
        t = np.where(inside, np.log(np.where(inside, T, Tg[j]) / Tg[j]) * r[jr], f(0))
        l0 = lnf[self.cell_region, j]
        l1 = lnf[self.cell_region, np.minimum(j + 1, nT - 1)]
        return np.exp(t[:, None] * (l1 - l0) + l0).astype(f)

    def _apply(self, f_new):
        if f_new.ndim == 1:
            return super()._apply(f_new)
        self.f = f_new
        self.sigma_cells = self.sigma0_cells * self._own(f_new)
        self.sigma_all_cells = self.sigma0_all_cells * f_new

    def _transition(self, f_new):
        """f_new ((N) or (N, G)) comes into force: the emission in transit rescaled per group by
        f_old / f_new and paid again, bpart and the sweep's line sets with the new opacities."""
        f = self.dtype
        B = self.Bcell
        owed = (self.owed + (self.Beff - B)) * (self._own(self.f) / self._own(f_new))
        pay = np.where(owed > -B, owed, -B)
        self.owed, self.Beff = owed - pay, B + pay
        self._apply(f_new)
        b = np.zeros(self.N, dtype=f)
        for gl in range(self.Gl):
            b = b + self.sigma_cells[:, gl] * self.dB[:, gl]
        self.bpart = b
        plain = self.law is None and self.table is None
        for half in (0, 1):
            self.lines[half] = self.map_lines[half] if plain else _LawCellSets(self, half)

    def set_table(self, T_grid, scale):
        """The table set, changed or (T_grid None) cleared; a law in force is replaced."""
        f = self.dtype
        self.law = None
        if T_grid is None:
            self.table = None
            return self._transition(np.ones(self.N, dtype=f))
        L = np.longdouble
        Tg = np.asarray(T_grid, dtype=np.float64)
        sc = np.asarray(scale, dtype=np.float64)
        assert sc.shape == (len(self.tables), Tg.size, self.G) and Tg.size >= 2
        assert (np.diff(Tg) > 0).all() and Tg[0] > 0 and np.isfinite(Tg).all() and (sc > 0).all() and np.isfinite(sc).all()
        r = (L(1) / np.log(Tg[1:].astype(L) / Tg[:-1].astype(L))).astype(f)
        self.table = (Tg.astype(f), r, np.log(sc.astype(L)).astype(f))
        self._transition(self._scale_table(self.T))

    def set_law(self, exponent, T_ref, scale_min, scale_max):
        """The parent's, from any state: with the table on, the law replaces it (exponent None
        leaves it, as the library does: the law is off already)."""
        f = self.dtype
        if exponent is None:
            if self.table is not None:
                return
            self.law = None
            return self._transition(np.ones(self.N, dtype=f))
        self.table = None
        self.law = (np.asarray(exponent, dtype=np.float64).astype(f), np.asarray(T_ref, dtype=np.float64).astype(f),
                    f(scale_min), f(scale_max))
        self._transition(self._scale(self.T))

    def _planck(self):
        if self.table is None:
            return super()._planck()
        f_new = self._scale_table(self.T)
        # the finalised owed emission, rescaled per group; the plain pass then adds dB x 0 and pays
        self.owed = (self.owed + self.dB * self.dTlast[:, None]) * (self._own(self.f) / self._own(f_new))
        self.dTlast = np.zeros_like(self.dTlast)
        self._apply(f_new)
        RegionMaterialReference._planck(self)

    # ---- read-outs ----
    def opacity_scale_groups(self):
        """(N, Gl) f of the handle's groups, in every state."""
        return np.broadcast_to(self._own(self.f), (self.N, self.Gl)).copy()


# ---------------------------------------------------------------------------
# the shared cases
# ---------------------------------------------------------------------------
STEPS, BCS, SCHEME_DT = olr.STEPS, olr.BCS, olr.SCHEME_DT
# opacity_law_ref's layouts and one with more groups than a wave has lanes: the table kernel's
# group loop takes two turns and a wave of the walk spans a group edge (H = 1: one line per group)
LAYOUTS = dict(olr.LAYOUTS, g70=dict(cells=(16, 16), seg=16, segments=2, MG=(2, 70)))
G70_CASE = ("g70", 3, (2, 1))
WIDE_CASE = ("n32_wide", 3, (2, 1))
EDGE_GRID = (0.03, 0.06, 0.3, 1.3, 2.0)
EDGE_TREF = (1.0, 0.5)
EDGE_KINK = 1.7


def case(oracle_mod, layout, ts, bc):
    """opacity_law_ref.case over LAYOUTS: the same medium, DXS, RHO, RHO_CV and T_REGION."""
    from test_material import params
    L = LAYOUTS[layout]
    M, G = L["MG"]
    cells = L["cells"]
    p = params(oracle_mod, ts=ts, dt=SCHEME_DT[ts], M=M, G=G, N=int(sum(cells)), bc_left=bc[0], bc_right=bc[1])
    p["psi_source"] = np.linspace(0.5, 2.0, M * G).reshape(M, G)
    regions = [dict(cells=int(c), width=float(c * d), rho=float(r), kappa_grey=p["kappa_grey"], T=float(t),
                    group_kappa=None) for c, d, r, t in zip(cells, olr.DXS, olr.RHO, olr.T_REGION)]
    return p, regions, olr.RHO_CV, olr.t_cells(cells)


def edge_exponents(G, nregions=2):
    """n_{k,g}: from 3.5 to 0.5 over the groups in region 0, from 1.5 to 0 in region 1 (a third
    region, the regime family's, from 2.5 to 0.25)."""
    return np.stack([np.linspace(3.5, 0.5, G), np.linspace(1.5, 0.0, G), np.linspace(2.5, 0.25, G)][:nregions])


def edge_table(G, T_ref=EDGE_TREF, grid=EDGE_GRID):
    """f_{k,g}(T_j) = (T_j / T_ref,k)^(-n_{k,g}), node 2 then times 1.7 for odd g: a kink no power
    law has.  Lines of one cell differ by decades (n from 3.5 to 0.5) and respond differently to T."""
    Tg = np.asarray(grid, dtype=np.float64)
    n = edge_exponents(G, len(T_ref))
    sc = (Tg[None, :, None] / np.asarray(T_ref, dtype=np.float64)[:, None, None]) ** (-n[:, None, :])
    sc[:, 2, 1::2] *= EDGE_KINK
    return Tg, sc


def as_law_table(G, law="clamped"):
    """The clamped power law written as a table: the nodes are the four temperatures at which
    either region's law meets a clamp, T_ref c^(-1/n) for c in the bounds; the scale is the law at
    the nodes, repeated over the groups.  (Between its clamps a power law is linear in log-log, and
    the other region's nodes lie on that line.)"""
    w = olr.LAWS[law]
    n, Tref, (lo, hi) = np.asarray(w["exponent"]), np.asarray(w["T_ref"]), w["bounds"]
    Tg = np.sort(np.concatenate([Tref * c ** (-1.0 / n) for c in (lo, hi)]))
    sc = np.clip((Tg[None, :] / Tref[:, None]) ** (-n[:, None]), lo, hi)
    return Tg, np.repeat(sc[:, :, None], G, axis=2)


TABLES = {"edge": edge_table, "as_law": as_law_table, "ones": lambda G: (np.array([0.1, 1.0]), np.ones((2, 2, G)))}


def table_args(name, G):
    return TABLES[name](G)


_runs = {}


def reference_run(oracle_mod, layout, table, ts, bc, g_lo=0, g_hi=0):
    """One fp64 reference run of STEPS steps per case, computed once and left unchanged: the
    reference after the last step, the f (N, G) it started from, and per step f, every cell's
    bracket, the BE residual relative to the total, min T and min Beff."""
    key = (layout, table, ts, bc, g_lo, g_hi)
    if key not in _runs:
        from test_material import net_outflow
        p, regions, rho_cv, T0 = case(oracle_mod, layout, ts, bc)
        ref = OpacityTableReference(oracle_mod, p, regions, rho_cv, T0, g_lo=g_lo, g_hi=g_hi,
                                    table=table_args(table, p["G"]))
        dx, rcv = ref.dx_cells, np.asarray(ref.rho_cv_cells, dtype=np.float64)
        rec = dict(ref=ref, p=p, regions=regions, rho_cv=rho_cv, T0=T0, f0=ref.f.copy(), f=[ref.f.copy()],
                   bracket=[ref.bracket(ref.T)[0]], resid=[], Tmin=[], Bmin=[])
        view = _RefView(ref)
        for _ in range(STEPS):
            e0 = olr.energy(ref, dx, rcv)
            ref.material_step(1)
            e1 = olr.energy(ref, dx, rcv)
            rec["resid"].append(((e1 - e0) + p["dt"] * net_outflow(view, p)) / e1)
            rec["f"].append(ref.f.copy())
            rec["bracket"].append(ref.bracket(ref.T)[0])
            rec["Tmin"].append(float(ref.temperature().min()))
            rec["Bmin"].append(float(ref.cell_emission().min()))
        _runs[key] = rec
    return _runs[key]
